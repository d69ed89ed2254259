"""The stochastic e-folds on the host build (tests/stochastic_twin.cpp compiles csrc/inflx_stochastic.h and csrc/inflx_philox.h for the
CPU): the random numbers against their known answers and their law, the generated noise header against sympy, the twin against the
numpy restatement lane by lane, the two exact diffusions, the classical limit bit for bit, the statuses a kick can cause, the
reduction against exact arithmetic, and the front end's argument checks.  Lane-by-lane bounds are 1e-10 plus twice the twin's own
difference with and without FMA contraction (profiles/background_stochastic.json, written by ``python tests/stochastic_reference.py``)."""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import sympy as sp

import stochastic_reference as sr
import workloads
from conftest import MODELS, ROOT
from stochastic_reference import ENDED, NONFINITE, RUNNING, TARGET

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.fixture(scope="module")
def hyper():
    _spec, art, model, p = sr.hyperbolic_case()
    return art, model, p, sr.StochasticTwin(art)


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(hyper, counter, key, want):
    twin = hyper[3]
    assert tuple(twin.philox(counter, key)) == want
    assert tuple(int(w) for w in sr.philox4x32_10(*counter, *key)) == want


def test_uniforms_are_inside_the_unit_interval_and_the_normals_are_normal(hyper):
    """u at the extreme words is 2^-53 and 1 - 2^-53, exact; over 2^20 draws (steps 0 .. 2^20 - 1 of one realisation) the means, the
    variances and the correlation of xi^0, xi^1 are within 5 standard errors, twin and restatement, and the two agree to rounding."""
    twin = hyper[3]
    for fn in (twin.uniform, lambda hi, lo: float(sr.uniform(hi, lo))):
        assert fn(0, 0) == 2.0**-53 and fn(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0**-53 and fn(0, 0xFFF) == 2.0**-53 and fn(0, 0x1000) == 1.5 * 2.0**-52
        assert 0.0 < fn(0, 0) and fn(0xFFFFFFFF, 0xFFFFFFFF) < 1.0
    n, seed = 1 << 20, 0x9E3779B97F4A7C15
    got = twin.normals(seed, 0, n, 3, 77)
    x0, x1 = sr.normals(seed, np.arange(n, dtype=np.uint64), 3, 77)
    assert np.abs(got[:, 0] - x0).max() <= 1e-13 and np.abs(got[:, 1] - x1).max() <= 1e-13
    for a, b in ((got[:, 0], got[:, 1]), (x0, x1)):
        z = [a.mean() * math.sqrt(n), b.mean() * math.sqrt(n), (a.var(ddof=1) - 1.0) / math.sqrt(2.0 / (n - 1)), (b.var(ddof=1) - 1.0) / math.sqrt(2.0 / (n - 1)),
             np.corrcoef(a, b)[0, 1] * math.sqrt(n)]  # fmt: skip
        print("z-scores of mean, mean, variance, variance, correlation:", [f"{v:.2f}" for v in z])
        assert all(abs(v) <= 5.0 for v in z), z
    # a step index above 2^32 reaches the second counter word
    assert not np.array_equal(twin.normals(seed, 1 << 32, 4, 3, 77), twin.normals(seed, 0, 4, 3, 77))
    assert np.allclose(twin.normals(seed, (1 << 32) + 5, 1, 3, 77)[0], [float(v) for v in sr.normals(seed, np.uint64((1 << 32) + 5), 3, 77)], rtol=0, atol=1e-13)


_PI_TEXT = "3.14159265359"


def _noise_models():
    import background_truth as bt

    for name in MODELS:
        spec, art = workloads.artifact_for(name)
        (a0, b0), (a1, b1) = np.asarray(spec.extent, dtype=np.float64).reshape(2, 2)
        yield name, art, workloads.model_for(name), np.asarray(spec.args, dtype=np.float64), (a0, b0, a1, b1)
    for name in bt.NONDIAGONAL:
        art = bt.host_artifact(name)
        yield name, art, bt.zoo_model(name).model, np.array([1.0, 1.2, 0.8])[: art.n_parameters], bt.zoo_model(name).box


@pytest.mark.parametrize("name", [*MODELS, "skew", "shear"])
def test_noise_header_against_sympy(name):
    """The generated inflx_noise_point on the host against sympy in 40 digits at 25 points of the model's extent: e e^T = G^-1 and
    Gamma^a = G^bc Gamma^a_bc (written with the inverse metric) to 1e-13, relative to the largest entry of G^-1 and of Gamma.  No example
    model is compiled with exact_constants, so pi is the 12-digit constant of every generated header on both sides."""
    import mpmath

    case = {n: rest for n, *rest in _noise_models()}[name]
    art, model, p, box = case
    assert name not in MODELS or not workloads.artifact_for(name)[0].compiler_kwargs.get("exact_constants")
    twin = sr.StochasticTwin(art)
    _e, gam, Gi = sr.noise_expressions(model)
    # (pi is the compiler's constant, 12 digits unless exact_constants: the generated headers print INFLX_M_PI, and so does the truth)
    exprs = [sp.sympify(e).subs(sp.pi, sp.Float(_PI_TEXT, 45)) for e in (Gi[0, 0], Gi[0, 1], Gi[1, 1], *gam)]
    params, slots = sr._slots(model, art.symbol_dictionary, exprs)
    fn = sp.lambdify([*model.coordinates, *params], exprs, modules="mpmath")
    rng = np.random.default_rng(12)
    pts = np.stack([rng.uniform(box[0], box[1], 25), rng.uniform(box[2], box[3], 25)], axis=1)
    got = twin.noise_point(p, pts)
    worst = [0.0, 0.0]
    with mpmath.workdps(40):
        for (x0, x1), g in zip(pts, got):
            want = [complex(v) if mpmath.im(v) != 0 else float(v) for v in fn(mpmath.mpf(float(x0)), mpmath.mpf(float(x1)), *[mpmath.mpf(float(p[k])) for k in slots])]
            if not all(isinstance(v, float) and math.isfinite(v) for v in want) or not (want[0] > 0 and want[0] * want[2] - want[1] ** 2 > 0):
                continue  # (outside the model's domain, or the metric is not positive definite there)
            eet = [g[0] * g[0], g[0] * g[1], g[1] * g[1] + g[2] * g[2]]
            scale = max(abs(v) for v in want[:3])
            worst[0] = max(worst[0], max(abs(a - b) for a, b in zip(eet, want[:3])) / scale)
            gscale = max(abs(want[3]), abs(want[4]))
            if gscale > 0.0:
                worst[1] = max(worst[1], max(abs(g[3] - want[3]), abs(g[4] - want[4])) / gscale)
            else:
                assert g[3] == 0.0 and g[4] == 0.0
            assert g[0] > 0.0 and g[2] > 0.0
    print(f"{name}: worst relative error of e e^T {worst[0]:.2e}, of Gamma^a {worst[1]:.2e}")
    assert worst[0] <= 1e-13 and worst[1] <= 1e-13


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("case", ["hyperbolic", "skew"])
def test_twin_is_the_restatement_lane_by_lane(case, solver):
    """Fixed dt, the same Philox stream, 3 points x 130 realisations: N_end, the final state and the status of every lane, the twin
    against the restatement on lambdified sympy functions, within 1e-10 + 2 d."""
    name, art, model, p, pts = next(c for c in sr.parity_cases() if c[0] == case)
    steps = sr.PARITY_STEPS if name == "hyperbolic" else 200
    kw = dict(seed=sr.PARITY_SEED, noise_scale=sr.PARITY_SCALE, max_steps=steps, solver=solver, dt=sr.PARITY_DT)
    got = sr.StochasticTwin(art).run(p, pts, sr.PARITY_R, **kw)
    want = sr.restatement_of(model, art, p).run(pts, sr.PARITY_R, **kw)
    diff = sr.lane_difference(got, want)
    print(f"{name} {solver}: worst |twin - restatement| {diff:.3e} (bound {sr.bound():.3e}); statuses {np.bincount(got.status)}")
    assert np.array_equal(got.accepted, want.accepted) and diff <= sr.bound()
    if name == "hyperbolic":
        assert (got.status == ENDED).sum() > 300 and got.accepted.max() > 256
        # the realisations of a point differ, and differ from the classical trajectory
        n = got.N.reshape(3, -1)
        assert np.all(n.std(axis=1) > 1e-3)


@pytest.mark.parametrize("curved", [False, True])
def test_exact_diffusion(curved):
    """V = V0, chi = 0, N_stop = 8, dN = 1/16, R = 2^16.  Flat chart: Var phi^0 = Var phi^1 = (H / 2 pi)^2 8 and no covariance, within
    5 standard errors sigma^2 sqrt(2 / (R - 1)) -- the scheme is exact for constant coefficients.  Hyperbolic plane, L = 1, phi_0 = 1.5:
    E[cosh phi] = cosh(phi_0) exp(sigma^2 N) = 2.54833 within 5 standard errors; without the Ito term it would be cosh(phi_0)
    exp(sigma^2 N / 2), 4 per cent lower."""
    art, p, init, dt = sr.constant_case(curved)
    R = 1 << 16
    got = sr.StochasticTwin(art).run(p, init, R, seed=0, N_stop=sr.N_DIFFUSE, dt=dt, solver="rk4", max_steps=1000)
    assert got.accepted.max() <= 129
    z = sr.diffusion_checks(curved, got.N, got.state, got.status, R)
    if curved:
        assert z["martingale"] > 20.0  # (the mean is far above the Gaussian martingale's)
    assert np.all(got.state[:, 2:4] == 0.0) and np.all(got.state[:, 4] == math.sqrt(sr.V_CONST / 3.0))


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_noise_scale_zero_is_the_classical_run_bit_for_bit(hyper, solver):
    """Every realisation at noise_scale = 0: N_end, state and status of the plain stepper's host twin with stop_at_end at a fixed dt;
    of the adaptive run with dN_max = inf; and with N_stop the located state of the sampled twin (which is inflx_bg_step_target's)."""
    from background_reference import BackgroundTwin
    from background_sampled_reference import SampledTwin

    art, _model, p, twin = hyper
    plain, sampled = BackgroundTwin(art), SampledTwin(art)
    for init in sr.PARITY_POINTS[:2]:
        for kw in (dict(dt=2e-2), dict(dt=None, dN_max=math.inf, max_err=1e-8)):
            got = twin.run(p, init[None], 3, noise_scale=0.0, solver=solver, seed=9, **kw)
            rows, meta = plain.solve(p, init, 2048, solver, max_err=1e-8, dt=kw["dt"], stop_at_end=True)
            assert meta["status"] == ENDED and np.all(got.status == ENDED) and np.all(got.accepted == meta["last_row"])
            assert np.all(got.N == meta["N_end"]) and np.all(got.state == rows[meta["last_row"], :5])
        out, meta = sampled.solve(p, init, [4.0], 100000, solver, max_err=1e-8, stop_at_end=True)
        got = twin.run(p, init[None], 3, noise_scale=0.0, solver=solver, N_stop=4.0, dN_max=math.inf, max_err=1e-8)
        assert meta["status"] == TARGET and np.all(got.status == TARGET) and np.all(got.N == 4.0) and np.all(got.state == out[0, :5])
    # with the default dN_max the adaptive run takes other steps: the bound on dN acts
    assert twin.run(p, sr.PARITY_POINTS[:1], 1, noise_scale=0.0).accepted[0] > twin.run(p, sr.PARITY_POINTS[:1], 1, noise_scale=0.0, dN_max=math.inf).accepted[0]


def test_a_kick_can_end_inflation_or_leave_the_domain(hyper):
    """Constructed in the restatement, asserted on the twin.  Hyperbolic, two e-folds before the end with a large noise_scale: some
    realisations end by a kick (epsilon_H >= 1 after it: N_end is N there), the others in a step.  The wall model V = V0 + m phi^(3/2)
    from phi = 0.05: a kick to phi < 0 gives NONFINITE."""
    import background_reference as br
    from deltan_reference import host_artifact_of

    art, model, p, twin = hyper
    init = np.array([[2.6, 0.3, -0.75, 1e-4]])
    kw = dict(seed=4, noise_scale=2.0, dt=2e-2, max_steps=400)
    want = sr.restatement_of(model, art, p).run(init, 64, **kw)
    got = twin.run(p, init, 64, **kw)
    kick, step = want.by_kick & (want.status == ENDED), ~want.by_kick & (want.status == ENDED)
    assert kick.sum() >= 3 and step.sum() >= 3, (kick.sum(), step.sum(), np.bincount(want.status))
    assert np.array_equal(got.status, want.status) and np.array_equal(got.accepted, want.accepted)
    assert np.abs(got.N - want.N)[want.status == ENDED].max() <= sr.bound() and np.nanmax(np.abs(got.state - want.state)) <= sr.bound()
    # by a kick: N_end is a multiple of the steps' own N, not interpolated -- the lane's epsilon_H is >= 1 at its final state
    eom = sr.model_functions(model, art.symbol_dictionary)
    kin = eom(*got.state[:, :4].T, p)[3]
    eps = 0.5 * kin / got.state[:, 4] ** 2
    assert np.all(eps[got.status == ENDED] >= 1.0 - 1e-9)

    wall = br.wall_model()
    wart = host_artifact_of(wall, name="wall")
    wp = sr.named_pars(wart, V0=br.WALL_V0, m=br.WALL_M)
    winit = np.array([[0.05, 0.0, 0.0, 0.0]])
    kw = dict(seed=11, noise_scale=1.0, dt=5e-2, max_steps=8)
    want = sr.restatement_of(wall, wart, wp).run(winit, 64, **kw)
    got = sr.StochasticTwin(wart).run(wp, winit, 64, **kw)
    assert (want.status == NONFINITE).sum() >= 5 and (want.status == RUNNING).sum() >= 5, np.bincount(want.status)
    assert np.array_equal(got.status, want.status) and np.array_equal(got.accepted, want.accepted)
    # by a kick: the kicked field is kept and says where the lane went (the others left the domain inside a step, from phi > 0)
    assert (got.state[got.status == NONFINITE, 0] < 0.0).sum() >= 5 and np.all(got.state[got.status == RUNNING, 0] > 0.0)


def test_moments_against_exact_arithmetic(hyper):
    """The twin's reduction (the order of inflx_st_reduce) of the twin's own results against math.fsum and long double: the mean to
    1e-14 relative, m_k to 1e-12 var^(k/2); extremes and counts exact; once with every lane ended, once with some that are not."""
    art, _model, p, twin = hyper
    full = twin.run(p, sr.PARITY_POINTS[:1], 3000, seed=2, noise_scale=sr.PARITY_SCALE, dt=sr.PARITY_DT, max_steps=600)
    short = twin.run(p, sr.PARITY_POINTS[:1], 3000, seed=2, noise_scale=sr.PARITY_SCALE, dt=sr.PARITY_DT, max_steps=320)
    assert np.all(full.status == ENDED) and 100 < (short.status == ENDED).sum() < 2900
    for run in (full, short):
        out = twin.moments(run.N, run.status)
        ended = run.status == ENDED
        mean, m2, m3, m4 = sr.exact_moments(run.N[ended])
        assert abs(out[0] - mean) <= 1e-14 * abs(mean)
        for k, (got, want) in enumerate(((out[1], m2), (out[2], m3), (out[3], m4)), start=2):
            assert abs(got - want) <= 1e-12 * m2 ** (k / 2), (k, got, want)
        assert out[4] == run.N[ended].min() and out[5] == run.N[ended].max()
        assert np.array_equal(out[6:], np.bincount(run.status, minlength=6))
    none = twin.moments(np.array([1.0, 2.0]), np.array([0.0, 2.0]))
    assert np.isnan(none[:6]).all() and np.array_equal(none[6:], [1, 0, 1, 0, 0, 0])


def test_recorded_difference_is_anchored():
    rec = sr.recorded()
    assert set(rec["d"]) == {"hyperbolic/rk4", "hyperbolic/rkf", "skew/rk4", "skew/rkf", "worst"}
    assert 0.0 <= rec["d"]["worst"] <= 1e-11 and rec["d"]["worst"] == max(v for k, v in rec["d"].items() if k != "worst")


def test_public_names_and_unchanged_surface():
    import ctypes
    import re

    from inflatox_amd import _native, background
    from inflatox_amd.compiler import _DELTAN_SOURCES, _STOCHASTIC_SOURCES, KERNEL_GROUPS, CompilationArtifact

    assert {"stochastic_efolds", "stochastic_map", "StochasticEfolds"} <= set(background.__all__)
    assert background.StochasticEfolds._fields == ("N_mean", "N_var", "N_m3", "N_m4", "N_min", "N_max", "n_ended", "counts", "N_classical", "N", "state", "status")
    assert all(name in background.__doc__ for name in ("stochastic_efolds", "stochastic_map"))
    assert "conditional" in background.stochastic_efolds.__doc__.lower() and "biased" in background.stochastic_efolds.__doc__
    assert callable(CompilationArtifact.ensure_stochastic) and "stochastic" not in KERNEL_GROUPS
    assert _STOCHASTIC_SOURCES == ("inflx_stochastic_kernels.hip", "inflx_stochastic.h", "inflx_stochastic_abi.h", "inflx_philox.h", "inflx_background.h",
                                   "inflx_background_abi.h") and _STOCHASTIC_SOURCES[4:] == _DELTAN_SOURCES[3:]  # fmt: skip
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inflx_hip_stochastic.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(inflx_[a-z_0-9]+)\s*\(", text))) == sorted(_native.STOCHASTIC_SIGNATURES) == ["inflx_stochastic_efolds"]
    assert '#include "inflx_hip_stochastic.h"' in open(os.path.join(ROOT, "include", "inflx_hip.h")).read()
    assert len(_native.STOCHASTIC_SIGNATURES["inflx_stochastic_efolds"][1]) == 18
    assert not set(_native.STOCHASTIC_SIGNATURES) & (set(_native.SIGNATURES) | set(_native.DELTAN_SIGNATURES) | set(_native.EVOLUTION_SIGNATURES))
    _native.build_library()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "inflx_stochastic_efolds") and callable(_native.InflatoxDevLib.stochastic_efolds)
    abi = open(os.path.join(ROOT, "inflatox_amd", "csrc", "inflx_stochastic_abi.h")).read()
    assert re.search(r"#define INFLX_ST_OUT_PLANES 12\b", abi) and re.search(r"#define INFLX_ST_SAMPLE_PLANES 7\b", abi)
    assert (_native.ST_OUT_PLANES, _native.ST_SAMPLE_PLANES, _native.ST_MAX_REALISATIONS) == (12, 7, 1 << 20)
    # the noise header is a file of its own: the core header and the equations of motion do not change with it
    _spec, art = workloads.artifact_for("hyperbolic")
    assert "inflx_noise_point" in art.noise_header_text() and "inflx_noise_point" not in art.eom_header_text() and "inflx_noise_point" not in art._build[0]


def test_bad_arguments_raise_before_the_device(monkeypatch):
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    for ensure in ("ensure_stochastic", "ensure_background"):
        monkeypatch.setattr(CompilationArtifact, ensure, no_device)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = np.zeros((3, 2)) + 2.0, np.zeros((3, 2)) + 0.1
    shape, value = _native.InflatoxShapeError, ValueError
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    bad = (dict(seed=-1), dict(seed=2**64), dict(seed=1.5), dict(noise_scale=-1.0), dict(noise_scale=float("nan")), dict(noise_scale=float("inf")), dict(noise_scale="abc"),
           dict(dN_max=0.0), dict(dN_max=-1.0), dict(dN_max=float("nan")), dict(N_stop=0.0), dict(N_stop=-2.0), dict(N_stop=float("inf")), dict(max_steps=0),
           dict(max_steps=2.5), dict(max_err=0.0), dict(max_err=float("nan")), dict(solver="euler"), dict(dt=0.0), dict(dt=float("inf")), dict(streams=[0, 1, -1]),
           dict(streams=[0, 1, 2**32]), dict(streams=[0.5, 1.0, 2.0]))  # fmt: skip
    for kw in bad:
        with pytest.raises(value):
            background.stochastic_efolds(art, p, x, v, 8, **kw)
    for R in (0, -1, 2**20 + 1, 2.5, "abc"):
        with pytest.raises(value):
            background.stochastic_efolds(art, p, x, v, R)
    for args, kw in (((p[:2], x, v, 8), {}), ((np.zeros((2, p.size)), x, v, 8), {}), ((p, x, v[:2], 8), {}), ((p, np.zeros((3, 3)), np.zeros((3, 3)), 8), {}),
                     ((p, x[0], v[0], 8), {}), ((p, x, v, 8), dict(streams=[1, 2])), ((p, x, v, 8), dict(streams=[[1, 2, 3]]))):  # fmt: skip
        with pytest.raises(shape):
            background.stochastic_efolds(art, *args, **kw)
    with pytest.raises(shape):
        background.stochastic_efolds(three, np.zeros(3), x, v, 8)
    grid = ([[1.5, 4.0], [-1.0, 1.0]], 3, 3)
    for kw in bad[:20]:
        with pytest.raises(value):
            background.stochastic_map(art, p, *grid, 8, **kw)
    for R in (0, 2**20 + 1):
        with pytest.raises(value):
            background.stochastic_map(art, p, *grid, R)
    with pytest.raises(value):
        background.stochastic_map(art, p, grid[0], 0, 3, 8)
    for args, kw in (((p, [1.0, 2.0, 3.0], 3, 3, 8), {}), ((np.zeros((9, p.size)), *grid, 8), {}), ((p, *grid, 8), dict(derivatives_init=(0.0, 0.0, 0.0)))):
        with pytest.raises(shape):
            background.stochastic_map(art, *args, **kw)
    with pytest.raises(TypeError):
        background.stochastic_map(art, p, *grid, 8, return_samples=True)  # (it never returns samples)


def test_twin_program_under_address_and_ub_sanitizers(tmp_path, hyper):
    """tests/stochastic_twin.cpp as a stand-alone program (STOCHASTIC_TWIN_MAIN) under ASan + UBSan on the CPU: two points x 70
    realisations, both steppers, to the end of inflation and to a stop on N, then the reduction and one Philox call."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not available")
    _art, _model, p, twin = hyper
    exe = str(tmp_path / "stochastic_twin")
    cmd = [gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DSTOCHASTIC_TWIN_MAIN",
           *twin.compile_options(*twin.headers), os.path.join(ROOT, "tests", "stochastic_twin.cpp"), "-o", exe]  # fmt: skip
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe, *map(repr, p.tolist())], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.count("ended 70") == 4 and run.stdout.count("target 70") == 4 and "6627e8d5 e169c58d bc57ac4c 9b00dbd8" in run.stdout, run.stdout[-3000:]
