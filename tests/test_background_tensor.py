"""Tensor modes, P_T and the observables n_s, r on the host build (tests/tensor_twin.cpp compiles csrc/inflx_tensor.h for the CPU):
the two independent truths, the Wronskian, the order of the fixed step, the background of a fixed-dt run, the relation to the scalar
spectator on the power law, the stop statuses, the differencing front end on host spectra and the front end's argument checks.  The
bounds against the truths are 1e-10 plus twice the twin's own recorded step-control error (profiles/background_tensor.json, written
by ``python tests/tensor_reference.py``), relative to P_T's own size: a margin for other libm and contraction choices, not for
defects."""

import math
from typing import NamedTuple

import numpy as np
import pytest

import background_truth as bt
import modes_reference as mo
import tensor_reference as tn
import transfer_reference as tr
import workloads
from tensor_reference import COMPLETE, ENDED, NONFINITE, TARGET


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return spec.args, tn.TensorTwin(art)


@pytest.mark.parametrize("max_err", tn.MAX_ERRS)
@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_twin_against_truth_on_the_curved_zoo(name, solver, max_err):
    """Truth (b'): 65 lanes, a parameter row per lane, kappa = H0 e^3, evaluated at the last e-fold sample of
    ``background_truth.samples_for``; no lane is left out, every status is TARGET and the truth is finite.  The Wronskian
    e^(3N) (ht conj(pt) - pt conj(ht)) = 2 i kappa of the same run's accepted final state needs no truth: it is bilinear in the mode,
    so its relative error is what P_T's is -- the same bound."""
    init, pars, kappa, target = tn.zoo_lanes(name)
    truth = tn.zoo_truth(name)
    assert truth.shape == (3, tn.LANES) and np.isfinite(truth).all()
    got = tn.zoo_twin(name).lanes(pars, init, kappa, target, max_err=max_err, solver=solver, stop_at_end=False)
    assert np.all(got.status == TARGET) and np.isfinite(got.out).all() and np.all(got.out[5] == target)
    err, wron, bound = tn.relative_error(got.out[0], truth[0]), tn.wronskian_error(got.final, kappa), tn.bound(name, solver, max_err)
    print(f"{name} {solver} max_err {max_err:g}: worst relative |twin - truth (b')| {err:.3e}, Wronskian {wron:.3e}, bound {bound:.3e}")
    assert err <= bound and wron <= bound
    assert np.allclose(got.out[7], truth[1], rtol=0, atol=1e-6) and np.allclose(got.out[0], tn.p_t_of(got.out[1] + 1j * got.out[2], kappa), rtol=1e-14)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_all_257_lanes_of_every_zoo_model_meet_the_gpu_tests_condition(name, solver):
    """What tests/test_background_tensor_gpu.py relies on, established with the twin alone: of the 257 lanes of
    ``background_truth.batch`` with kappa = H0 e^3 and at most 20 000 steps, all of the first 65 and at least 250 in all are TARGET."""
    init, pars, kappa, target = tn.zoo_lanes(name, 257)
    got = tn.zoo_twin(name).lanes(pars, init, kappa, target, max_steps=20_000, solver=solver, stop_at_end=False)
    ok = got.status == TARGET
    print(f"{name} {solver}: {ok.sum()} of 257 lanes TARGET; the others {sorted(set(got.status[~ok].tolist()))}")
    assert ok[: tn.LANES].all() and ok.sum() >= 250


# The coarser of the two step counts per stepper, chosen as tests/test_background_modes.py chooses its own: the first of 20, 40, 80 at
# which every one of the 17 lanes of ``transfer_reference.hyper_states`` (seed 0) has a ratio >= 14.5 to T = 1 with kappa = 2 H0.
# n = 20 held for both: rk4 ratios 16.4 .. 17.1, rkf 16.9 .. 18.5.
ORDER_N = {"rk4": 20, "rkf": 20}


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_fixed_step_is_fourth_order_in_the_tensor_mode(hyper, solver):
    """A fixed dt = T / n to T = 1 on 17 inflating lanes of the hyperbolic model with kappa = 2 H0, the end state's two components
    of ht and two of pt / kappa against the two equations integrated by DOP853 at rtol 1e-13, and halving dt cuts every lane's error
    by >= 14.5; the error at the finer step is above 1e-10."""
    p, twin = hyper
    x, v = tr.hyper_states(17)
    init = np.concatenate([x, v], axis=1)
    kappa = 2.0 * tn.friedmann_h(twin, p, init)
    g = tn.workload_rhs("hyperbolic")
    want = np.array([tn.truth_final(g, init[k], p, kappa[k], bt.T_ORDER) for k in range(17)])

    def errors(n):
        sol = twin.lanes(p, init, kappa, np.nan, max_steps=n, solver=solver, dt=bt.T_ORDER / n, stop_at_end=False)
        assert np.all(sol.status == COMPLETE) and np.all(sol.accepted == n) and np.isnan(sol.out).all()
        d = np.abs(sol.final[:, 6:10] - want)
        d[:, 2:] /= kappa[:, None]
        return d.max(axis=1)

    n = ORDER_N[solver]
    for smaller in (m for m in (20, 40) if m < n):  # (n is the FIRST at which it holds)
        assert (errors(smaller) / errors(2 * smaller)).min() < 14.5
    coarse, fine = errors(n), errors(2 * n)
    ratios = coarse / fine
    print(f"{solver}: n = {n}; error at n = {2 * n} {fine.min():.2e} .. {fine.max():.2e}, ratios {ratios.min():.2f} .. {ratios.max():.2f}")
    assert fine.min() > 1e-10 and ratios.min() >= 14.5, (ratios.min(), int(np.argmin(ratios)))


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_fixed_dt_background_is_solve_eom_sampled_bit_for_bit(hyper, solver):
    """With a fixed dt the steps do not depend on the mode and the first six components are computed with the expressions of the
    plain stepper: N, t and eps_H at the target are the sampled stepper's at that sample, bit for bit, and the carried background
    does not depend on kappa."""
    from background_sampled_reference import SampledTwin

    p, twin = hyper
    x, v = tr.hyper_states(9)
    init = np.concatenate([x, v], axis=1)
    kappa = 20.0 * tn.friedmann_h(twin, p, init)
    got = twin.lanes(p, init, kappa, 0.1, max_steps=2000, solver=solver, dt=2e-3)
    assert np.all(got.status == TARGET)
    plain = SampledTwin(twin.artifact)
    for k in range(9):
        out, meta = plain.solve(p, init[k], [0.1], 2000, solver, dt=2e-3, stop_at_end=True)
        assert meta["status"] == TARGET and meta["accepted"] == got.accepted[k]
        assert got.out[5, k] == out[0, 5] and got.out[6, k] == out[0, 6] and got.out[7, k] == out[0, 7]
    other = twin.lanes(p, init, 3.0 * kappa, 0.1, max_steps=2000, solver=solver, dt=2e-3)
    assert np.array_equal(other.final[:, :6], got.final[:, :6]) and not np.array_equal(other.out[0], got.out[0])


def test_power_law_spectrum_is_the_exact_one():
    """Truth (c'): power-law inflation, p = 8.  The formula is first confirmed by DOP853 from the project's own initial conditions
    (the vacuum put in N_sub = 3 e-folds before the exit leaves an error of order e^(-2 N_sub), recorded in the profile); the twin is
    then within twice that of the formula.  The flat second field of the model is a massless spectator that obeys the tensor
    equation, so P_T = 16 eps P_S with ``ModesTwin``'s P_S needs no truth: both twins are within their bounds of their formulas,
    which are in that ratio, hence within the sum of each other.  The slope between the two wavenumbers is -2 eps / (1 - eps)."""
    import background_reference as br

    art, p, init, h_k = mo.power_law_case()
    want = tn.power_law_formula(h_k)
    assert np.allclose(want, 16.0 / br.P_POW * mo.power_law_formula(h_k), rtol=1e-15)
    start, bound = tn.power_law_start_error(), tn.power_law_bound()
    assert 0.0 < start <= 4.0 * math.exp(-2.0 * tn.N_SUB) and start <= 1.01 * bound / 2.0 and bound / 2.0 <= 1.01 * start  # (the formula, and the record)
    kw = dict(N_eval=mo.POWER_N_EVAL, N_sub=tn.N_SUB, stop_at_end=False)
    ts = tn.TensorTwin(art).tensor_spectra(p, mo.POWER_N_EXIT, init[None, :2], init[None, 2:], **kw)
    ps = mo.ModesTwin(art).power_spectra(p, mo.POWER_N_EXIT, init[None, :2], init[None, 2:], **kw)
    assert np.all(ts.status == TARGET) and np.all(ts.N == mo.POWER_N_EVAL) and np.allclose(ts.eps_H, 1 / br.P_POW, rtol=1e-9) and np.array_equal(ts.k, ps.k)
    eps = 1.0 / br.P_POW
    err, rel = np.abs(ts.P_T[0] - want) / want, np.abs(ts.P_T[0] / (16.0 * eps * ps.P_S[0]) - 1.0)
    slope = math.log(ts.P_T[0, 1] / ts.P_T[0, 0]) / math.log(ts.k[0, 1] / ts.k[0, 0])
    print(f"power law: |P_T - formula| / formula {err.max():.3e} (bound {bound:.3e}), |P_T / (16 eps P_S) - 1| {rel.max():.3e} "
          f"(bound {bound + mo.power_law_bound():.3e}); slope {slope:.6f}, exact {-2 * eps / (1 - eps):.6f}")  # fmt: skip
    assert err.max() <= bound and rel.max() <= bound + mo.power_law_bound()
    assert abs(slope + 2 * eps / (1 - eps)) <= 2 * bound / math.log(ts.k[0, 1] / ts.k[0, 0])


def test_every_status_and_what_each_emits(hyper):
    """TARGET: the located state.  ENDED: the mode linear across the last step, eps_H = 1, N = N_end; with a target past the end of
    inflation the lane still ENDS.  COMPLETE: nothing.  A lane AT REST runs to its TARGET with a finite P_T (the scalar lanes refuse
    it).  A kappa that is zero, negative, NaN or infinite: NONFINITE at once, nothing.  A target <= 0 is the initial state: the
    vacuum's own spectrum."""
    p, twin = hyper
    x, v = tr.hyper_states(9)
    init = np.concatenate([x, v], axis=1)
    init[3, 2:] = 0.0
    H0 = tn.friedmann_h(twin, p, init)
    kappa = 20.0 * H0
    kappa[4], kappa[6], kappa[7], kappa[8] = -1.0, 0.0, np.nan, np.inf
    target = np.array([0.2, 50.0, 0.2, 0.2, 0.2, 0.0, 0.2, 0.2, 0.2])
    got = twin.lanes(p, init, kappa, target, max_steps=100_000)
    assert got.status.tolist() == [TARGET, ENDED, TARGET, TARGET, NONFINITE, TARGET, NONFINITE, NONFINITE, NONFINITE]
    assert np.isfinite(got.out[:, [0, 1, 2, 3, 5]]).all() and np.isnan(got.out[:, [4, 6, 7, 8]]).all() and np.all(got.accepted[[4, 6, 7, 8]] == 0)
    assert got.out[0, 3] > 0.0 and got.out[5, 3] == 0.2 and got.out[7, 3] > 0.0  # (at rest at the start: it has rolled by the target)
    assert got.out[7, 1] == 1.0 and got.out[5, 1] == got.N_end[1] and 0.2 < got.N_end[1] < 50.0 and np.isnan(got.N_end[[0, 2, 3, 5]]).all()
    free = twin.lanes(p, init[:3], kappa[:3], np.nan)
    assert np.all(free.status == ENDED) and np.array_equal(free.out[:, 1], got.out[:, 1])
    short = twin.lanes(p, init[:4], kappa[:4], 0.2, max_steps=7)
    assert np.all(short.status == COMPLETE) and np.isnan(short.out).all()
    rest = twin.lanes(p, init[3:4], kappa[3:4], 0.0)  # at rest and evaluated there: eps_H = 0, and P_T is the vacuum's all the same
    vac = 2.0 * kappa[[5, 3]] ** 2 / math.pi**2
    assert rest.status[0] == TARGET and rest.out[7, 0] == 0.0 and rest.out[0, 0] == pytest.approx(vac[1], rel=1e-15)
    assert got.out[0, 5] == pytest.approx(vac[0], rel=1e-15) and got.out[1, 5] == 1.0 and got.out[2, 5] == 0.0 and got.out[3, 5] == -H0[5] and got.out[4, 5] == -kappa[5]
    assert got.out[5, 5] == 0.0 and got.out[6, 5] == 0.0 and got.accepted[5] == 0


class Spectra(NamedTuple):
    """the members ``background.observables_from_spectra`` reads, from any source"""

    P_R: np.ndarray
    P_S: np.ndarray
    C_RS: np.ndarray
    P_T: np.ndarray
    k: np.ndarray
    N_end: np.ndarray
    status: np.ndarray


def test_stencil_is_exact_on_a_quadratic_and_its_weights_are_the_lagrange_ones():
    """``log_slopes`` on ln P = a + b x + c x^2 at unequal spacings returns b + 2 c x_0 and 2 c; the weights sum to 0 and reproduce x"""
    from inflatox_amd.background import log_slopes, stencil_weights

    x = np.array([[0.3, 0.9, 1.2], [-2.0, -1.1, 0.5]])
    a, b, c = 0.7, -0.28, 0.013
    d1, d2 = log_slopes(np.exp(x), np.exp(a + b * x + c * x * x))
    assert np.allclose(d1, b + 2 * c * x[:, 1], rtol=0, atol=1e-13) and np.allclose(d2, 2 * c, rtol=0, atol=1e-12)
    w1, w2 = stencil_weights(np.exp(x))
    assert np.allclose(w1.sum(-1), 0, atol=1e-13) and np.allclose((w1 * x).sum(-1), 1) and np.allclose(w2.sum(-1), 0, atol=1e-12) and np.allclose((w2 * x).sum(-1), 0, atol=1e-12)


def test_observables_on_the_power_law_are_the_exact_ones():
    """``observables``' differencing half, fed the two twins' spectra at N_exit = 3.5 -/+ dN, dN = 0.5: n_s - 1 = n_t = -2/7, r = 2,
    alpha_s = 0.  ln P is exactly linear in ln k, so the quadratic has no error of its own, and each twin's spectrum is within its
    power-law bound of its formula at every wavenumber (the model is self-similar: the start at N_sub leaves the same relative error
    at each): the bound on each result is what ``stencil_bounds`` derives from those two recorded values and the stencil's weights."""
    import background_reference as br
    from inflatox_amd import background

    art, p, init, _h = mo.power_law_case()
    pivots, dN = np.array([3.5]), 0.5
    pts, inverse = np.unique(np.concatenate([pivots - dN, pivots, pivots + dN]), return_inverse=True)
    kw = dict(N_eval=mo.POWER_N_EVAL, N_sub=tn.N_SUB, stop_at_end=False)
    ps = mo.ModesTwin(art).power_spectra(p, pts, init[None, :2], init[None, 2:], **kw)
    ts = tn.TensorTwin(art).tensor_spectra(p, pts, init[None, :2], init[None, 2:], **kw)
    obs = background.observables_from_spectra(ps, ts, inverse.reshape(3, 1), TARGET)
    assert isinstance(obs, background.Observables) and obs.n_s.shape == (1, 1) and obs.status[0, 0] == TARGET and np.isnan(obs.N_end).all()
    eps = 1.0 / br.P_POW
    b_ns, b_alpha, b_nt, b_r = tn.stencil_bounds(ps.k[:, inverse.reshape(3, 1).T], mo.power_law_bound(), tn.power_law_bound())
    tilt = -2.0 * eps / (1.0 - eps)
    print(f"power law: n_s - 1 {obs.n_s[0, 0] - 1:.6f} and n_t {obs.n_t[0, 0]:.6f} (exact {tilt:.6f}; bounds {b_ns:.2e}, {b_nt:.2e}), r {obs.r[0, 0]:.6f} (bound {b_r:.2e} "
          f"of 2), alpha_s {obs.alpha_s[0, 0]:.2e} (bound {b_alpha:.2e})")  # fmt: skip
    assert abs(obs.n_s[0, 0] - 1.0 - tilt) <= b_ns and abs(obs.n_t[0, 0] - tilt) <= b_nt and abs(obs.alpha_s[0, 0]) <= b_alpha
    assert abs(obs.r[0, 0] / (16.0 * eps) - 1.0) <= b_r and obs.A_s[0, 0] == ps.P_R[0, 1] and obs.A_t[0, 0] == ts.P_T[0, 1] and obs.k[0, 0] == ps.k[0, 1]
    assert abs(obs.beta_iso[0, 0] - 0.5) <= mo.power_law_bound() and abs(obs.cos_delta[0, 0]) <= 1e-12
    # a lane that did not stop where asked makes its pivot NaN and hands on its status
    bad = ts._replace(status=np.array([[TARGET, TARGET, COMPLETE]], dtype=np.int8))
    lost = background.observables_from_spectra(ps, bad, inverse.reshape(3, 1), TARGET)
    assert lost.status[0, 0] == COMPLETE and all(np.isnan(m).all() for m in lost[:8]) and lost.k[0, 0] == obs.k[0, 0]


def test_observables_pipeline_on_truth_spectra_of_the_hyperbolic_model():
    """The same pipeline on the hyperbolic example model, once on the twins' spectra and once on truth spectra -- (b) for the scalars,
    (b') for the tensors, both from the twins' own first stage -- at the pivot N_exit = 3.25 with dN = 0.25, N_sub = 3, N = 6,
    max_err = 1e-10: the results agree within what the recorded errors of the two twins on this run (``hyper_bound``) allow through
    the stencil's weights."""
    from inflatox_amd import background

    spec, art = workloads.artifact_for("hyperbolic")
    x, v = mo.hyper_states(2)
    pts = np.array([3.0, 3.25, 3.5])
    kw = dict(N_eval=mo.HYPER_N_EVAL, N_sub=tn.N_SUB, max_err=mo.HYPER_MAX_ERR)
    mtwin, ttwin = mo.ModesTwin(art), tn.TensorTwin(art)
    ps, ts = mtwin.power_spectra(spec.args, pts, x, v, **kw), ttwin.tensor_spectra(spec.args, pts, x, v, **kw)
    assert np.all(ps.status == TARGET) and np.all(ts.status == TARGET) and np.array_equal(ps.k, ts.k)
    start, h_exit, _st, starts = ttwin.stage1(spec.args, pts, x, v, tn.N_SUB, max_err=mo.HYPER_MAX_ERR)
    gs, gt = mo.workload_rhs("hyperbolic"), tn.workload_rhs("hyperbolic")
    lanes = [(b, j, h_exit[b, j] * math.exp(tn.N_SUB), mo.HYPER_N_EVAL - starts[j]) for b in range(2) for j in range(3)]
    scalar = np.array([mo.truth_lane(gs, start[b, j], spec.args, kappa, target)[:3] for b, j, kappa, target in lanes]).reshape(2, 3, 3)
    tensor = np.array([tn.truth_lane(gt, start[b, j], spec.args, kappa, target)[0] for b, j, kappa, target in lanes]).reshape(2, 3)
    truth = Spectra(scalar[..., 0], scalar[..., 1], scalar[..., 2], tensor, ps.k, ps.N_end, ps.status)
    cols = np.array([[0], [1], [2]])
    got = background.observables_from_spectra(ps, ts, cols, TARGET)
    want = background.observables_from_spectra(truth, truth, cols, TARGET)
    b_ns, b_alpha, b_nt, b_r = tn.stencil_bounds(ps.k[:, None, :], mo.hyper_bound("rkf"), tn.hyper_bound("rkf"))
    print(f"hyperbolic: n_s {want.n_s[:, 0]}, r {want.r[:, 0]}, n_t {want.n_t[:, 0]}, alpha_s {want.alpha_s[:, 0]}; |twins - truths| n_s {np.abs(got.n_s - want.n_s).max():.2e} "
          f"(bound {b_ns:.2e}), alpha_s {np.abs(got.alpha_s - want.alpha_s).max():.2e} ({b_alpha:.2e}), n_t {np.abs(got.n_t - want.n_t).max():.2e} ({b_nt:.2e}), "
          f"r {np.abs(got.r / want.r - 1).max():.2e} ({b_r:.2e})")  # fmt: skip
    assert np.isfinite(np.array(want[:8])).all() and np.all(want.r > 0) and np.all(want.n_t < 0)
    assert np.abs(got.n_s - want.n_s).max() <= b_ns and np.abs(got.alpha_s - want.alpha_s).max() <= b_alpha and np.abs(got.n_t - want.n_t).max() <= b_nt
    assert np.abs(got.r / want.r - 1).max() <= b_r


def test_recorded_errors_are_anchored():
    """The bounds come from profiles/background_tensor.json, which tests/tensor_reference.py writes from the host build.  Two anchors
    keep a re-recording from widening them unseen: the file carries the hash of the stepper's code it was measured with, which must
    be the present code's, and every recorded value is at most 100 max_err^(4/5), the cap of tests/test_background_transfer.py."""
    rec = tn.recorded()
    assert rec["stepper_code"] == tn.stepper_code_hash()
    values = {f"{group}/{k}": v for group in ("zoo", "hyperbolic", "wronskian") for k, v in rec[group].items()}
    assert len(values) == 32 + 2 + 32
    for key, value in values.items():
        max_err = float(key.rsplit("/", 1)[1])
        assert 0.0 < value <= 100.0 * max_err**0.8, (key, value)
    assert rec["power_law"]["N_sub"] == tn.N_SUB


def test_public_names_and_unchanged_surface():
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import _MODES_SOURCES, _TENSOR_SOURCES, KERNEL_GROUPS, CompilationArtifact

    assert {"tensor_spectra", "TensorSpectra", "observables", "Observables", "observables_map"} <= set(background.__all__)
    assert background.TensorSpectra._fields == tn.TwinSpectra._fields[:7]
    assert background.Observables._fields == ("A_s", "A_t", "r", "n_s", "alpha_s", "n_t", "beta_iso", "cos_delta", "k", "N_end", "status")
    assert len(_native.SIGNATURES) == 57 and len(_native.SIGNATURES["inflx_mode_spectra"][1]) == 16
    assert _native.MODES_TENSOR == 8 and _native.MODES_TENSOR & _native.EOM_STOP_AT_END == 0
    assert all(name in background.__doc__ for name in ("tensor_spectra", "observables", "observables_map"))
    assert callable(CompilationArtifact.ensure_tensor) and "tensor" not in KERNEL_GROUPS
    assert _TENSOR_SOURCES == ("inflx_tensor_kernels.hip", "inflx_tensor.h", "inflx_tensor_abi.h", "inflx_background.h", "inflx_background_abi.h")
    assert _MODES_SOURCES[3:] == _TENSOR_SOURCES[3:]


def test_bad_arguments_raise_before_the_device(monkeypatch):
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    for ensure in ("ensure_tensor", "ensure_modes", "ensure_background"):
        monkeypatch.setattr(CompilationArtifact, ensure, no_device)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = np.zeros((3, 2)) + 2.0, np.zeros((3, 2)) + 0.1
    good = [5.5, 6.0]
    shape, value = _native.InflatoxShapeError, ValueError
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    common = (dict(max_steps=0), dict(max_steps=-1), dict(max_steps=2.5), dict(max_err=0.0), dict(max_err=-1e-6), dict(max_err=float("nan")), dict(solver="euler"),
              dict(dt=0.0), dict(dt=float("inf")), dict(N_sub=0.0), dict(N_sub=-1.0), dict(N_sub=float("nan")), dict(N_sub="abc"), dict(N_sub=5.6), dict(N_eval=6.0),
              dict(N_eval=5.5), dict(N_eval=float("nan")), dict(N_eval=float("inf")), dict(N_eval="abc"), dict(stop_at_end=False))  # fmt: skip
    for fn in (background.tensor_spectra, background.observables):
        for bad in ([4.9, 6.0], [5.5, float("nan")], [5.5, float("inf")], [], "abc"):
            with pytest.raises(value):
                fn(art, p, bad, x, v)
        with pytest.raises(shape):
            fn(art, p, [[5.5, 6.0]], x, v)
        for args in ((p[:2], good, x, v), (np.zeros((2, p.size)), good, x, v), (p, good, x, v[:2]), (p, good, np.zeros((3, 3)), np.zeros((3, 3)))):
            with pytest.raises(shape):
                fn(art, *args)
        for kw in common:
            with pytest.raises(value):
                fn(art, p, good, x, v, **kw)
        with pytest.raises(shape):
            fn(three, np.zeros(3), good, x, v)
    # observables' own: dN, the lower point against N_sub, N_eval against the upper point
    for kw in (dict(dN=0.0), dict(dN=-0.5), dict(dN=float("nan")), dict(dN=float("inf")), dict(dN="abc"), dict(dN=0.6), dict(N_eval=6.4), dict(N_eval=6.5)):
        with pytest.raises(value):
            background.observables(art, p, good, x, v, **kw)
    om = background.observables_map
    for kw in (dict(N_star=-1.0), dict(N_star=float("nan")), dict(N_sub=0.0), dict(N_sub=float("inf")), dict(dN=0.0), dict(dN=float("nan")), dict(dN="abc"), dict(max_err=0.0),
               dict(solver="euler")):  # fmt: skip
        with pytest.raises(value):
            om(art, p, [[1.5, 4.0], [-1.0, 1.0]], 3, 3, **kw)
    with pytest.raises(shape):
        om(art, p[:2], [[1.5, 4.0], [-1.0, 1.0]], 3, 3)
