"""Tensor modes, P_T and the observables on the GPU (inflatox_amd.background.tensor_spectra, observables, observables_map,
InflatoxDevLib.mode_spectra with MODES_TENSOR): the kernels against truth (b') and the host twin on the curved zoo, a run of several
launches with its lane numbering and lane independence, more than one pass, every stop status side by side, the two heaviest example
models, truth (c') and the scalar spectator, the refusal of a tensor object of another layout, the scalar path untouched by a tensor
call, and the front end against its halves.  Truths, twin and bounds are those tests/test_background_tensor.py establishes on the host
build (tests/tensor_reference.py, profiles/background_tensor.json); every difference is printed."""

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import background_truth as bt
import modes_reference as mo
import tensor_reference as tn
import workloads
from tensor_reference import COMPLETE, ENDED, NONFINITE, TARGET

pytestmark = pytest.mark.gpu

MEMBERS = ("P_T", "k", "N", "eps_H", "modes", "N_end", "status")


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return spec.args, art, tn.TensorTwin(art)


def _lanes(bg, art, pars, init, kappa, target, max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None, stop_at_end=True):
    """``InflatoxDevLib.mode_spectra`` with ``MODES_TENSOR`` on the artefact's handle, as a ``TwinLanes`` without ``accepted`` and
    ``final``"""
    from inflatox_amd import _native

    art.ensure_tensor()
    n = len(init)
    out, n_end, status = bg._dylib(art, background=False).mode_spectra(
        pars, init, np.broadcast_to(np.asarray(kappa, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(target, dtype=np.float64), (n,)), max_steps,
        bg._METHODS[solver], max_err, dt or 0.0, _native.MODES_TENSOR | (_native.EOM_STOP_AT_END if stop_at_end else 0))  # fmt: skip
    return tn.TwinLanes(out, n_end, status, None, None)


def _same(a, b, rows=slice(None), cols=slice(None)):
    """the members of two TensorSpectra, bit for bit and NaN where NaN; ``rows``, ``cols`` select from ``a``"""
    return all(np.array_equal(getattr(a, m)[rows][:, cols], getattr(b, m), equal_nan=True) for m in MEMBERS)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_kernel_against_truth_and_twin(bg, name, solver):
    """All 257 lanes of ``background_truth.batch`` (four wavefronts and one lane: the last workgroup and the last wavefront are
    partial), a parameter row per lane, kappa = H0 e^3, the default max_err = 1e-8, at most 20 000 steps.  ``status`` is the host
    twin's on every lane; on the lanes the twin reports TARGET -- all of the first 65 and at least 250 in all, which
    tests/test_background_tensor.py establishes with the twin alone -- P_T is within the bound of the twin.  Truth (b') is established
    for the first 65 lanes: there P_T is within the bound of it."""
    art = bt.device_artifact(name)
    init, pars, kappa, target = tn.zoo_lanes(name, 257)
    assert init.shape == (257, 4) and pars.shape == (257, art.n_parameters)
    truth = tn.zoo_truth(name)
    got = _lanes(bg, art, pars, init, kappa, target, max_steps=20_000, solver=solver, stop_at_end=False)
    twin = tn.zoo_twin(name).lanes(pars, init, kappa, target, max_steps=20_000, solver=solver, stop_at_end=False)
    ok = twin.status == TARGET
    bound = tn.bound(name, solver, 1e-8)
    err = tn.relative_error(got.out[0, : tn.LANES], truth[0])
    diff = tn.relative_error(got.out[0, ok], twin.out[0, ok])
    print(f"{name} {solver}: worst relative |GPU - truth (b')| {err:.3e} (bound {bound:.3e}), worst relative |GPU - host twin| on {ok.sum()} TARGET lanes {diff:.3e}")
    assert got.out.shape == (8, 257) and np.array_equal(got.status, twin.status)
    assert ok[: tn.LANES].all() and ok.sum() >= 250
    assert np.isfinite(got.out[:, ok]).all() and np.isnan(got.out[:, ~ok]).all() and err <= bound and diff <= bound
    assert np.all(got.out[5, ok] == target) and np.isnan(got.N_end).all()


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_several_launches_lane_numbering_and_lane_independence(bg, hyper, solver):
    """B = 5 trajectories high on the hyperbolic potential, K = 52 wavenumbers with N_exit = 3 .. 3.51, N_sub = 3, max_err = 1e-10: 260
    lanes, each of more than 256 accepted steps by the twin's count, so two or more launches and a carried state.  Lane b K + j is
    trajectory b with wavenumber j: the twin, fed the device's own first stage, has the same statuses; evaluated at N = 6, P_T is
    within the bound of the twin's own error there (profiles/background_tensor.json), lane by lane, and ``k`` is ``power_spectra``'s
    bit for bit.  To the end of inflation N_end agrees with the twin's to 1e-3, the accuracy ``efolds_map`` documents for it, and a
    permuted batch and the sub-batches (B, K) = (1, 1) and (5, 13) give the same lanes bit for bit."""
    p, art, twin = hyper
    x, v = mo.hyper_states()
    kw = dict(N_sub=tn.N_SUB, max_err=mo.HYPER_MAX_ERR, solver=solver)
    pts = np.unique(np.concatenate([mo.HYPER_N_EXIT - tn.N_SUB, mo.HYPER_N_EXIT]))
    stage1 = bg.solve_eom_sampled(art, p, pts, x, v, 1_000_000, mo.HYPER_MAX_ERR, solver)
    at = bg.tensor_spectra(art, p, mo.HYPER_N_EXIT, x, v, N_eval=mo.HYPER_N_EVAL, **kw)
    want = twin.tensor_spectra(p, mo.HYPER_N_EXIT, x, v, N_eval=mo.HYPER_N_EVAL, stage1=stage1, **kw)
    assert isinstance(at, bg.TensorSpectra) and at.P_T.shape == at.modes.shape == (mo.HYPER_B, mo.HYPER_K) and np.iscomplexobj(at.modes)
    assert np.all(at.status == TARGET) and np.array_equal(at.status, want.status) and want.accepted.min() > 256
    diff, bound = tn.relative_error(at.P_T, want.P_T), tn.hyper_bound(solver)
    print(f"{solver}: {want.accepted.min()} .. {want.accepted.max()} accepted steps to N = {mo.HYPER_N_EVAL:g}, worst relative |GPU - host twin| {diff:.3e} (bound {bound:.3e})")
    assert np.isfinite(at.P_T).all() and diff <= bound and np.array_equal(at.k, want.k) and np.all(at.N == mo.HYPER_N_EVAL) and np.isnan(at.N_end).all()
    assert np.all(np.diff(at.k, axis=1) > 0) and np.allclose(at.modes, want.modes, rtol=0, atol=bound * np.abs(want.modes).max())
    scalar = bg.power_spectra(art, p, mo.HYPER_N_EXIT, x, v, N_eval=mo.HYPER_N_EVAL, **kw)
    assert np.array_equal(at.k, scalar.k) and np.all(at.P_T < 16.0 * scalar.P_R)  # (r < 16 eps < 16)
    got = bg.tensor_spectra(art, p, mo.HYPER_N_EXIT, x, v, **kw)
    end = twin.tensor_spectra(p, mo.HYPER_N_EXIT, x, v, stage1=stage1, **kw)
    print(f"{solver}: {end.accepted.min()} .. {end.accepted.max()} accepted steps to the end, worst |N_end - host twin's| {np.abs(got.N_end - end.N_end).max():.3e}, "
          f"worst relative |GPU - host twin| there {tn.relative_error(got.P_T, end.P_T):.3e}")  # fmt: skip
    assert np.all(got.status == ENDED) and np.array_equal(got.status, end.status) and end.accepted.min() > 256
    assert np.isfinite(got.P_T).all() and np.all(got.eps_H == 1.0) and np.array_equal(got.N, got.N_end) and np.abs(got.N_end - end.N_end).max() <= 1e-3
    assert np.array_equal(got.k, at.k)
    perm = np.random.default_rng(9).permutation(mo.HYPER_B)
    assert _same(got, bg.tensor_spectra(art, p, mo.HYPER_N_EXIT, x[perm], v[perm], **kw), perm)
    assert _same(got, bg.tensor_spectra(art, p, mo.HYPER_N_EXIT[17:18], x[3:4], v[3:4], **kw), slice(3, 4), slice(17, 18))
    assert _same(got, bg.tensor_spectra(art, p, mo.HYPER_N_EXIT[39:], x, v, **kw), slice(None), slice(39, 52))


def test_more_than_one_pass_is_the_same_lanes_in_two_calls(bg, hyper):
    """n = 2^20 + 257 lanes -- a pass holds at most 2^20 --, two fixed steps of dt = 0.01: every lane with a target of 0.02 e-folds
    reaches it within them (TARGET, values emitted), the others run out of steps (COMPLETE, NaN).  The result equals the
    first 2^20 lanes and the last 257 run as two calls, bit for bit."""
    p, art, twin = hyper
    n, first = (1 << 20) + 257, 1 << 20
    rng = np.random.default_rng(5)
    x = np.stack([rng.uniform(4.5, 5.0, n), rng.uniform(-1.0, 1.0, n)], axis=1)
    init = np.concatenate([x, np.stack([np.full(n, -0.8), rng.uniform(-1e-3, 1e-3, n)], axis=1)], axis=1)
    kappa = rng.uniform(2.0, 6.0, n)
    target = np.where(np.arange(n) % 3 == 2, np.nan, 0.02)
    kw = dict(max_steps=2, dt=0.01)
    whole = _lanes(bg, art, p, init, kappa, target, **kw)
    head = _lanes(bg, art, p, init[:first], kappa[:first], target[:first], **kw)
    tail = _lanes(bg, art, p, init[first:], kappa[first:], target[first:], **kw)
    assert whole.out.shape == (8, n) and np.array_equal(whole.status, np.where(np.isnan(target), COMPLETE, TARGET))
    assert np.isfinite(whole.out[:, whole.status == TARGET]).all() and np.isnan(whole.out[:, whole.status == COMPLETE]).all()
    for a, b, c in zip(whole[:3], head[:3], tail[:3]):
        assert np.array_equal(a[..., :first], b, equal_nan=True) and np.array_equal(a[..., first:], c, equal_nan=True)
    want = twin.lanes(p, init[first - 3 :], kappa[first - 3 :], target[first - 3 :], **kw)  # the lanes on either side of the seam
    assert np.array_equal(whole.status[first - 3 :], want.status)
    emits = want.status == TARGET
    assert tn.relative_error(whole.out[0, first - 3 :][emits], want.out[0, emits]) <= 1e-11


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_every_status_side_by_side(bg, hyper, solver):
    """257 lanes of four kinds, in turn, five steps of dt = 0.05, kappa = 2 H0 and the target N = 0.2: a lane high on the potential
    reaches it (TARGET); a slower one runs out of steps (COMPLETE, all NaN); one that starts 0.05 e-folds before epsilon_H = 1 ends
    there (ENDED: the values at the end, eps_H = 1); one AT REST reaches the target as well (TARGET, a finite P_T: the scalar lanes
    refuse it).  The last lane has kappa = 0: NONFINITE, all NaN.  Five fixed steps leave the host twin and the device a few
    roundings apart -- some thousand operations of 1e-16 each, amplified by at most the few e-folds of growth: 1e-11 of P_T, the
    bound tests/test_background_modes_gpu.py uses for the same run."""
    p, art, twin = hyper
    kinds = np.array([[4.7, 0.3, 2e-3], [2.5, -0.2, 2e-2], [2.2, 0.1, 1e-2], [3.0, 0.5, 0.0]])
    x = np.tile(kinds[:, :2], (65, 1))[:257]
    H = np.sqrt((x[:, 0] - 1) ** 2 / 6)
    v = np.stack([-(x[:, 0] - 1) / (3 * H), np.tile(kinds[:, 2], 65)[:257]], axis=1)
    kind = np.arange(257) % 4
    v[kind == 3] = 0.0
    x[:, 1] += np.linspace(0.0, 0.3, 257)  # (theta is cyclic: every lane its own start, the same physics)
    init = np.concatenate([x, v], axis=1)
    kappa = 2.0 * tn.friedmann_h(twin, p, init)
    kappa[256] = 0.0
    expected = np.array([TARGET, COMPLETE, ENDED, TARGET], dtype=np.int8)[kind]
    expected[256] = NONFINITE
    got = _lanes(bg, art, p, init, kappa, 0.2, max_steps=5, solver=solver, dt=0.05)
    want = twin.lanes(p, init, kappa, 0.2, max_steps=5, solver=solver, dt=0.05)
    assert np.array_equal(got.status, expected) and np.array_equal(got.status, want.status)
    emits = (expected == TARGET) | (expected == ENDED)
    assert np.isfinite(got.out[:, emits]).all() and np.isnan(got.out[:, ~emits]).all() and np.all(got.out[0, emits] > 0.0)
    diff = tn.relative_error(got.out[0, emits], want.out[0, emits])
    print(f"{solver}: worst relative |GPU - host twin| {diff:.3e}; P_T of a lane at rest {got.out[0, 3]:.6e}")
    assert diff <= 1e-11 and np.allclose(got.out[5:, emits], want.out[5:, emits], rtol=0, atol=1e-11)
    ended = expected == ENDED
    assert np.all(got.out[7, ended] == 1.0) and np.array_equal(got.out[5, ended], got.N_end[ended]) and np.all(got.out[5, expected == TARGET] == 0.2)
    assert np.all(got.N_end[ended] < 0.2) and np.all(got.N_end[ended] > 0.0) and np.isnan(got.N_end[~ended]).all()
    # theta is cyclic and every lane of a kind starts from the same phi and velocities: the same values bit for bit
    assert np.array_equal(got.out[:, ended], np.repeat(got.out[:, 2:3], ended.sum(), axis=1))


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", ["egno", "d5"])
def test_heavy_example_models_against_twin(bg, name, solver):
    """The tensor objects of the two example models with the highest register demand (D5's advance kernels fill the register file),
    adaptive at the default max_err over a short span, kappa = H0 e^3: ``status`` is the host twin's and P_T agrees with it to the
    project's parity bar, 1e-10 of its size.  The lanes are those of tests/test_background_modes_gpu.py: EGNO's 64 seeds to
    N = 0.02, 257 lanes of D5 to N = 2e-4."""
    from background_sampled_reference import EGNO_SEEDS
    from test_background import VELOCITY, _points, initial_state

    spec, art = workloads.artifact_for(name)
    if name == "egno":
        init, target = np.array([initial_state("egno", seed) for seed in EGNO_SEEDS]), 0.02
    else:
        init, target = _points(name, 257) * np.array([1, 1, VELOCITY[name], VELOCITY[name]]), 2e-4
    twin = tn.TensorTwin(art)
    kappa = tn.friedmann_h(twin, spec.args, init) * math.exp(tn.N_SUB)
    got = _lanes(bg, art, spec.args, init, kappa, target, solver=solver, stop_at_end=False)
    want = twin.lanes(spec.args, init, kappa, target, solver=solver, stop_at_end=False)
    assert np.array_equal(got.status, want.status) and np.all(got.status == TARGET)
    rel = tn.relative_error(got.out[0], want.out[0])
    modes = np.max(np.abs(got.out[1:5] - want.out[1:5]) / np.maximum(np.abs(want.out[1:5]), 1e-3))
    print(f"{name} {solver}: worst relative |GPU - host twin| {rel:.3e} (the 4 mode components, floor 1e-3: {modes:.3e}); {want.accepted.min()} .. {want.accepted.max()} steps")
    assert rel <= 1e-10


def test_power_law_spectrum_is_the_exact_one(bg):
    """Truth (c') on the GPU, through the front end: P_T within twice the recorded start error of the exact formula, and
    P_T = 16 eps P_S of the device's own ``power_spectra`` -- the flat second field is a massless spectator that obeys the tensor
    equation -- within the sum of the two bounds; k = H_k e^N_exit."""
    import background_reference as br

    art, p, init, h_k = mo.power_law_case()
    want, bound = tn.power_law_formula(h_k), tn.power_law_bound()
    kw = dict(N_eval=mo.POWER_N_EVAL, N_sub=tn.N_SUB, stop_at_end=False)
    ts = bg.tensor_spectra(art, p, mo.POWER_N_EXIT, init[None, :2], init[None, 2:], **kw)
    ps = bg.power_spectra(art, p, mo.POWER_N_EXIT, init[None, :2], init[None, 2:], **kw)
    assert np.all(ts.status == TARGET) and np.all(ts.N == mo.POWER_N_EVAL) and np.isnan(ts.N_end).all() and np.array_equal(ts.k, ps.k)
    err, rel = np.abs(ts.P_T[0] - want) / want, np.abs(ts.P_T[0] / (16.0 / br.P_POW * ps.P_S[0]) - 1.0)
    print(f"power law: |P_T - formula| / formula {err.max():.3e} (bound {bound:.3e}), |P_T / (16 eps P_S) - 1| {rel.max():.3e} (bound {bound + mo.power_law_bound():.3e})")
    assert err.max() <= bound and rel.max() <= bound + mo.power_law_bound()
    assert np.allclose(ts.k[0], h_k * np.exp(mo.POWER_N_EXIT), rtol=1e-7)


def test_tensor_object_of_another_layout_is_refused(bg):
    """An object built with -DINFLX_TN_ABI_VERSION=2 is refused with INFLX_ERR_VERSION, a missing one is INFLX_ERR_SYMBOL with the
    way to build it; the artefact's own build then replaces the refused file and works on the same handle."""
    from background_reference import power_law_artifact, power_law_init
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".tensor"
    headers = {stale + ".model.h": header_text, stale + ".eom.h": art.eom_header_text()}
    init = np.array([power_law_init()], dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    kappa, target = np.array([100.0]), np.array([1e-3])
    out, status = np.empty((8, 1)), np.empty(1, dtype=np.int8)
    dp = C.POINTER(C.c_double)
    flags = _native.MODES_TENSOR

    def raw(lib):  # the C entry point's own return code
        return lib._lib.inflx_mode_spectra(lib._h, p.ctypes.data_as(dp), 1, lib.n_parameters, init.ctypes.data_as(dp), 1, kappa.ctypes.data_as(dp), target.ctypes.data_as(dp),
                                           1000, _native.EOM_RKF, 1e-8, 0.0, flags, out.ctypes.data_as(dp), None, status.ctypes.data_as(C.POINTER(C.c_int8)))  # fmt: skip

    try:
        if os.path.exists(stale):
            os.remove(stale)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        assert raw(lib) == _native.ERR_SYMBOL
        with pytest.raises(SystemError, match=r"ensure_tensor\(\)") as err:
            lib.mode_spectra(p, init, kappa, target, 1000, _native.EOM_RKF, 1e-8, 0.0, flags)
        assert ".tensor exists" in str(err.value)
        for path, text in headers.items():
            with open(path, "w") as fh:
                fh.write(text)
        hdr, eom_hdr = headers
        cmd = [hipcc_path(), *options, "-DINFLX_TN_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', os.path.join(_CSRC, "inflx_tensor_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        assert raw(lib) == _native.ERR_VERSION
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.mode_spectra(p, init, kappa, target, 1000, _native.EOM_RKF, 1e-8, 0.0, flags)
        assert "INFLX_TN_ABI 2, expected 1" in str(err.value)
        os.remove(stale)
        art.ensure_tensor()
        got = lib.mode_spectra(p, init, kappa, target, 1000, _native.EOM_RKF, 1e-8, 0.0, flags)
        assert got[0].shape == (8, 1) and got[2][0] == TARGET and np.isfinite(got[0]).all()
        lib.close()
    finally:
        for path in (stale, *headers):
            if os.path.exists(path):
                os.remove(path)


def test_the_flag_does_not_leak_into_the_scalar_path(bg):
    """``mode_spectra`` without the flag on one zoo model, 65 lanes: the same 22 planes, N_end and statuses bit for bit before and
    after a tensor call on the same handle, and the tensor call itself is repeatable."""
    from inflatox_amd import _native

    name = "fuzz0"
    art = bt.device_artifact(name)
    init, pars, kappa, target = tn.zoo_lanes(name)
    art.ensure_modes()
    art.ensure_tensor()
    lib = bg._dylib(art, background=False)
    args = (pars, init, kappa, np.full(len(init), target), 20_000, _native.EOM_RKF, 1e-8, 0.0)
    before = lib.mode_spectra(*args, 0)
    tensor = lib.mode_spectra(*args, _native.MODES_TENSOR)
    after = lib.mode_spectra(*args, 0)
    again = lib.mode_spectra(*args, _native.MODES_TENSOR)
    assert before[0].shape == (22, len(init)) and tensor[0].shape == (8, len(init)) and np.all(before[2] == TARGET) and np.all(tensor[2] == TARGET)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after)) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(tensor, again))


def test_observables_on_the_power_law_are_the_exact_ones(bg):
    """``observables`` on the device at the pivot N_exit = 3.5, dN = 0.5, N_sub = 3, N = 10: n_s - 1 = n_t = -2/7, r = 2, alpha_s = 0,
    each within the bound tests/test_background_tensor.py derives from the two recorded power-law errors and the stencil's weights."""
    import background_reference as br

    art, p, init, _h = mo.power_law_case()
    obs = bg.observables(art, p, [3.5], init[None, :2], init[None, 2:], dN=0.5, N_eval=mo.POWER_N_EVAL, N_sub=tn.N_SUB, stop_at_end=False)
    assert isinstance(obs, bg.Observables) and obs.n_s.shape == (1, 1) and obs.status[0, 0] == TARGET
    eps = 1.0 / br.P_POW
    tilt = -2.0 * eps / (1.0 - eps)
    k3 = tn.power_law_exits([3.0, 3.5, 4.0]) * np.exp([3.0, 3.5, 4.0])
    b_ns, b_alpha, b_nt, b_r = tn.stencil_bounds(k3, mo.power_law_bound(), tn.power_law_bound())
    print(f"power law: n_s - 1 {obs.n_s[0, 0] - 1:.6f} and n_t {obs.n_t[0, 0]:.6f} (exact {tilt:.6f}; bounds {b_ns:.2e}, {b_nt:.2e}), r {obs.r[0, 0]:.6f} (bound {b_r:.2e} "
          f"of 2), alpha_s {obs.alpha_s[0, 0]:.2e} (bound {b_alpha:.2e})")  # fmt: skip
    assert abs(obs.n_s[0, 0] - 1.0 - tilt) <= b_ns and abs(obs.n_t[0, 0] - tilt) <= b_nt and abs(obs.alpha_s[0, 0]) <= b_alpha
    assert abs(obs.r[0, 0] / (16.0 * eps) - 1.0) <= b_r and np.isclose(obs.k[0, 0], k3[1], rtol=1e-7)


def test_observables_map_is_its_two_halves(bg, hyper):
    """A 6 x 5 grid of the hyperbolic model from rest with N_star = 50 and the defaults N_sub = 5, dN = 0.5, over a range whose
    lowest rows inflate for fewer than 55.5 e-folds: ``observables_map`` equals ``horizon_exit_map`` at N_star + N_sub + dN followed
    by ``observables`` with ``N_exit=[N_sub + dN]`` from the states found, bit for bit, and is NaN exactly where no state was found.
    n_s and r of the grid are printed."""
    p, art, _twin = hyper
    ss = [[14.0, 19.0], [-1.0, 1.0]]
    obs, state, n_end, status = bg.observables_map(art, p, ss, 6, 5, N_star=50.0, return_status=True)
    short = bg.observables_map(art, p, ss, 6, 5, N_star=50.0)
    state2, n_end2, status2 = bg.horizon_exit_map(art, p, ss, 6, 5, N_star=55.5, return_status=True)
    assert np.array_equal(state, state2, equal_nan=True) and np.array_equal(n_end, n_end2, equal_nan=True)
    found = status2 == TARGET
    assert 0 < found.sum() < 30 and isinstance(obs, bg.Observables) and all(member.shape == (6, 5) for member in obs)
    flat = state2[found]
    half = bg.observables(art, p, [5.5], flat[:, :2], flat[:, 2:4], dN=0.5, N_sub=5.0, max_steps=100_000)
    with np.printoptions(precision=5, linewidth=200):
        print(f"n_s:\n{obs.n_s}\nr:\n{obs.r}")
    for grid, member in zip(obs[:-1], half[:-1]):
        assert np.array_equal(grid[found], member[:, 0], equal_nan=True) and np.isnan(grid[~found]).all()
    assert np.array_equal(obs.status, status) and np.array_equal(status[found], half.status[:, 0]) and np.array_equal(status[~found], status2[~found])
    ended = status == ENDED
    assert np.array_equal(ended, found) and all(np.isfinite(member[ended]).all() for member in obs[:-1])
    assert len(short) == 3 and all(np.array_equal(u, w, equal_nan=True) for u, w in zip(short[0], obs))
