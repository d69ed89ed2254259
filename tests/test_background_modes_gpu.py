"""Mode functions and power spectra on the GPU (inflatox_amd.background.power_spectra, spectrum_map, InflatoxDevLib.mode_spectra):
the kernels against truth (b) and the host twin on the curved zoo, a run of several launches with its lane numbering and lane
independence, every stop status side by side, the two heaviest example models, truths (a) and (c), ``spectrum_map`` against its two
halves and the refusal of a modes object of another layout.  Truths, twin and bounds are those tests/test_background_modes.py
establishes on the host build (tests/modes_reference.py, profiles/background_modes.json); every difference is printed."""

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import background_truth as bt
import kinematics_reference as kr
import modes_reference as mo
import workloads
from modes_reference import COMPLETE, ENDED, NONFINITE, TARGET

pytestmark = pytest.mark.gpu

MEMBERS = ("P_R", "P_S", "C_RS", "k", "N", "eps_H", "modes", "N_end", "status")


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return spec.args, art, mo.ModesTwin(art)


def _lanes(bg, art, pars, init, kappa, target, max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None, stop_at_end=True):
    """``InflatoxDevLib.mode_spectra`` on the artefact's handle, as a ``TwinLanes`` without ``accepted`` and ``final``"""
    from inflatox_amd import _native

    art.ensure_modes()
    n = len(init)
    out, n_end, status = bg._dylib(art, background=False).mode_spectra(
        pars, init, np.broadcast_to(np.asarray(kappa, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(target, dtype=np.float64), (n,)), max_steps,
        bg._METHODS[solver], max_err, dt or 0.0, _native.EOM_STOP_AT_END if stop_at_end else 0)  # fmt: skip
    return mo.TwinLanes(out, n_end, status, None, None)


def _same(a, b, rows=slice(None), cols=slice(None)):
    """the members of two PowerSpectra, bit for bit and NaN where NaN; ``rows``, ``cols`` select from ``a``"""
    return all(np.array_equal(getattr(a, m)[rows][:, cols], getattr(b, m), equal_nan=True) for m in MEMBERS)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_kernel_against_truth_and_twin(bg, name, solver):
    """All 257 lanes of ``background_truth.batch`` (four wavefronts and one lane, B = 257 and K = 1), a parameter row per lane,
    kappa = H0 e^3, the default max_err = 1e-8, at most 20 000 steps.  ``status`` is the host twin's on every lane; on the lanes
    the twin reports TARGET -- all but five of fuzz1 and two of fuzz3, whose velocity passes through zero, where Omega is singular:
    they UNDERFLOW (rk4) or crawl until the steps run out (rkf), on both sides -- the spectra are within the bound of the twin
    (relative to each spectrum's own scale; the difference is printed).  Truth (b) is established for the first 65 lanes (the
    others are not known to keep H > 0), every one of which is TARGET: there the spectra are within the bound of it."""
    art = bt.device_artifact(name)
    init, pars, kappa, target = mo.zoo_lanes(name, 257)
    assert init.shape == (257, 4) and pars.shape == (257, art.n_parameters)
    truth = mo.zoo_truth(name)
    got = _lanes(bg, art, pars, init, kappa, target, max_steps=20_000, solver=solver, stop_at_end=False)
    twin = mo.zoo_twin(name).lanes(pars, init, kappa, target, max_steps=20_000, solver=solver, stop_at_end=False)
    ok = twin.status == TARGET
    bound = mo.bound(name, solver, 1e-8)
    err = mo.relative_error(got.out[:3, : mo.LANES], truth[:3])
    diff = mo.relative_error(got.out[:3][:, ok], twin.out[:3][:, ok])
    print(f"{name} {solver}: worst relative |GPU - truth (b)| {err:.3e} (bound {bound:.3e}), worst relative |GPU - host twin| on {ok.sum()} TARGET lanes {diff:.3e}")
    assert got.out.shape == (22, 257) and np.array_equal(got.status, twin.status)
    assert ok[: mo.LANES].all() and ok.sum() >= 250
    assert np.isfinite(got.out[:, ok]).all() and np.isnan(got.out[:, ~ok]).all() and err <= bound and diff <= bound
    assert np.all(got.out[19, ok] == target) and np.isnan(got.N_end).all()


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_several_launches_lane_numbering_and_lane_independence(bg, hyper, solver):
    """B = 5 trajectories high on the hyperbolic potential, K = 52 wavenumbers with N_exit = 3 .. 3.51, N_sub = 3, max_err = 1e-10: 260
    lanes, each of more than 256 accepted steps by the twin's count, so two or more launches and a carried state.  Lane b K + j is
    trajectory b with wavenumber j: the twin, fed the device's own first stage, has the same statuses; evaluated at N = 6 the spectra
    are within the bound of the twin's own error there (profiles/background_modes.json), lane by lane.  To the end of inflation the
    values are linear across the last step and carry that interpolation's error, and the trajectory's last e-folds amplify a
    rounding (FMA contraction alone moves the host build's N_end by 2e-9 and its end spectra by 8e-9 of their scale on these lanes;
    the device's are 3e-9 and 1e-8 from the uncontracted host build, printed): there N_end agrees with the twin's to 1e-3, the
    accuracy ``efolds_map`` documents for it, and a permuted batch and the sub-batches (B, K) = (1, 1) and (5, 13) give the same
    lanes bit for bit."""
    p, art, twin = hyper
    x, v = mo.hyper_states()
    kw = dict(N_sub=mo.N_SUB, max_err=mo.HYPER_MAX_ERR, solver=solver)
    pts = np.unique(np.concatenate([mo.HYPER_N_EXIT - mo.N_SUB, mo.HYPER_N_EXIT]))
    stage1 = bg.solve_eom_sampled(art, p, pts, x, v, 1_000_000, mo.HYPER_MAX_ERR, solver)
    at = bg.power_spectra(art, p, mo.HYPER_N_EXIT, x, v, N_eval=mo.HYPER_N_EVAL, **kw)
    want = twin.power_spectra(p, mo.HYPER_N_EXIT, x, v, N_eval=mo.HYPER_N_EVAL, stage1=stage1, **kw)
    assert isinstance(at, bg.PowerSpectra) and at.P_R.shape == (mo.HYPER_B, mo.HYPER_K) and at.modes.shape == (mo.HYPER_B, mo.HYPER_K, 2, 2)
    assert np.all(at.status == TARGET) and np.array_equal(at.status, want.status) and want.accepted.min() > 256
    diff, bound = mo.relative_error((at.P_R, at.P_S, at.C_RS), (want.P_R, want.P_S, want.C_RS)), mo.hyper_bound(solver)
    print(f"{solver}: {want.accepted.min()} .. {want.accepted.max()} accepted steps to N = {mo.HYPER_N_EVAL:g}, worst relative |GPU - host twin| {diff:.3e} (bound {bound:.3e})")
    assert np.isfinite(at.P_R).all() and diff <= bound and np.array_equal(at.k, want.k) and np.all(at.N == mo.HYPER_N_EVAL) and np.isnan(at.N_end).all()
    assert np.all(np.diff(at.k, axis=1) > 0) and np.allclose(at.modes, want.modes, rtol=0, atol=bound * np.abs(want.modes).max())
    got = bg.power_spectra(art, p, mo.HYPER_N_EXIT, x, v, **kw)
    end = twin.power_spectra(p, mo.HYPER_N_EXIT, x, v, stage1=stage1, **kw)
    print(f"{solver}: {end.accepted.min()} .. {end.accepted.max()} accepted steps to the end, worst |N_end - host twin's| {np.abs(got.N_end - end.N_end).max():.3e}, "
          f"worst relative |GPU - host twin| there {mo.relative_error((got.P_R, got.P_S, got.C_RS), (end.P_R, end.P_S, end.C_RS)):.3e}")  # fmt: skip
    assert np.all(got.status == ENDED) and np.array_equal(got.status, end.status) and end.accepted.min() > 256
    assert np.isfinite(got.P_R).all() and np.all(got.eps_H == 1.0) and np.array_equal(got.N, got.N_end) and np.abs(got.N_end - end.N_end).max() <= 1e-3
    assert np.array_equal(got.k, at.k)
    perm = np.random.default_rng(9).permutation(mo.HYPER_B)
    assert _same(got, bg.power_spectra(art, p, mo.HYPER_N_EXIT, x[perm], v[perm], **kw), perm)
    assert _same(got, bg.power_spectra(art, p, mo.HYPER_N_EXIT[17:18], x[3:4], v[3:4], **kw), slice(3, 4), slice(17, 18))
    assert _same(got, bg.power_spectra(art, p, mo.HYPER_N_EXIT[39:], x, v, **kw), slice(None), slice(39, 52))


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_every_status_side_by_side(bg, hyper, solver):
    """257 lanes of four kinds, in turn, five steps of dt = 0.05, kappa = 2 H0 and the target N = 0.2: a lane high on the potential
    reaches it (TARGET); a slower one runs out of steps (COMPLETE, all NaN); one that starts 0.05 e-folds before epsilon_H = 1 ends
    there (ENDED: the values at the end, eps_H = 1); one at rest is NONFINITE, all NaN.  Five steps leave the host twin and the
    device a few roundings apart: 1e-11 of each spectrum's scale."""
    p, art, twin = hyper
    kinds = np.array([[4.7, 0.3, 2e-3], [2.5, -0.2, 2e-2], [2.2, 0.1, 1e-2], [3.0, 0.5, 0.0]])
    x = np.tile(kinds[:, :2], (65, 1))[:257]
    H = np.sqrt((x[:, 0] - 1) ** 2 / 6)
    v = np.stack([-(x[:, 0] - 1) / (3 * H), np.tile(kinds[:, 2], 65)[:257]], axis=1)
    kind = np.arange(257) % 4
    v[kind == 3] = 0.0
    x[:, 1] += np.linspace(0.0, 0.3, 257)  # (theta is cyclic: every lane its own start, the same physics)
    init = np.concatenate([x, v], axis=1)
    kappa = 2.0 * mo.friedmann_h(twin, p, init)
    got = _lanes(bg, art, p, init, kappa, 0.2, max_steps=5, solver=solver, dt=0.05)
    want = twin.lanes(p, init, kappa, 0.2, max_steps=5, solver=solver, dt=0.05)
    assert np.array_equal(got.status, np.array([TARGET, COMPLETE, ENDED, NONFINITE], dtype=np.int8)[kind]) and np.array_equal(got.status, want.status)
    emits = (kind == 0) | (kind == 2)
    assert np.isfinite(got.out[:, emits]).all() and np.isnan(got.out[:, ~emits]).all()
    diff = mo.relative_error(got.out[:3][:, emits], want.out[:3][:, emits])
    print(f"{solver}: worst relative |GPU - host twin| {diff:.3e}")
    assert diff <= 1e-11 and np.allclose(got.out[19:, emits], want.out[19:, emits], rtol=0, atol=1e-11)
    ended = kind == 2
    assert np.all(got.out[21, ended] == 1.0) and np.array_equal(got.out[19, ended], got.N_end[ended]) and np.all(got.out[19, kind == 0] == 0.2)
    assert np.all(got.N_end[ended] < 0.2) and np.all(got.N_end[ended] > 0.0) and np.isnan(got.N_end[~ended]).all()
    # theta is cyclic and every lane of a kind starts from the same phi and velocities: the same values bit for bit
    assert np.array_equal(got.out[:, ended], np.repeat(got.out[:, 2:3], ended.sum(), axis=1))


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", ["egno", "d5"])
def test_heavy_example_models_against_twin(bg, name, solver):
    """The modes objects of the two example models with the highest register demand, adaptive at the default max_err over a short
    span, kappa = H0 e^3: ``status`` is the host twin's and the spectra agree with it to the project's parity bar, 1e-10 of each
    spectrum's scale -- FMA contraction alone moves the host build by 2e-13 (EGNO) and 5e-12 (D5) of that scale on these lanes.
    EGNO: the 64 seeds of ``background_sampled_reference.EGNO_SEEDS``, to N = 0.02.  D5: 257 lanes of ``test_background._points``,
    to N = 2e-4 (13 to 20 accepted steps)."""
    from background_sampled_reference import EGNO_SEEDS
    from test_background import VELOCITY, _points, initial_state

    spec, art = workloads.artifact_for(name)
    if name == "egno":
        init, target = np.array([initial_state("egno", seed) for seed in EGNO_SEEDS]), 0.02
    else:
        init, target = _points(name, 257) * np.array([1, 1, VELOCITY[name], VELOCITY[name]]), 2e-4
    twin = mo.ModesTwin(art)
    kappa = mo.friedmann_h(twin, spec.args, init) * math.exp(mo.N_SUB)
    got = _lanes(bg, art, spec.args, init, kappa, target, solver=solver, stop_at_end=False)
    want = twin.lanes(spec.args, init, kappa, target, solver=solver, stop_at_end=False)
    assert np.array_equal(got.status, want.status) and np.all(got.status == TARGET)
    rel = mo.relative_error(got.out[:3], want.out[:3])
    modes = np.max(np.abs(got.out[3:19] - want.out[3:19]) / np.maximum(np.abs(want.out[3:19]), 1e-3))
    print(f"{name} {solver}: worst relative |GPU - host twin| {rel:.3e} (the 16 mode components, floor 1e-3: {modes:.3e}); {want.accepted.min()} .. {want.accepted.max()} steps")
    assert rel <= 1e-10


def test_plane_against_the_field_basis_system(bg):
    """Truth (a) on the GPU: the 17 Cartesian plane states at the default max_err, within the bound the host build establishes."""
    from inflatox_amd import Compiler

    _pa, ca, _pp, cp, _ps, _cs, a, b = mo.plane_case()
    cs, kappa = mo.plane_lanes()
    _polar, cart = kr.plane_models()
    art = Compiler(cart, silent=True).compile()
    assert art.symbol_dictionary == ca.symbol_dictionary
    got = _lanes(bg, art, cp, cs[:, :4], kappa, mo.PLANE_TARGET, stop_at_end=False)
    assert np.all(got.status == TARGET)
    err, bound = mo.plane_error(got, cs, kappa, a, b), mo.plane_bound("rkf", 1e-8)
    print(f"plane: worst relative |GPU - truth (a)| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_power_law_spectrum_is_the_exact_one(bg):
    """Truth (c) on the GPU, through the front end: P_R within twice the recorded start error of the exact formula, P_S = P_R within
    the same bound, no correlation, and k = H_k e^N_exit."""
    art, p, init, h_k = mo.power_law_case()
    want, bound = mo.power_law_formula(h_k), mo.power_law_bound()
    ps = bg.power_spectra(art, p, mo.POWER_N_EXIT, init[None, :2], init[None, 2:], N_eval=mo.POWER_N_EVAL, N_sub=mo.N_SUB, stop_at_end=False)
    assert np.all(ps.status == TARGET) and np.all(ps.N == mo.POWER_N_EVAL) and np.isnan(ps.N_end).all()
    err_r, err_s = np.abs(ps.P_R[0] - want) / want, np.abs(ps.P_S[0] / ps.P_R[0] - 1.0)
    print(f"power law: |P_R - formula| / formula {err_r.max():.3e}, |P_S / P_R - 1| {err_s.max():.3e} (bound {bound:.3e})")
    assert err_r.max() <= bound and err_s.max() <= bound and np.all(np.abs(ps.C_RS) <= 1e-12 * ps.P_R)
    assert np.allclose(ps.k[0], h_k * np.exp(mo.POWER_N_EXIT), rtol=1e-7)


def test_spectrum_map_is_its_two_halves(bg, hyper):
    """A 5 x 7 grid over a range that holds points too close to the end of inflation for N_star + N_sub = 0.8: ``spectrum_map``
    equals ``horizon_exit_map`` at N_star + N_sub followed by ``power_spectra`` with ``N_exit=[N_sub]`` from the states found, bit
    for bit, NaN where no state was found."""
    p, art, _twin = hyper
    ss, d = [[1.8, 4.0], [-1.0, 1.0]], (-0.2, 1e-3)
    kw = dict(N_star=0.5, N_sub=0.3, derivatives_init=d)
    (p_r, p_s, c_rs), state, n_end, status = bg.spectrum_map(art, p, ss, 5, 7, return_status=True, **kw)
    short = bg.spectrum_map(art, p, ss, 5, 7, **kw)
    state2, n_end2, status2 = bg.horizon_exit_map(art, p, ss, 5, 7, N_star=0.8, derivatives_init=d, return_status=True)
    assert np.array_equal(state, state2, equal_nan=True) and np.array_equal(n_end, n_end2, equal_nan=True)
    found = status2 == TARGET
    assert 0 < found.sum() < 35 and p_r.shape == p_s.shape == c_rs.shape == status.shape == (5, 7)
    flat = state2[found]
    ps = bg.power_spectra(art, p, [0.3], flat[:, :2], flat[:, 2:4], N_sub=0.3, max_steps=100_000)
    assert np.all(ps.status == ENDED)
    for grid, member in ((p_r, ps.P_R), (p_s, ps.P_S), (c_rs, ps.C_RS)):
        assert np.array_equal(grid[found], member[:, 0]) and np.isfinite(grid[found]).all() and np.isnan(grid[~found]).all()
    assert np.array_equal(status[found], ps.status[:, 0]) and np.array_equal(status[~found], status2[~found])
    assert len(short) == 3 and all(np.array_equal(u, w, equal_nan=True) for u, w in zip(short[0], (p_r, p_s, c_rs)))
    # the states are about N_star + N_sub from the end, and the second stage finds about that many e-folds again
    assert np.abs(ps.N_end[:, 0] - 0.8).max() < 0.05 and np.all(p_r[found] > 0) and np.all(p_s[found] > 0)


def test_modes_object_of_another_layout_is_refused(bg):
    """An object built with -DINFLX_MD_ABI_VERSION=2 is refused with INFLX_ERR_VERSION, a missing one is INFLX_ERR_SYMBOL with the
    way to build it; the artefact's own build then replaces the refused file and works on the same handle."""
    from background_reference import power_law_artifact, power_law_init
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".modes"
    headers = {stale + ".model.h": header_text, stale + ".eom.h": art.eom_header_text(), stale + ".kin.h": art.kinematics_header_text(),
               stale + ".mass.h": art.masses_header_text()}  # fmt: skip
    init = np.array([power_law_init()], dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    kappa, target = np.array([100.0]), np.array([1e-3])
    out, status = np.empty((22, 1)), np.empty(1, dtype=np.int8)
    dp = C.POINTER(C.c_double)

    def raw(lib):  # the C entry point's own return code
        return lib._lib.inflx_mode_spectra(lib._h, p.ctypes.data_as(dp), 1, lib.n_parameters, init.ctypes.data_as(dp), 1, kappa.ctypes.data_as(dp), target.ctypes.data_as(dp),
                                           1000, _native.EOM_RKF, 1e-8, 0.0, 0, out.ctypes.data_as(dp), None, status.ctypes.data_as(C.POINTER(C.c_int8)))  # fmt: skip

    try:
        if os.path.exists(stale):
            os.remove(stale)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        assert raw(lib) == _native.ERR_SYMBOL
        with pytest.raises(SystemError, match=r"ensure_modes\(\)") as err:
            lib.mode_spectra(p, init, kappa, target, 1000, _native.EOM_RKF, 1e-8, 0.0, 0)
        assert ".modes exists" in str(err.value)
        for path, text in headers.items():
            with open(path, "w") as fh:
                fh.write(text)
        hdr, eom_hdr, kin_hdr, mass_hdr = headers
        cmd = [hipcc_path(), *options, "-DINFLX_MD_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_KIN_HEADER="{kin_hdr}"', f'-DINFLX_MASS_HEADER="{mass_hdr}"',
               os.path.join(_CSRC, "inflx_modes_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        assert raw(lib) == _native.ERR_VERSION
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.mode_spectra(p, init, kappa, target, 1000, _native.EOM_RKF, 1e-8, 0.0, 0)
        assert "INFLX_MD_ABI 2, expected 1" in str(err.value)
        os.remove(stale)
        art.ensure_modes()
        got = lib.mode_spectra(p, init, kappa, target, 1000, _native.EOM_RKF, 1e-8, 0.0, 0)
        assert got[0].shape == (22, 1) and got[2][0] == TARGET and np.isfinite(got[0]).all()
        lib.close()
    finally:
        for path in (stale, *headers):
            if os.path.exists(path):
                os.remove(path)


def test_more_than_one_pass_is_the_same_lanes_run_alone(bg, hyper):
    """n = 2^20 + 257 scalar lanes -- a pass holds at most 2^20 --, two fixed steps of dt = 0.01, as in
    tests/test_background_tensor_gpu.py: every lane with a target of 0.02 e-folds reaches it within them (TARGET, values emitted), the
    others run out of steps (COMPLETE, NaN).  The first five lanes, the lanes on either side of the seam and the last five are the
    same lanes run alone, bit for bit and NaN where NaN, in every returned array; lanes on both sides of the seam hold values."""
    p, art, _twin = hyper
    n, first = (1 << 20) + 257, 1 << 20
    rng = np.random.default_rng(5)
    x = np.stack([rng.uniform(4.5, 5.0, n), rng.uniform(-1.0, 1.0, n)], axis=1)
    init = np.concatenate([x, np.stack([np.full(n, -0.8), rng.uniform(-1e-3, 1e-3, n)], axis=1)], axis=1)
    kappa = rng.uniform(2.0, 6.0, n)
    target = np.where(np.arange(n) % 3 == 2, np.nan, 0.02)
    kw = dict(max_steps=2, dt=0.01)
    whole = _lanes(bg, art, p, init, kappa, target, **kw)
    assert whole.out.shape == (22, n) and np.array_equal(whole.status, np.where(np.isnan(target), COMPLETE, TARGET))
    assert np.isfinite(whole.out[:, whole.status == TARGET]).all() and np.isnan(whole.out[:, whole.status == COMPLETE]).all()
    assert (whole.status[first - 3 : first] == TARGET).any() and (whole.status[first : first + 3] == TARGET).any()
    for sl in (slice(0, 5), slice(first - 3, first + 3), slice(n - 5, n)):
        alone = _lanes(bg, art, p, init[sl], kappa[sl], target[sl], **kw)
        for a, b in zip(whole[:3], alone[:3]):
            assert np.array_equal(a[..., sl], b, equal_nan=True), sl
