"""Super-horizon transfer functions on the GPU (inflatox_amd.background.transfer_functions, transfer_map): the kernels against truth
(b) and the host twin on the curved zoo, the background of a fixed-dt run against ``solve_eom_sampled`` bit for bit, a run of
several launches, lane independence, every stop status side by side, ``transfer_map`` against its two halves, the refusal of a
transfer object of another layout, and truth (a) on the plane.  Truths, twin and bounds are those tests/test_background_transfer.py
establishes on the host build (tests/transfer_reference.py, profiles/background_transfer.json)."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import background_truth as bt
import kinematics_reference as kr
import transfer_reference as tr
import workloads
from transfer_reference import COMPLETE, ENDED, NONFINITE, TARGET

pytestmark = pytest.mark.gpu

MEMBERS = ("T_SS", "T_RS", "t", "N", "eps_H", "states", "n_stored", "N_end", "T_SS_end", "T_RS_end", "status")


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return spec.args, art, tr.TransferTwin(art)


def _same(a, b, lanes=slice(None)):
    """the members of two solutions, bit for bit and NaN where NaN; ``lanes`` selects from ``a``"""
    return all(np.array_equal(getattr(a, m)[lanes], getattr(b, m), equal_nan=True) for m in MEMBERS)


def _to_twin(got, twin):
    """worst |GPU - host twin| over T_SS and T_RS where both are finite"""
    with np.errstate(invalid="ignore"):
        return float(max(np.nanmax(np.abs(got.T_SS - twin.T_SS)), np.nanmax(np.abs(got.T_RS - twin.T_RS))))


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_kernel_against_truth_and_twin(bg, name, solver):
    """All 257 lanes of ``background_truth.batch`` (four wavefronts and one lane), a parameter row per lane, the default max_err =
    1e-8.  ``n_stored`` and ``status`` are the host twin's on every lane; on the lanes the twin reports TARGET -- all but five of
    fuzz1 and two of fuzz3, whose velocity passes through zero, where omega is singular, and which UNDERFLOW on both sides -- T_SS
    and T_RS are within the bound of the twin (the difference is printed; FMA contraction alone moves the host build by 1e-10 at
    the most there).  Truth (b) is established for the first 65 lanes (the others are not known to keep H > 0): there T_SS and T_RS
    are within the bound of it at all four samples."""
    art = bt.device_artifact(name)
    init, pars = bt.batch(name)
    assert init.shape == (257, 4) and pars.shape == (257, art.n_parameters)
    samples, truth = tr.zoo_truth(name)
    got = bg.transfer_functions(art, pars, samples, init[:, :2], init[:, 2:], solver=solver, stop_at_end=False)
    twin = tr.zoo_twin(name).solve(pars, samples, init[:, :2], init[:, 2:], solver=solver, stop_at_end=False)
    assert isinstance(got, bg.TransferSolution) and got.T_SS.shape == (257, 4) and got.states.shape == (257, 4, 5)
    ok = twin.status == TARGET
    first = type(got)(*(member[: tr.LANES] for member in got))
    err, bound = tr.zoo_error(first, truth), tr.bound(name, solver, 1e-8)
    diff = max(np.abs(got.T_SS[ok] - twin.T_SS[ok]).max(), np.abs(got.T_RS[ok] - twin.T_RS[ok]).max())
    print(f"{name} {solver}: worst |GPU - truth (b)| {err:.3e} (bound {bound:.3e}), worst |GPU - host twin| on {ok.sum()} TARGET lanes {diff:.3e}")
    assert np.array_equal(got.n_stored, twin.n_stored) and np.array_equal(got.status, twin.status)
    assert ok[: tr.LANES].all() and ok.sum() >= 252
    assert np.isfinite(got.T_SS[ok]).all() and np.isfinite(got.T_RS[ok]).all() and err <= bound and diff <= bound
    assert np.array_equal(got.N[ok], np.broadcast_to(samples, (257, 4))[ok])
    # the (B, S[, .]) members are views of the one (S, 10, B) array
    base = got.T_SS.base
    assert base.shape == (4, 10, 257) and all(getattr(got, m).base is base for m in ("T_RS", "t", "N", "eps_H", "states"))
    assert np.isnan(got.N_end).all() and np.isnan(got.T_SS_end).all() and np.isnan(got.T_RS_end).all()


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", ["egno", "d5"])
def test_heavy_example_models_against_twin(bg, name, solver):
    """The transfer objects of the two example models with the highest register demand (362 and 488 registers, DESIGN.md section
    12), adaptive at the default max_err over a short span: ``n_stored`` and ``status`` are the host twin's and T_SS, T_RS agree
    with it to the project's parity bar, 1e-10 of each value's scale (floor 1e-3) -- FMA contraction alone moves the host build by
    7e-12 of that scale on these lanes.  EGNO: the 64 seeds of ``background_sampled_reference.EGNO_SEEDS``, for which the model is
    well conditioned, samples up to N = 0.02.  D5: 257 lanes of ``test_background._points``, samples up to N = 2e-4 (its entropic
    mass is of order 1e6 H^2 there: 14 to 24 accepted steps; N = 0.02 takes 60 000)."""
    from background_sampled_reference import EGNO_SEEDS
    from test_background import VELOCITY, _points, initial_state

    spec, art = workloads.artifact_for(name)
    if name == "egno":
        init, samples = np.array([initial_state("egno", seed) for seed in EGNO_SEEDS]), [0.0, 0.01, 0.02]
    else:
        init, samples = _points(name, 257) * np.array([1, 1, VELOCITY[name], VELOCITY[name]]), [0.0, 1e-4, 2e-4]
    got = bg.transfer_functions(art, spec.args, samples, init[:, :2], init[:, 2:], solver=solver, stop_at_end=False)
    twin = tr.TransferTwin(art).solve(spec.args, samples, init[:, :2], init[:, 2:], solver=solver, stop_at_end=False)
    assert np.array_equal(got.status, twin.status) and np.array_equal(got.n_stored, twin.n_stored) and np.all(got.status == TARGET)
    rel = max(np.max(np.abs(getattr(got, m) - getattr(twin, m)) / np.maximum(np.abs(getattr(twin, m)), 1e-3)) for m in ("T_SS", "T_RS"))
    print(f"{name} {solver}: worst |GPU - host twin| / scale {rel:.3e}; |T_SS - 1| up to {np.abs(twin.T_SS - 1).max():.2e}, |T_RS| up to {np.abs(twin.T_RS).max():.2e}")
    assert rel <= 1e-10 and np.abs(twin.T_SS[:, -1] - 1).max() > 1e-3


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_fixed_dt_background_is_solve_eom_sampled_bit_for_bit(bg, hyper, solver):
    """257 lanes (four wavefronts and one lane) of the hyperbolic model at dt = 2e-3: the steps do not depend on (q, u, r), and the
    first six components are computed with the expressions of the plain stepper."""
    p, art, _twin = hyper
    x, v = tr.hyper_states(257)
    samples = [0.0, 0.02, 0.05, 0.1]
    got = bg.transfer_functions(art, p, samples, x, v, max_steps=2000, solver=solver, dt=2e-3)
    ref = bg.solve_eom_sampled(art, p, samples, x, v, max_steps=2000, solver=solver, dt=2e-3)
    assert np.all(got.status == TARGET) and np.all(got.n_stored == 4)
    for m in ("states", "t", "N", "eps_H", "n_stored", "status"):
        assert np.array_equal(getattr(got, m), getattr(ref, m)), m
    assert np.isfinite(got.T_SS).all() and np.abs(got.T_RS[:, -1]).max() > 1e-3


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_several_launches_and_lane_independence(bg, hyper, solver):
    """257 lanes more than three e-folds from the end, adaptive at max_err = 1e-12, samples up to N = 3: every lane takes more than
    256 accepted steps, so two or more launches and a carried state.  Equal to the same run's twin within the bound of the twin's
    own error there; a permuted batch and the sub-batches B = 1 and 63 give the same lanes bit for bit."""
    p, art, twin = hyper
    x, v = tr.long_states(257)
    kw = dict(max_err=tr.LONG_MAX_ERR, solver=solver)
    got = bg.transfer_functions(art, p, tr.LONG_SAMPLES, x, v, **kw)
    want = twin.solve(p, tr.LONG_SAMPLES, x, v, **kw)
    assert np.all(got.status == TARGET) and np.array_equal(got.n_stored, want.n_stored) and want.accepted.min() > 256
    diff = _to_twin(got, want)
    print(f"{solver}: {want.accepted.min()} .. {want.accepted.max()} accepted steps, worst |GPU - host twin| {diff:.3e} (bound {tr.long_bound(solver):.3e})")
    assert np.isfinite(got.T_SS).all() and np.isfinite(got.T_RS).all() and diff <= tr.long_bound(solver)
    perm = np.random.default_rng(9).permutation(257)
    assert _same(got, bg.transfer_functions(art, p, tr.LONG_SAMPLES, x[perm], v[perm], **kw), perm)
    assert _same(got, bg.transfer_functions(art, p, tr.LONG_SAMPLES, x[100:101], v[100:101], **kw), slice(100, 101))
    assert _same(got, bg.transfer_functions(art, p, tr.LONG_SAMPLES, x[194:], v[194:], **kw), slice(194, 257))


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_every_status_side_by_side(bg, hyper, solver):
    """257 lanes of four kinds, in turn, five steps of dt = 0.05 and the samples N = 0, 0.05, 0.2: a lane high on the potential
    passes every sample (TARGET); a slower one runs out of steps before the last (COMPLETE, its third sample NaN); one that starts
    0.05 e-folds before epsilon_H = 1 ends there (ENDED: two samples, the third NaN, and end values within the bound that linear
    interpolation across the last step allows against the truth with an exact event); one at rest is NONFINITE, all NaN."""
    p, art, twin = hyper
    kinds = np.array([[4.7, 0.3, 2e-3], [2.5, -0.2, 2e-2], [2.2, 0.1, 1e-2], [3.0, 0.5, 0.0]])
    x = np.tile(kinds[:, :2], (65, 1))[:257]
    H = np.sqrt((x[:, 0] - 1) ** 2 / 6)
    v = np.stack([-(x[:, 0] - 1) / (3 * H), np.tile(kinds[:, 2], 65)[:257]], axis=1)
    kind = np.arange(257) % 4
    v[kind == 3] = 0.0
    x[:, 1] += np.linspace(0.0, 0.3, 257)  # (theta is cyclic: every lane its own start, the same physics)
    samples = [0.0, 0.05, 0.2]
    got = bg.transfer_functions(art, p, samples, x, v, max_steps=5, solver=solver, dt=0.05)
    want = twin.solve(p, samples, x, v, max_steps=5, solver=solver, dt=0.05)
    assert np.array_equal(got.status, np.array([TARGET, COMPLETE, ENDED, NONFINITE], dtype=np.int8)[kind])
    assert np.array_equal(got.status, want.status) and np.array_equal(got.n_stored, want.n_stored)
    assert np.array_equal(got.n_stored, np.array([3, 2, 2, 0])[kind])
    reached = np.arange(3)[None, :] < got.n_stored[:, None]
    for m in ("T_SS", "T_RS", "t", "N", "eps_H"):
        assert np.isfinite(getattr(got, m)[reached]).all() and np.isnan(getattr(got, m)[~reached]).all(), m
    assert np.isnan(got.states[kind == 3]).all()
    ended = kind == 2
    for m in ("N_end", "T_SS_end", "T_RS_end"):
        assert np.isfinite(getattr(got, m)[ended]).all() and np.isnan(getattr(got, m)[~ended]).all(), m
        assert np.allclose(getattr(got, m)[ended], getattr(want, m)[ended], rtol=0, atol=1e-11), m
    assert np.all(got.N_end[ended] < 0.2) and np.all(got.N_end[ended] > 0.05)
    g = tr.workload_rhs("hyperbolic")
    (n_end, ss_end, rs_end), (b_ss, b_rs) = tr.end_truth(g, [*x[2], *v[2]], p, 0.05 * H[2])
    print(f"{solver}: N_end {got.N_end[2]:.6f} (truth {n_end:.6f}), |T_SS_end - truth| {abs(got.T_SS_end[2] - ss_end):.2e} (bound {b_ss:.2e}), "
          f"|T_RS_end - truth| {abs(got.T_RS_end[2] - rs_end):.2e} (bound {b_rs:.2e})")  # fmt: skip
    assert abs(got.T_SS_end[2] - ss_end) <= b_ss and abs(got.T_RS_end[2] - rs_end) <= b_rs
    # theta is cyclic and every lane of a kind starts from the same phi and velocities: the same values bit for bit
    assert np.array_equal(got.T_SS_end[ended], np.full(ended.sum(), got.T_SS_end[2]))


def test_transfer_map_is_its_two_halves(bg, hyper):
    """A 5 x 7 grid over a range that holds points too close to the end of inflation for N_star = 0.5: ``transfer_map`` equals
    ``horizon_exit_map`` followed by ``transfer_functions`` from the exit states with ``samples=[0.0]``, bit for bit, NaN where no
    exit state was found."""
    p, art, _twin = hyper
    ss, d = [[1.8, 4.0], [-1.0, 1.0]], (-0.2, 1e-3)
    (t_rs, t_ss), state, n_end, status = bg.transfer_map(art, p, ss, 5, 7, N_star=0.5, derivatives_init=d, return_status=True)
    short = bg.transfer_map(art, p, ss, 5, 7, N_star=0.5, derivatives_init=d)
    state2, n_end2, status2 = bg.horizon_exit_map(art, p, ss, 5, 7, N_star=0.5, derivatives_init=d, return_status=True)
    assert np.array_equal(state, state2, equal_nan=True) and np.array_equal(n_end, n_end2, equal_nan=True)
    found = status2 == TARGET
    assert 0 < found.sum() < 35 and t_rs.shape == t_ss.shape == status.shape == (5, 7)
    flat = state2[found]
    tf = bg.transfer_functions(art, p, [0.0], flat[:, :2], flat[:, 2:4])
    assert np.all(tf.status == ENDED)
    assert np.array_equal(t_rs[found], tf.T_RS_end) and np.array_equal(t_ss[found], tf.T_SS_end) and np.isfinite(t_rs[found]).all()
    assert np.isnan(t_rs[~found]).all() and np.isnan(t_ss[~found]).all()
    assert np.array_equal(status[found], tf.status) and np.array_equal(status[~found], status2[~found])
    assert np.array_equal(short[0][0], t_rs, equal_nan=True) and np.array_equal(short[0][1], t_ss, equal_nan=True) and len(short) == 3
    # dq_dN per grid point: a constant array is the scalar; a varying one is the hand call with the found points' values
    const = bg.transfer_map(art, p, ss, 5, 7, N_star=0.5, derivatives_init=d, dq_dN=np.full((5, 7), -0.2))
    scalar = bg.transfer_map(art, p, ss, 5, 7, N_star=0.5, derivatives_init=d, dq_dN=-0.2)
    assert all(np.array_equal(u, w, equal_nan=True) for u, w in zip(const[0], scalar[0])) and not np.array_equal(scalar[0][1], t_ss, equal_nan=True)
    grid = np.linspace(-0.5, 0.3, 35).reshape(5, 7)
    varied = bg.transfer_map(art, p, ss, 5, 7, N_star=0.5, derivatives_init=d, dq_dN=grid)
    hand = bg.transfer_functions(art, p, [0.0], flat[:, :2], flat[:, 2:4], dq_dN=grid[found])
    assert np.array_equal(varied[0][0][found], hand.T_RS_end) and np.array_equal(varied[0][1][found], hand.T_SS_end) and np.isnan(varied[0][0][~found]).all()
    # the exit states are about N_star from the end, and the second stage finds about that many e-folds again
    assert np.abs(tf.N_end - 0.5).max() < 0.05 and np.abs(t_rs[found]).max() > 1e-4


def test_transfer_object_of_another_layout_is_refused(bg):
    """An object built with -DINFLX_TR_ABI_VERSION=2 is refused with INFLX_ERR_VERSION, a missing one is INFLX_ERR_SYMBOL with the
    way to build it; the artefact's own build then replaces the refused file and works on the same handle."""
    from background_reference import power_law_artifact, power_law_init
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".transfer"
    headers = {stale + ".model.h": header_text, stale + ".eom.h": art.eom_header_text(), stale + ".kin.h": art.kinematics_header_text(),
               stale + ".mass.h": art.masses_header_text()}  # fmt: skip
    init = np.array([power_law_init()], dtype=np.float64)
    init[0, 3] = 1e-3  # (a direction to measure the entropic perturbation across)
    p = np.ascontiguousarray(p, dtype=np.float64)
    samples = np.array([0.0, 1e-3])
    out, status = np.empty((2, 10, 1)), np.empty(1, dtype=np.int8)
    dp = C.POINTER(C.c_double)

    def raw(lib):  # the C entry point's own return code
        return lib._lib.inflx_transfer_functions(lib._h, p.ctypes.data_as(dp), 1, lib.n_parameters, init.ctypes.data_as(dp), 1, None, samples.ctypes.data_as(dp), 2, 100,
                                                 _native.EOM_RKF, 1e-8, 0.0, 0, out.ctypes.data_as(dp), None, None, status.ctypes.data_as(C.POINTER(C.c_int8)), None)  # fmt: skip

    try:
        if os.path.exists(stale):
            os.remove(stale)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        assert raw(lib) == _native.ERR_SYMBOL
        with pytest.raises(SystemError, match=r"ensure_transfer\(\)") as err:
            lib.transfer_functions(p, init, None, samples, 100, _native.EOM_RKF, 1e-8, 0.0, 0)
        assert ".transfer exists" in str(err.value)
        for path, text in headers.items():
            with open(path, "w") as fh:
                fh.write(text)
        hdr, eom_hdr, kin_hdr, mass_hdr = headers
        cmd = [hipcc_path(), *options, "-DINFLX_TR_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_KIN_HEADER="{kin_hdr}"', f'-DINFLX_MASS_HEADER="{mass_hdr}"',
               os.path.join(_CSRC, "inflx_transfer_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        assert raw(lib) == _native.ERR_VERSION
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.transfer_functions(p, init, None, samples, 100, _native.EOM_RKF, 1e-8, 0.0, 0)
        assert "INFLX_TR_ABI 2, expected 1" in str(err.value)
        os.remove(stale)
        art.ensure_transfer()
        got = lib.transfer_functions(p, init, None, samples, 100, _native.EOM_RKF, 1e-8, 0.0, 0)
        assert got[0].shape == (2, 10, 1) and got[3][0] == TARGET and np.isfinite(got[0]).all()
        lib.close()
    finally:
        for path in (stale, *headers):
            if os.path.exists(path):
                os.remove(path)


def test_plane_against_the_field_basis_system(bg):
    """Truth (a) on the GPU: the 17 Cartesian plane states at the default max_err, within the bound the host build establishes."""
    from inflatox_amd import Compiler

    _pa, ca, _pp, cp, _ps, cs, a, b = tr.plane_case()
    _polar, cart = kr.plane_models()
    art = Compiler(cart, silent=True).compile()
    assert art.symbol_dictionary == ca.symbol_dictionary
    got = bg.transfer_functions(art, cp, tr.PLANE_SAMPLES, cs[:, :2], cs[:, 2:4], dq_dN=tr.PLANE_DQ, stop_at_end=False)
    assert np.all(got.status == TARGET) and np.all(got.T_SS[:, 0] == 1.0) and np.all(got.T_RS[:, 0] == 0.0)
    err, bound = tr.plane_error(got, cs, a, b), tr.plane_bound("rkf", 1e-8)
    print(f"plane: worst |GPU - truth (a)| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_more_than_one_pass_lands_behind_the_first_in_every_plane(bg, hyper):
    """S = 64 samples are 64 x 10 doubles per lane, so the 256 MiB sample buffer holds floor(2^28 / 5120) = 52 428 lanes, whole
    workgroups of 256: 52 224.  B = 52 224 + 5 takes two passes, five fixed steps of dt = 1e-3 each, and the second one's five lanes
    land behind the first one's in every plane of the result: the first five lanes, the lanes on either side of the seam and the
    last five are the same lanes run alone, bit for bit and NaN where NaN.  The first sample is N = 0, which every lane stores."""
    p, art, _twin = hyper
    first, B = 52_224, 52_224 + 5
    x, v = tr.hyper_states(B, seed=4)
    samples = np.linspace(0.0, 3e-3, 64)
    kw = dict(max_steps=5, solver="rkf", dt=1e-3, stop_at_end=False)
    big = bg.transfer_functions(art, p, samples, x, v, **kw)
    assert big.T_SS.shape == (B, 64) and np.all(big.n_stored >= 1) and np.all(big.T_SS[:, 0] == 1.0) and np.isfinite(big.states[:, 0]).all()
    print(f"n_stored {big.n_stored.min()} .. {big.n_stored.max()}, statuses {np.bincount(big.status)}")
    assert big.n_stored.max() > 1 and np.isfinite(big.T_RS[first - 2 : first + 2, 1]).all()
    for sl in (slice(0, 5), slice(first - 2, first + 2), slice(B - 5, B)):
        assert _same(big, bg.transfer_functions(art, p, samples, x[sl], v[sl], **kw), sl), sl
