"""A target on N on the GPU (inflatox_amd.background.state_at_efolds, horizon_exit_map): the analytic power-law attractor, lane
independence with per-lane targets, the host build of the same stepper, the horizon-exit map against efolds_map and scipy's DOP853,
and the refusal of a background object of the previous layout."""

import math
import os
import subprocess

import numpy as np
import pytest

import workloads
from background_reference import COMPLETE, ENDED, model_functions, power_law_artifact, power_law_exact, power_law_init, solve_ivp_reference
from background_target_reference import TARGET, TargetTwin
from test_background_gpu import RESTATEMENT_TOL, _hyper_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def power_law():
    return power_law_artifact()


def _power_law_error(got, n_target):
    """error of (state, N, t) against the attractor at N = n_target, relative with a floor of 1"""
    t_exact = math.exp(n_target / 8.0) - 1.0  # N = p ln(1 + t), p = 8
    exact = np.append(power_law_exact(t_exact), t_exact)
    return float(np.max(np.abs(got - exact) / np.maximum(np.abs(exact), 1.0)))


def _rows(res):
    """(B, 7): state, N, t"""
    return np.concatenate([res.state, res.N[:, None], res.t[:, None]], axis=1)


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_located_state_is_fourth_order(bg, power_law, method):
    """Fixed dt = 2/n: halving dt cuts the error of the located state by >= 14 (fourth order: 16)."""
    art, p = power_law
    x0 = power_law_init()
    targets = np.array([0.37, 2.0])
    X, V = np.tile(x0[:2], (2, 1)), np.tile(x0[2:], (2, 1))
    errs = []
    for n in (40, 80):
        res = bg.state_at_efolds(art, p, X, V, targets, max_steps=10_000, solver=method, dt=2.0 / n, stop_at_end=False)
        assert np.all(res.status == TARGET) and np.array_equal(res.N, targets)
        errs.append([_power_law_error(row, nt) for row, nt in zip(_rows(res), targets)])
    ratios = np.array(errs[0]) / np.array(errs[1])
    print(f"{method}: errors {errs}, ratios {ratios}")
    assert np.all(ratios >= 14.0), (errs, ratios)


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_adaptive_located_state_on_the_power_law(bg, power_law, method):
    """Three targets in one call; N_t = 8 takes 635 accepted steps with rk4, so that lane crosses two launch boundaries."""
    art, p = power_law
    x0 = power_law_init()
    targets = np.array([0.37, 2.0, 8.0])
    res = bg.state_at_efolds(art, p, np.tile(x0[:2], (3, 1)), np.tile(x0[2:], (3, 1)), targets, max_err=1e-10, solver=method)
    assert np.all(res.status == TARGET) and np.array_equal(res.N, targets) and np.all(np.isnan(res.N_end))
    errs = [_power_law_error(row, nt) for row, nt in zip(_rows(res), targets)]
    print(f"{method}: errors {errs}")
    assert max(errs) <= 1e-8, errs
    assert np.max(np.abs(res.eps_H - 1.0 / 8.0)) <= 1e-8  # epsilon_H of the attractor is 1/p


@pytest.fixture(scope="module")
def hyper_lanes():
    x, v = _hyper_batch(300)
    targets = np.random.default_rng(11).uniform(0.0, 1.5, 300)
    return x, v, targets


FIELDS = ("state", "t", "N", "eps_H", "N_end", "status")


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_lane_independence(bg, hyper_lanes, solver):
    spec, art = workloads.artifact_for("hyperbolic")
    x, v, targets = hyper_lanes
    full = bg.state_at_efolds(art, spec.args, x, v, targets, solver=solver)
    assert (full.status == TARGET).any() and (full.status == ENDED).any(), np.bincount(full.status)
    hit = full.status == TARGET
    assert np.isfinite(full.state[hit]).all() and np.isnan(full.state[~hit]).all() and np.isnan(full.eps_H[~hit]).all()
    assert np.array_equal(full.N[hit], targets[hit])
    ended = full.status == ENDED
    assert np.isfinite(full.N_end[ended]).all() and np.all(full.N_end[ended] < targets[ended]) and np.isnan(full.N_end[~ended]).all()
    perm = np.random.default_rng(1).permutation(300)
    shuffled = bg.state_at_efolds(art, spec.args, x[perm], v[perm], targets[perm], solver=solver)
    part = bg.state_at_efolds(art, spec.args, x[:63], v[:63], targets[:63], solver=solver)
    for f in FIELDS:
        assert np.array_equal(getattr(full, f)[perm], getattr(shuffled, f), equal_nan=True), f
        assert np.array_equal(getattr(full, f)[:63], getattr(part, f), equal_nan=True), f


def test_edge_cases(bg):
    spec, art = workloads.artifact_for("hyperbolic")
    x, v = np.array([[3.0, 0.5]] * 4), np.array([[0.0, 0.1]] * 4)
    res = bg.state_at_efolds(art, spec.args, x, v, [0.0, -2.0, 1e3, 0.5])
    assert list(res.status) == [TARGET, TARGET, ENDED, TARGET]
    first = bg.solve_eom_batch(art, spec.args, 1, x[:1], v[:1])
    for k in (0, 1):  # a target <= 0: the initial state, t = 0
        assert np.array_equal(res.state[k], first.states[0, 0]) and res.t[k] == 0.0 and res.N[k] == 0.0 and np.isfinite(res.eps_H[k])
    assert np.isnan(res.state[2]).all() and np.isnan(res.t[2]) and np.isfinite(res.N_end[2])
    nend = bg.solve_eom_batch(art, spec.args, 2, x[:1], v[:1], max_err=1e-8, stop_at_end=True, substeps=100_000).N_end[0]
    assert res.N_end[2] == nend
    # max_steps run out first: 300 fixed steps (two launches, 256 + 44) reach t = 0.3, long before the end of inflation
    short = bg.state_at_efolds(art, spec.args, x, v, 1e3, max_steps=300, solver="rk4", dt=1e-3)
    assert np.all(short.status == COMPLETE) and np.isnan(short.state).all() and np.isnan(short.N_end).all()


def test_agrees_with_the_host_stepper(bg, hyper_lanes):
    """Fixed dt = 1e-3, rk4: the kernel against the host build of the same stepper (tests/background_target_twin.cpp), which differ
    by FMA contraction only -- the bound test_background_gpu.py sets for the same kind of comparison."""
    spec, art = workloads.artifact_for("hyperbolic")
    twin = TargetTwin(art)
    x, v, targets = (a[:8] for a in hyper_lanes)
    res = bg.state_at_efolds(art, spec.args, x, v, targets, solver="rk4", dt=1e-3)
    got = np.concatenate([_rows(res), res.eps_H[:, None]], axis=1)
    assert (res.status == TARGET).sum() >= 4, res.status
    worst = 0.0
    for k in range(8):
        want, meta = twin.solve(spec.args, np.concatenate([x[k], v[k]]), targets[k], 100_000, "rk4", dt=1e-3, stop_at_end=True)
        assert res.status[k] == meta["status"]
        if meta["status"] == TARGET:
            worst = max(worst, float(np.max(np.abs(got[k] - want) / np.maximum(np.abs(want), 1e-3))))
        else:
            assert meta["status"] == ENDED and abs(res.N_end[k] - meta["N_end"]) <= RESTATEMENT_TOL["hyperbolic"] * max(meta["N_end"], 1e-3)
    print(f"fixed-dt GPU vs host stepper, max relative difference {worst:.3e}")
    assert worst <= RESTATEMENT_TOL["hyperbolic"], worst


MAP = dict(start_stop=np.array([[1.0, 5.0], [-1.0, 1.0]]), N0=24, N1=8)
# agreement of the exit state with DOP853 at the four points below, relative with a floor of 1.  It cannot be better than the
# error of N_end (linear in epsilon_H across the last step, test_background_gpu.py: <= 6e-4 e-folds at 1e-8) times |dphi/dN|.
# Measured with the host build of the stepper, which differs from the kernel by FMA rounding only (~1e-12,
# test_agrees_with_the_host_stepper), at max_err = 1e-9 (N_end 2.1e-4 .. 2.4e-4 e-folds off): 4.7e-4, 6.9e-5, 6.3e-5, 7.5e-5 -- the first point exits 0.02
# e-folds after the start, where the field still accelerates from rest and chi^0 takes the error; the bound is twice the worst
EXIT_TOL = 9.5e-4
EXIT_POINTS = ((11, 0), (15, 3), (19, 5), (23, 7))  # N_end = 1.02, 1.83, 2.86, 4.09


def test_horizon_exit_map(bg):
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    kw = dict(max_steps=20_000, max_err=1e-9)
    state, n_end, status = bg.horizon_exit_map(art, p, MAP["start_stop"], MAP["N0"], MAP["N1"], N_star=1.0, return_status=True, **kw)
    want_end, want_status = bg.efolds_map(art, p, MAP["start_stop"], MAP["N0"], MAP["N1"], return_status=True, **kw)
    assert state.shape == (24, 8, 5) and status.dtype == np.int8
    assert np.array_equal(n_end, want_end, equal_nan=True)
    with np.errstate(invalid="ignore"):
        long_enough = n_end >= 1.0
    assert np.array_equal(np.isfinite(state).all(axis=2), long_enough) and np.array_equal(np.isnan(state).all(axis=2), ~long_enough)
    assert np.array_equal(status == TARGET, long_enough)
    short = np.isfinite(n_end) & ~long_enough
    assert np.array_equal(status == bg.ENDED_SHORT, short) and np.array_equal(status[np.isnan(n_end)], want_status[np.isnan(n_end)])
    # both kinds of NaN points: row 0 (phi = phi0, the minimum of V: H = 0) never ends, and some rows end short
    assert np.isnan(n_end[0]).all() and not np.isin(status[0], (ENDED, TARGET, bg.ENDED_SHORT)).any() and short.any() and long_enough.any()
    pair = bg.horizon_exit_map(art, p, MAP["start_stop"], MAP["N0"], MAP["N1"], N_star=1.0, **kw)
    assert len(pair) == 2 and np.array_equal(pair[0], state, equal_nan=True) and np.array_equal(pair[1], n_end, equal_nan=True)
    # N_star = 0: the state at the end of inflation itself, wherever inflation ends
    state0, n_end0, status0 = bg.horizon_exit_map(art, p, MAP["start_stop"], MAP["N0"], MAP["N1"], N_star=0.0, return_status=True, **kw)
    assert np.array_equal(status0 == TARGET, np.isfinite(n_end)) and not (status0 == bg.ENDED_SHORT).any()

    from scipy.optimize import brentq

    eom = model_functions(workloads.model_for("hyperbolic"), art.symbol_dictionary)
    x0, x1 = bg.grid_points(MAP["start_stop"], MAP["N0"], MAP["N1"])
    diffs = []
    for i, j in EXIT_POINTS:
        assert long_enough[i, j], (i, j, n_end[i, j])
        ref = solve_ivp_reference(eom, p, [x0[i], x1[j], 0.0, 0.0], 1e4, end_event=True)
        n_exit = ref.y_events[0][0][5] - 1.0
        t_exit = brentq(lambda t: ref.sol(t)[5] - n_exit, 0.0, ref.t_events[0][0], xtol=1e-14, rtol=1e-14)
        want = ref.sol(t_exit)[:5]
        diffs.append(float(np.max(np.abs(state[i, j] - want) / np.maximum(np.abs(want), 1.0))))
    print(f"horizon exit vs DOP853 at {EXIT_POINTS}: {diffs}")
    assert max(diffs) <= EXIT_TOL, diffs


def test_stale_background_object_is_refused():
    """A background object of the previous layout version (INFLX_BG_ABI = 2: no target kernels, twelve carry planes) is refused."""
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".background"
    hdr, eom_hdr = stale + ".model.h", stale + ".eom.h"
    try:
        for path, text in ((hdr, header_text), (eom_hdr, art.eom_header_text())):
            with open(path, "w") as fh:
                fh.write(text)
        cmd = [hipcc_path(), *options, "-DINFLX_BG_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', os.path.join(_CSRC, "inflx_background_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        init = np.array([power_law_init()])
        with pytest.raises(SystemError, match="does not belong"):
            lib.solve_eom(p, init, 10, 1, _native.EOM_RKF, 1e-6, 0.0, 0)
        with pytest.raises(SystemError, match="does not belong"):
            lib.solve_eom_to_efolds(p, init, np.array([0.5]), 100, _native.EOM_RKF, 1e-6, 0.0, 0)
        lib.close()
    finally:
        for path in (stale, hdr, eom_hdr):
            if os.path.exists(path):
                os.remove(path)


def test_more_than_one_pass_lands_behind_the_first(bg):
    """B = 2^20 + 3 -- a pass holds at most 2^20 lanes --, three fixed steps of dt = 0.01 from inflating states of the hyperbolic
    model: two lanes in three have a target of 0.004 e-folds, which they reach (TARGET), the third one of 1, which it does not
    (COMPLETE, NaN).  The first five lanes, the lanes on either side of the seam and the last five are the same lanes run alone,
    bit for bit and NaN where NaN, in every member; lanes on both sides of the seam hold a located state."""
    from transfer_reference import hyper_states

    spec, art = workloads.artifact_for("hyperbolic")
    first, B = 1 << 20, (1 << 20) + 3
    x, v = hyper_states(B, seed=12)
    targets = np.where(np.arange(B) % 3 == 2, 1.0, 0.004)
    kw = dict(max_steps=3, solver="rkf", dt=0.01)
    big = bg.state_at_efolds(art, spec.args, x, v, targets, **kw)
    assert np.array_equal(big.status, np.where(targets == 1.0, COMPLETE, TARGET)), np.bincount(big.status)
    assert np.isfinite(big.state[big.status == TARGET]).all() and np.isnan(big.state[big.status == COMPLETE]).all()
    assert np.isfinite(big.state[first - 3 : first]).any() and np.isfinite(big.state[first:]).any()
    for sl in (slice(0, 5), slice(first - 3, first + 3), slice(B - 5, B)):
        small = bg.state_at_efolds(art, spec.args, x[sl], v[sl], targets[sl], **kw)
        for f in FIELDS:
            assert np.array_equal(getattr(big, f)[sl], getattr(small, f), equal_nan=True), (sl, f)
