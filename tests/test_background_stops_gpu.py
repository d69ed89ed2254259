"""The stop statuses REJECTED, UNDERFLOW and mid-run NONFINITE of the background kernels, and the pending plane carried across a
launch, on the GPU.  The lanes, and the reasons why their statuses hold whatever the rounding, are in tests/test_background_stops.py,
which checks them on the host builds; here the kernels (rows, final-only, target, sampled, the row transpose, and the transfer and
mode kernels that borrow inflx_bg_step_taken) must reach the same statuses, write the same last_row, leave NaN after a stop, and
leave the other lanes of the batch alone.

Every call that holds a lane on the wall runs WITHOUT stop_at_end: at phi = 0, phidot = -1 the model has epsilon_H = 1 - 2e-16, one
rounding away from a lane that ENDED in its init, and the statuses under test are not about that."""

import numpy as np
import pytest

import workloads
from background_reference import COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW, BackgroundTwin
from background_sampled_reference import SampledTwin
from background_target_reference import TARGET, TargetTwin
from test_background_gpu import RESTATEMENT_TOL
from test_background_stops import (
    ACCEPTED_THEN_NAN,
    ACCEPTED_THEN_NAN_DT,
    AWAY,
    BORROWED_AWAY,
    BORROWED_N_EXIT,
    BORROWED_REJECTED,
    BORROWED_SAMPLES,
    CLAMPED_ROWS,
    MAX_ERR,
    MAX_STEPS,
    METHODS,
    PENDING_DT,
    PENDING_FINE_ROWS,
    PENDING_ROWS,
    PENDING_SUBSTEPS,
    SAMPLES,
    TARGET_N,
    TOWARD,
    TOWARD_FIXED,
    WALL_START,
    pending_inits,
    wall,
    wall_twin,
)

pytestmark = pytest.mark.gpu

B = 257
TOL = RESTATEMENT_TOL["hyperbolic"]
WALL, TO, AWAY_K, NAN = range(4)  # the lane kinds, k % 4
NAN_INPUT = (np.nan, 0.0, -1.0, 0.0)
FIXED_DT = 1e-4
# the four calls of the batch: options, and the status of every lane kind
CALLS = {
    "adaptive": (dict(steps=80, max_err=MAX_ERR), (REJECTED, UNDERFLOW, COMPLETE, NONFINITE)),
    "adaptive-7": (dict(steps=12, max_err=MAX_ERR, substeps=7), (REJECTED, UNDERFLOW, COMPLETE, NONFINITE)),
    "fixed": (dict(steps=30, dt=FIXED_DT), (NONFINITE, NONFINITE, COMPLETE, NONFINITE)),
    "fixed-3": (dict(steps=12, dt=FIXED_DT, substeps=3), (NONFINITE, NONFINITE, COMPLETE, NONFINITE)),
}


def batch(fixed, n=B):
    """(n, 4): wall at the start, toward the wall, away from it, a NaN input, in turn"""
    kinds = np.array([WALL_START, TOWARD_FIXED if fixed else TOWARD, AWAY, NAN_INPUT])
    return kinds[np.arange(n) % 4]


def planes(sol):
    """(B, rows, 7): y[0..5], t -- the host twin's rows"""
    return np.concatenate([sol.states, sol.N[:, :, None], sol.t[:, :, None]], axis=2)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def same_solution(a, b, sl=slice(None)):
    return all(same(np.asarray(getattr(a, f))[sl], np.asarray(getattr(b, f))) for f in ("states", "t", "N", "status", "last_row", "N_end"))


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def wall_case():
    """the wall artefact, its parameter row and the host build without contraction"""
    art, p = wall()
    return art, p, wall_twin()


@pytest.fixture(scope="module")
def hyper_case():
    spec, art = workloads.artifact_for("hyperbolic")
    return art, spec.args, BackgroundTwin(art)


@pytest.fixture(scope="module")
def batches(bg, wall_case):
    """solve_eom_batch of the B = 257 batch, every (call, solver) once"""
    art, p, _ = wall_case
    done = {}

    def get(call, method):
        if (call, method) not in done:
            options, _ = CALLS[call]
            init = batch("dt" in options)
            done[call, method] = bg.solve_eom_batch(art, p, fields_init=init[:, :2], derivatives_init=init[:, 2:], solver=method, **options)
        return done[call, method]

    return get


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("call", CALLS)
def test_one_batch_of_every_kind(bg, wall_case, batches, call, method):
    """257 lanes of four kinds in one call: every kind reaches its status; the kinds whose steps do not depend on rounding -- on the
    wall at the start, a fixed step toward the wall, away from it -- match the host build in last_row, in the NaN pattern and in
    every stored row within 1e-12 (the two host builds differ by 1.1e-16); every lane equals, bit for bit, every other lane of its
    kind, a B = 1 call on it alone, and -- the "away" lanes, which share their wavefronts with three stopped ones -- a call that
    holds nothing but "away" lanes.

    The adaptive "away" lane is compared with the host build on its first ``CLAMPED_ROWS`` rows, where the controller's factor is
    clamped at 5.  After those its dt follows an error estimate that is rounding noise to ~1e-7 relative, and the two HOST builds
    already differ by 2.7e-8 over the 80 rows (test_background_stops.py::test_away_lane_of_the_long_adaptive_calls): last_row, the
    NaN pattern and the status are asserted on all rows, the difference of the later rows is printed."""
    art, p, twin = wall_case
    options, statuses = CALLS[call]
    fixed = "dt" in options
    steps, substeps = options["steps"], options.get("substeps", 1)
    twin_options = {k: v for k, v in options.items() if k != "steps"}
    init = batch(fixed)
    sol = batches(call, method)
    got = planes(sol)
    kind = np.arange(B) % 4
    for k in range(4):
        assert np.all(sol.status[kind == k] == statuses[k]), (k, sol.status[kind == k])
    assert np.isnan(sol.N_end).all()
    for b in range(B):  # rows up to last_row hold states, the rows after it NaN and nothing else
        assert np.isnan(got[b, sol.last_row[b] + 1 :]).all()
        assert np.isfinite(got[b, : sol.last_row[b] + 1]).all() or kind[b] == NAN
    assert np.all(sol.last_row[kind == NAN] == 0) and np.all(sol.last_row[kind == WALL] == 0) and np.all(sol.last_row[kind == AWAY_K] == steps - 1)
    # against the host build
    deterministic = [(WALL, steps), (AWAY_K, steps if fixed else (CLAMPED_ROWS - 1) // substeps + 1)] + ([(TO, steps)] if fixed else [])
    for k, compared in deterministic:
        want, meta = twin.solve(p, init[k], steps, method, **twin_options)
        assert meta["status"] == statuses[k] and sol.last_row[k] == meta["last_row"]
        assert np.array_equal(np.isnan(got[k]), np.isnan(want))
        rel = np.abs(got[k] - want) / np.maximum(np.abs(want), 1e-3)
        worst = np.nanmax(rel[:compared])
        print(f"{call} {method} kind {k}: last_row {sol.last_row[k]}, device against host build, max relative difference {worst:.3e} over {compared} rows (bound {TOL:g})")
        assert worst <= TOL, (k, worst)
        if compared < steps:
            print(f"{call} {method} kind {k}: rows {compared} .. {steps - 1}, where dt follows the error estimate: {np.nanmax(rel[compared:]):.3e}")
    if fixed:  # the lane that steps into the wall: ten steps, then a stage at phi < 0 -- the row that step falls in is NaN
        assert np.all(sol.last_row[kind == TO] == 10 // substeps)
    # every lane of a kind is the same lane
    for k in range(4):
        for f in ("states", "t", "N", "last_row"):
            v = getattr(sol, f)[kind == k]
            assert same(v, np.broadcast_to(v[:1], v.shape)), (k, f)
    # alone
    for k in range(4):
        one = bg.solve_eom_batch(art, p, fields_init=init[k : k + 1, :2], derivatives_init=init[k : k + 1, 2:], solver=method, **options)
        assert same_solution(sol, one, slice(k, k + 1)), k
    # a stopped lane does not disturb its wavefront
    away = np.flatnonzero(kind == AWAY_K)
    alone = bg.solve_eom_batch(art, p, fields_init=init[away, :2], derivatives_init=init[away, 2:], solver=method, **options)
    assert same_solution(sol, alone, away)


@pytest.mark.parametrize("method", METHODS)
def test_adaptive_underflow_lanes(wall_case, batches, method):
    """The lanes that creep up to the wall until t + dt == t.  How many steps that takes depends on rounding (the host builds: 70
    against 68 with rk4), so the count is printed, not asserted.  Asserted: the status; rows 1 .. last_row are finite with phi
    strictly decreasing and positive and t strictly increasing; every later row is NaN; the call with 7 substeps holds every 7th row
    of the other bit for bit and its last_row is last_row // 7 -- the row the lane stopped in is not counted and not written --;
    the last stored t is the time at which the trajectory meets the wall, 1.001043e-3 on both host builds, with its fourth digit
    left open, and the last stored phi lies in (0, 1e-15)."""
    art, p, twin = wall_case
    one, seven = batches("adaptive", method), batches("adaptive-7", method)
    _, meta = twin.solve(p, TOWARD, 80, method, max_err=MAX_ERR)
    lanes = np.flatnonzero(np.arange(B) % 4 == TO)
    assert np.all(one.status[lanes] == UNDERFLOW) and np.all(seven.status[lanes] == UNDERFLOW)
    b = lanes[0]
    last1, last7 = int(one.last_row[b]), int(seven.last_row[b])
    print(f"{method}: UNDERFLOW after {last1} accepted steps on the device, {meta['accepted']} on the host build")
    assert 0 < last1 < 79 and last7 == last1 // 7
    g1, g7 = planes(one)[b], planes(seven)[b]
    for g, last in ((g1, last1), (g7, last7)):
        assert np.isfinite(g[: last + 1]).all() and np.isnan(g[last + 1 :]).all()
        assert np.all(np.diff(g[: last + 1, 0]) < 0) and np.all(g[: last + 1, 0] > 0) and np.all(np.diff(g[: last + 1, 6]) > 0)
    assert np.array_equal(g7[: last7 + 1], g1[: 7 * last7 + 1 : 7])
    assert 1.0010e-3 <= g1[last1, 6] <= 1.0011e-3, g1[last1, 6]
    assert 0.0 < g1[last1, 0] < 1e-15, g1[last1, 0]


def test_accepted_state_exit(bg, wall_case):
    """rk4, dt = 0.02: the lane whose first step has every stage in front of the wall and its end behind it (test_background_stops.py)
    among "away" lanes.  The rows kernel stops it NONFINITE with last_row 0 and NaN rows, as the host build does.  The final-only
    kernel shows which exit was taken: the state it leaves is the accepted one, finite, with phi in (-5.9e-7, 0) and t = dt -- a
    trial that failed would have left the initial state and t = 0.  The "away" lanes equal a call without the stopped ones."""
    from inflatox_amd import _native

    art, p, twin = wall_case
    n = 129
    init = np.tile(np.array(AWAY), (n, 1))
    stopped = np.arange(n) % 2 == 0
    init[stopped] = ACCEPTED_THEN_NAN
    sol = bg.solve_eom_batch(art, p, 4, init[:, :2], init[:, 2:], solver="rk4", dt=ACCEPTED_THEN_NAN_DT)
    assert np.all(sol.status[stopped] == NONFINITE) and np.all(sol.last_row[stopped] == 0) and np.all(sol.status[~stopped] == COMPLETE)
    got = planes(sol)
    assert np.isnan(got[stopped, 1:]).all() and np.isfinite(got[stopped, 0]).all() and np.isfinite(got[~stopped]).all()
    for k in (0, 1):
        want, meta = twin.solve(p, init[k], 4, "rk4", dt=ACCEPTED_THEN_NAN_DT)
        assert meta["status"] == sol.status[k] and meta["last_row"] == sol.last_row[k] and np.array_equal(np.isnan(got[k]), np.isnan(want))
        assert np.nanmax(np.abs(got[k] - want) / np.maximum(np.abs(want), 1e-3)) <= TOL
        assert same(got[k::2], np.broadcast_to(got[k], got[k::2].shape))
    alone = bg.solve_eom_batch(art, p, 4, init[~stopped, :2], init[~stopped, 2:], solver="rk4", dt=ACCEPTED_THEN_NAN_DT)
    assert same_solution(sol, alone, ~stopped)
    states, t, _, status, last_row = bg._dylib(art).solve_eom(p, init, 4, 1, _native.EOM_RK4, MAX_ERR, ACCEPTED_THEN_NAN_DT, _native.EOM_FINAL_ONLY)
    assert np.array_equal(status, sol.status) and np.array_equal(last_row, sol.last_row)
    assert np.isfinite(states[stopped]).all() and np.all(states[stopped, 0] < 0.0) and np.all(states[stopped, 0] > -5.9e-7), states[0]
    assert np.all(t[stopped] == ACCEPTED_THEN_NAN_DT)
    assert np.array_equal(states[~stopped], got[~stopped, 3, :6]) and np.array_equal(t[~stopped], got[~stopped, 3, 6])


@pytest.mark.parametrize("method", METHODS)
def test_pending_row_across_launches(bg, hyper_case, method):
    """65 lanes that end (stop_at_end, dt = 1e-3) at accepted steps in (512, 768), with 300 substeps: inside row 3 and inside the
    third launch of 256 steps, while row 3 is complete at step 899, in the fourth.  The end state has to be carried to that launch
    and written there: for every lane the coarse row ceil(r / 300) is the fine row r of a call with one substep, bit for bit, N_end,
    status and last_row == ceil(r / 300) agree, the rows before are every 300th fine row and the rows after are NaN.  The
    device-resident call (the transpose kernel) and the final-only kernel, reached as efolds_map reaches it, give the same."""
    from inflatox_amd import _native

    art, p, twin = hyper_case
    init = pending_inits()
    n = init.shape[0]
    ends = np.array([twin.solve(p, lane, PENDING_FINE_ROWS, method, dt=PENDING_DT, stop_at_end=True)[1]["last_row"] for lane in init])
    assert np.all((ends > 512) & (ends < 768) & (ends % PENDING_SUBSTEPS != 0)), ends  # (a condition on the inputs)
    x, v = init[:, :2], init[:, 2:]
    fine = bg.solve_eom_batch(art, p, PENDING_FINE_ROWS, x, v, solver=method, dt=PENDING_DT, stop_at_end=True)
    coarse = bg.solve_eom_batch(art, p, PENDING_ROWS, x, v, solver=method, dt=PENDING_DT, substeps=PENDING_SUBSTEPS, stop_at_end=True)
    print(f"{method}: end steps on the device {fine.last_row.tolist()}")
    assert np.all(fine.status == ENDED) and np.all(coarse.status == ENDED)
    assert np.array_equal(fine.last_row, ends)
    gf, gc = planes(fine), planes(coarse)
    for b in range(n):
        r = int(fine.last_row[b])
        row = -(-r // PENDING_SUBSTEPS)
        assert coarse.last_row[b] == row == 3
        assert np.array_equal(gc[b, row], gf[b, r]) and np.isfinite(gc[b, row]).all()
        assert np.array_equal(gc[b, :row], gf[b, 0:r:PENDING_SUBSTEPS])
        assert np.isnan(gc[b, row + 1 :]).all() and np.isnan(gf[b, r + 1 :]).all()
    assert np.array_equal(coarse.N_end, fine.N_end) and np.isfinite(coarse.N_end).all()
    dev = bg.solve_eom_batch_device(art, p, PENDING_ROWS, x, v, solver=method, dt=PENDING_DT, substeps=PENDING_SUBSTEPS, stop_at_end=True)
    assert same(dev.states.cpu().numpy(), coarse.states) and same(dev.t.cpu().numpy(), coarse.t) and same(dev.N.cpu().numpy(), coarse.N)
    assert np.array_equal(dev.status, coarse.status) and np.array_equal(dev.last_row, coarse.last_row) and np.array_equal(dev.N_end, coarse.N_end)
    lib = bg._dylib(art)
    flags = _native.EOM_STOP_AT_END | _native.EOM_FINAL_ONLY
    states, t, n_end, status, last_row = lib.solve_eom(p, init, PENDING_ROWS, PENDING_SUBSTEPS, bg._METHODS[method], 1e-6, PENDING_DT, flags)
    assert np.array_equal(n_end, coarse.N_end) and np.array_equal(status, coarse.status) and np.array_equal(last_row, coarse.last_row)
    assert np.array_equal(states, gc[np.arange(n), 3, :6]) and np.array_equal(t, gc[np.arange(n), 3, 6])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("fixed", [False, True], ids=["adaptive", "fixed"])
def test_final_only_kernel_stops_like_the_rows_kernel(bg, wall_case, method, fixed):
    """The final-only kernel (the _native flag efolds_map uses) on the four lane kinds, 2000 steps, eight launches: status, last_row
    and the state it leaves are those of the rows kernel bit for bit -- the state of row last_row --, the statuses of the stopping
    kinds are the rows kernel's, and the "away" lanes equal a call without the others.  (The adaptive "away" lane comes back to the
    wall within 2000 steps; what it does there is compared between the two kernels, not with a constant.)"""
    from inflatox_amd import _native

    art, p, twin = wall_case
    init = batch(fixed)
    kind = np.arange(B) % 4
    dt = FIXED_DT if fixed else 0.0
    lib = bg._dylib(art)
    states, t, n_end, status, last_row = lib.solve_eom(p, init, MAX_STEPS + 1, 1, bg._METHODS[method], MAX_ERR, dt, _native.EOM_FINAL_ONLY)
    want = (NONFINITE, NONFINITE, COMPLETE, NONFINITE) if fixed else (REJECTED, UNDERFLOW, None, NONFINITE)
    for k in range(4):
        assert want[k] is None or np.all(status[kind == k] == want[k]), (k, status[kind == k])
    assert np.all(last_row[kind == WALL] == 0) and np.all(last_row[kind == NAN] == 0) and np.isnan(n_end).all()
    if fixed:
        assert np.all(last_row[kind == TO] == 10) and np.all(last_row[kind == AWAY_K] == MAX_STEPS)
        ref, meta = twin.solve(p, AWAY, MAX_STEPS + 1, method, dt=FIXED_DT)
        rel = np.abs(np.append(states[AWAY_K], t[AWAY_K]) - ref[-1]) / np.maximum(np.abs(ref[-1]), 1e-3)
        print(f"{method}: final-only, fixed dt, away lane after {MAX_STEPS} steps against the host build: {rel.max():.3e}")
        assert meta["status"] == COMPLETE and rel.max() <= TOL
    rows = bg.solve_eom_batch(art, p, MAX_STEPS + 1, init[:, :2], init[:, 2:], MAX_ERR, method, dt=dt or None)
    assert np.array_equal(status, rows.status) and np.array_equal(last_row, rows.last_row)
    g = planes(rows)[np.arange(B), rows.last_row]
    assert same(states, g[:, :6]) and same(t, g[:, 6])
    away = np.flatnonzero(kind == AWAY_K)
    a_states, a_t, _, a_status, a_last = lib.solve_eom(p, init[away], MAX_STEPS + 1, 1, bg._METHODS[method], MAX_ERR, dt, _native.EOM_FINAL_ONLY)
    assert np.array_equal(a_states, states[away]) and np.array_equal(a_t, t[away]) and np.array_equal(a_status, status[away]) and np.array_equal(a_last, last_row[away])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("fixed", [False, True], ids=["adaptive", "fixed"])
def test_target_kernel_stops(bg, wall_case, method, fixed):
    """state_at_efolds with the target N = 1e-3 on the four lane kinds: REJECTED / UNDERFLOW / TARGET / NONFINITE (adaptive),
    NONFINITE / NONFINITE / TARGET / NONFINITE (fixed), the host build's statuses; a lane that stopped has NaN in every output;
    the "away" lanes equal a call without the others and the located state is the host build's within 1e-12.  With a fixed dt half
    of the "away" lanes get a target they do not reach in 2000 steps: the call then runs eight launches, seven of them after every
    other lane has stopped, and the stopped lanes must come out as from a B = 1 call, which makes one launch."""
    art, p, _ = wall_case
    init = batch(fixed)
    kind = np.arange(B) % 4
    options = dict(max_steps=MAX_STEPS, max_err=MAX_ERR, solver=method, dt=FIXED_DT if fixed else None, stop_at_end=False)
    twin_options = dict(max_err=MAX_ERR, dt=FIXED_DT if fixed else None)
    target = np.full(B, TARGET_N)
    far = np.arange(B) % 8 == AWAY_K + 4 if fixed else np.zeros(B, dtype=bool)
    target[far] = 1.0
    sol = bg.state_at_efolds(art, p, init[:, :2], init[:, 2:], target, **options)
    outputs = np.concatenate([sol.state, sol.t[:, None], sol.N[:, None], sol.eps_H[:, None]], axis=1)
    ttwin = TargetTwin(art)
    for k in range(4):
        want, meta = ttwin.solve(p, init[k], TARGET_N, MAX_STEPS, method, **twin_options)
        lanes = (kind == k) & ~far
        assert np.all(sol.status[lanes] == meta["status"]), (k, sol.status[lanes], meta["status"])
        assert same(outputs[lanes], np.broadcast_to(outputs[k], outputs[lanes].shape))
        if meta["status"] == TARGET:
            got = np.concatenate([sol.state[k], [sol.N[k], sol.t[k], sol.eps_H[k]]])
            rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-3)
            print(f"{method} {'fixed' if fixed else 'adaptive'}: located state against the host build, {meta['accepted']} steps: {rel.max():.3e}")
            assert k == AWAY_K and np.isfinite(got).all() and sol.N[k] == TARGET_N
            assert rel.max() <= TOL or not fixed  # (adaptive: the last steps follow the error estimate, see test_one_batch_of_every_kind)
        else:
            assert np.isnan(outputs[lanes]).all()
    want = (NONFINITE, NONFINITE, TARGET, NONFINITE) if fixed else (REJECTED, UNDERFLOW, TARGET, NONFINITE)
    assert all(np.all(sol.status[(kind == k) & ~far] == want[k]) for k in range(4))
    assert np.all(sol.status[far] == COMPLETE) and np.isnan(outputs[far]).all() and np.isnan(sol.N_end).all()
    for k in range(4):
        one = bg.state_at_efolds(art, p, init[k : k + 1, :2], init[k : k + 1, 2:], TARGET_N, **options)
        assert all(same(np.asarray(a)[k : k + 1], b) for a, b in zip(sol, one)), k
    away = np.flatnonzero(kind == AWAY_K)
    alone = bg.state_at_efolds(art, p, init[away, :2], init[away, 2:], target[away], **options)
    assert all(same(np.asarray(a)[away], b) for a, b in zip(sol, alone))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("fixed", [False, True], ids=["adaptive", "fixed"])
def test_sampled_kernel_stops(bg, wall_case, method, fixed):
    """solve_eom_sampled at N = (0, 2e-4, 1e-3) on the four lane kinds: the statuses of test_target_kernel_stops, n_stored = 1 / 2 / 3
    / 0 -- the lane on the wall emits the sample at 0 and no more, the lane that runs at the wall the first two --, NaN exactly
    where the host build has NaN, and the "away" lanes equal to a call without the others.  A second call, fixed dt, puts the last
    sample out of reach: the "away" lanes run all 2000 steps, eight launches, and the lanes that stopped in the first must still
    come out as from a B = 1 call."""
    art, p, _ = wall_case
    init = batch(fixed)
    kind = np.arange(B) % 4
    options = dict(max_steps=MAX_STEPS, max_err=MAX_ERR, solver=method, dt=FIXED_DT if fixed else None, stop_at_end=False)
    twin_options = dict(max_err=MAX_ERR, dt=FIXED_DT if fixed else None)
    stwin = SampledTwin(art)
    for samples in (SAMPLES,) + (((0.0, 2e-4, 1.0),) if fixed else ()):
        reached = samples[-1] < 1.0
        sol = bg.solve_eom_sampled(art, p, samples, init[:, :2], init[:, 2:], **options)
        got = np.concatenate([sol.states, sol.N[:, :, None], sol.t[:, :, None], sol.eps_H[:, :, None]], axis=2)  # (B, S, 8), the host twin's columns
        away_status = TARGET if reached else COMPLETE
        want_status = (NONFINITE, NONFINITE, away_status, NONFINITE) if fixed else (REJECTED, UNDERFLOW, away_status, NONFINITE)
        want_stored = (1, 2, 3 if reached else 2, 0)
        for k in range(4):
            want, meta = stwin.solve(p, init[k], samples, MAX_STEPS, method, **twin_options)
            lanes = kind == k
            assert meta["status"] == want_status[k] and meta["n_stored"] == want_stored[k]
            assert np.all(sol.status[lanes] == want_status[k]) and np.all(sol.n_stored[lanes] == want_stored[k]), (k, sol.status[lanes], sol.n_stored[lanes])
            assert same(got[lanes], np.broadcast_to(got[k], got[lanes].shape))
            assert np.array_equal(np.isnan(got[k]), np.isnan(want)), (k, got[k], want)
            assert np.isnan(got[k, want_stored[k] :]).all()
            if k != NAN and (fixed or k == WALL):
                rel = np.abs(got[k] - want) / np.maximum(np.abs(want), 1e-3)
                assert np.nanmax(rel) <= TOL, (k, np.nanmax(rel))
        assert np.isnan(sol.N_end).all()
        for k in range(4):
            one = bg.solve_eom_sampled(art, p, samples, init[k : k + 1, :2], init[k : k + 1, 2:], **options)
            assert all(same(np.asarray(a)[k : k + 1], b) for a, b in zip(sol, one)), k
        away = np.flatnonzero(kind == AWAY_K)
        alone = bg.solve_eom_sampled(art, p, samples, init[away, :2], init[away, 2:], **options)
        assert all(same(np.asarray(a)[away], b) for a, b in zip(sol, alone))


def borrowed_batch(n=24):
    """(n, 4): at every third index a stopping lane, REJECTED and UNDERFLOW in turn -- eight of them --, among "away" lanes"""
    init = np.tile(np.array(BORROWED_AWAY), (n, 1))
    stops = np.arange(0, n, 3)
    init[stops[0::2]] = BORROWED_REJECTED
    init[stops[1::2]] = TOWARD
    want = np.full(n, TARGET)
    want[stops[0::2]], want[stops[1::2]] = REJECTED, UNDERFLOW
    return init, want


@pytest.mark.parametrize("method", METHODS)
def test_transfer_kernel_stops(bg, wall_case, method):
    """transfer_functions borrows inflx_bg_step_taken.  mu_s2 holds d^2V/dphi^2 = 3 m / (4 sqrt(phi)), infinite on the wall itself, so
    the REJECTED lane starts one hair inside it (test_background_stops.py); the sample lies beyond the wall, so a stopped lane has
    emitted nothing: REJECTED and UNDERFLOW, every output NaN, and the "away" lanes equal to a call without the stopped ones."""
    art, p, _ = wall_case
    init, want = borrowed_batch()
    options = dict(max_steps=MAX_STEPS, max_err=MAX_ERR, solver=method, stop_at_end=False)
    sol = bg.transfer_functions(art, p, BORROWED_SAMPLES, init[:, :2], init[:, 2:], **options)
    assert np.array_equal(sol.status, want), sol.status
    stopped = want != TARGET
    assert np.all(sol.n_stored[stopped] == 0) and np.all(sol.n_stored[~stopped] == 1)
    for f in ("T_SS", "T_RS", "t", "N", "eps_H", "states", "N_end", "T_SS_end", "T_RS_end"):
        assert np.isnan(getattr(sol, f)[stopped]).all(), f
    assert np.isfinite(sol.T_SS[~stopped]).all() and np.isfinite(sol.T_RS[~stopped]).all() and np.isfinite(sol.states[~stopped]).all()
    alone = bg.transfer_functions(art, p, BORROWED_SAMPLES, init[~stopped, :2], init[~stopped, 2:], **options)
    assert all(same(np.asarray(a)[~stopped], b) for a, b in zip(sol, alone))
    # the lane on the wall itself: not finite in the transfer init, before a step is tried
    on_wall = bg.transfer_functions(art, p, BORROWED_SAMPLES, [WALL_START[:2]], [WALL_START[2:]], **options)
    assert on_wall.status[0] == NONFINITE and np.isnan(on_wall.T_SS).all()


@pytest.mark.parametrize("method", METHODS)
def test_mode_kernel_stops(bg, wall_case, method):
    """power_spectra on the same batch, one wavenumber that leaves the horizon at N = 2e-4 and starts at the initial state, evaluated
    at N = 1e-3, beyond the wall.  The REJECTED lane stops in the front end's first stage (the sampled kernel) and keeps that status,
    the UNDERFLOW lane reaches its exit and stops in the second, the mode kernel; both have NaN in every output and the "away"
    lanes equal a call without them.  The mode kernel itself, called as the front end calls it, gives REJECTED as well."""
    art, p, _ = wall_case
    init, want = borrowed_batch()
    options = dict(N_eval=TARGET_N, N_sub=BORROWED_N_EXIT[0], max_steps=MAX_STEPS, max_err=MAX_ERR, solver=method, stop_at_end=False)
    sol = bg.power_spectra(art, p, BORROWED_N_EXIT, init[:, :2], init[:, 2:], **options)
    assert np.array_equal(sol.status[:, 0], want), sol.status[:, 0]
    stopped = want != TARGET
    for f in ("P_R", "P_S", "C_RS", "N", "eps_H", "modes", "N_end"):
        assert np.isnan(getattr(sol, f)[stopped]).all(), f
    assert np.isnan(sol.k[want == REJECTED]).all()  # (the UNDERFLOW lane reached its exit: its k is known)
    assert np.isfinite(sol.P_R[~stopped]).all() and np.isfinite(sol.modes[~stopped]).all()
    alone = bg.power_spectra(art, p, BORROWED_N_EXIT, init[~stopped, :2], init[~stopped, 2:], **options)
    assert all(same(np.asarray(a)[~stopped], b) for a, b in zip(sol, alone))
    lib = bg._dylib(art, background=False)
    kappa, target = np.ones(init.shape[0]), np.full(init.shape[0], TARGET_N)
    out, _, status = lib.mode_spectra(p, init, kappa, target, MAX_STEPS, bg._METHODS[method], MAX_ERR, 0.0, 0)
    assert np.array_equal(status, want), status
    out2, _, status2 = lib.mode_spectra(p, init[~stopped], kappa[~stopped], target[~stopped], MAX_STEPS, bg._METHODS[method], MAX_ERR, 0.0, 0)
    assert np.array_equal(out[:, ~stopped], out2) and np.all(status2 == TARGET)
