"""The stop statuses of the background stepper (csrc/inflx_background.h) that nothing else reaches -- REJECTED, UNDERFLOW and the two
mid-run NONFINITE exits -- and a lane that ends inside a row that is not yet written, all without a GPU: the numpy restatement
against the host build, and the host build with and without contraction.

The instrument is ``background_reference.wall_model``: V = V0 + m phi^(3/2) on a flat field space, finite at phi = 0 (V = V0,
dV = 0) and NaN for every phi < 0.  A lane at phi = 0 with phidot = -1 evaluates a stage at phi < 0 in every trial step of every
size: the adaptive controller cuts dt by 0.2 fifty times (1e-10 -> ~1e-45, still a normal double, and t + dt != t at t = 0) and
returns REJECTED; a fixed step returns NONFINITE from the trial.  A lane that starts a little inside and runs at the wall creeps up
to it until t + dt == t: UNDERFLOW.  None of this depends on rounding, which ``test_statuses_do_not_depend_on_contraction`` guards:
the device contracts a*b+c into FMAs and the host twin does not, and inputs whose status depended on that could not be asserted
on the GPU (tests/test_background_stops_gpu.py takes its lanes from here).  The number of steps an UNDERFLOW lane takes does
depend on it (70 against 68 with rk4), so no test asserts it across builds.
"""

import functools
import math

import numpy as np
import pytest

import workloads
from background_reference import COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW, BackgroundTwin, Restatement, wall_artifact
from background_sampled_reference import SampledTwin
from background_target_reference import TARGET, TargetTwin

METHODS = ("rk4", "rkf")

WALL_START = (0.0, 0.0, -1.0, 0.0)  # on the wall, moving into it
TOWARD = (1e-3, 0.0, -1.0, 0.0)  # reaches the wall at t = 1.001043e-3
TOWARD_FIXED = (1.05e-3, 0.0, -1.0, 0.0)  # with dt = 1e-4: ten steps, the eleventh has a stage at phi < 0
AWAY = (0.0, 0.0, 1.0, 0.0)
MAX_ERR = 1e-8

# init, options of ``solve``, status, and (last_row, accepted) where the step sequence does not depend on rounding.  The first five
# are arithmetic-independent throughout; on the UNDERFLOW rows only the status is.
CASES = {
    "rejected": (WALL_START, dict(rows=6), REJECTED, (0, 0)),
    "trial-nonfinite": (WALL_START, dict(rows=6, dt=1e-3), NONFINITE, (0, 0)),
    "away": (AWAY, dict(rows=6), COMPLETE, (5, 5)),
    "fixed-into-wall": (TOWARD_FIXED, dict(rows=30, dt=1e-4), NONFINITE, (10, 10)),
    "fixed-into-wall-substeps": (TOWARD_FIXED, dict(rows=12, dt=1e-4, substeps=3), NONFINITE, (3, 10)),  # row 4 is NaN: step 10 is lost
    "underflow": (TOWARD, dict(rows=400, max_err=MAX_ERR), UNDERFLOW, None),
    "underflow-substeps": (TOWARD, dict(rows=60, max_err=MAX_ERR, substeps=7), UNDERFLOW, None),
    "underflow-near": ((1.5e-10, 0.0, -1.0, 0.0), dict(rows=400, max_err=MAX_ERR), UNDERFLOW, None),
    "underflow-turning": ((1e-3, 0.3, -1.0, 0.2), dict(rows=400, max_err=1e-10), UNDERFLOW, None),
    "underflow-slow": ((2e-2, 0.0, -0.5, 0.0), dict(rows=400, max_err=1e-6), UNDERFLOW, None),
}

# rows 0 .. 7 of an adaptive "away" run: seven steps of 1e-10 * 5^k, every factor clamped (the "away" case of ``CASES`` has five)
CLAMPED_ROWS = 8

# rk4, dt = 0.02: every stage of the first step is at phi >= 0 and the step ends at phi < 0, where the right-hand side is NaN -- the
# NONFINITE exit after the accepted state.  The window of phi_0 for that is [0.01961583, 0.01961641]; this is its middle, 2.7e-7 from
# either end, and the rounding of one step is ~1e-18.  (Fehlberg's last stages lie beyond its fourth-order end point: no such window.)
ACCEPTED_THEN_NAN = (0.0196161, 0.0, -1.0, 0.0)
ACCEPTED_THEN_NAN_DT = 0.02

# lanes of the target and the sampled stepper: init, options, status, samples stored, the accepted step that emits the second sample
TARGET_N = 1e-3
SAMPLES = (0.0, 2e-4, 1e-3)
MAX_STEPS = 2000
STOP_LANES = {
    "rejected": (WALL_START, {}, REJECTED, 1, None),
    "trial-nonfinite": (WALL_START, dict(dt=1e-3), NONFINITE, 1, None),
    "trial-nonfinite-1e-4": (WALL_START, dict(dt=1e-4), NONFINITE, 1, None),
    "fixed-into-wall": (TOWARD_FIXED, dict(dt=1e-4), NONFINITE, 2, 3),
    "underflow": (TOWARD, {}, UNDERFLOW, 2, 11),
    "away": (AWAY, {}, TARGET, 3, None),
    "away-fixed": (AWAY, dict(dt=1e-4), TARGET, 3, None),
}

# a lane that ends inside a row: the hyperbolic model at its workload parameters, dt = 1e-3, stop_at_end; the end is accepted step 652
PENDING_INIT = (1.3, 0.3, 0.0, 0.05)
PENDING_DT, PENDING_SUBSTEPS, PENDING_ROWS, PENDING_FINE_ROWS = 1e-3, 300, 5, 1201


@functools.lru_cache(maxsize=None)
def wall():
    """(artefact, parameter row) of the wall model, compiled once"""
    return wall_artifact()


@functools.lru_cache(maxsize=None)
def wall_twin(contract="off"):
    return BackgroundTwin(wall()[0], contract=contract)


def wall_restatement():
    twin, p = wall_twin(), wall()[1]

    def eom(a, b, c, d, pp):
        return tuple(twin.eom(pp, np.array([[a, b, c, d]]))[0])

    return Restatement(eom, p)


def _solve(solver, init, method, options):
    options = dict(options)
    rows = options.pop("rows")
    if isinstance(solver, Restatement):
        return solver.solve(init, rows, method, **options)
    return solver.solve(wall()[1], init, rows, method, **options)


def test_the_wall_model_is_finite_on_the_wall_and_nan_behind_it():
    got = wall_twin().eom(wall()[1], np.array([[0.0, 0.0, -1.0, 0.0], [-1e-300, 0.0, -1.0, 0.0], [-0.0, 0.0, 1.0, 0.0]]))
    assert np.array_equal(got[0], [0.0, 0.0, 1.0, 1.0]) and np.array_equal(got[2], [0.0, 0.0, 1.0, 1.0])
    assert np.isnan(got[1, 0]) and np.isnan(got[1, 2])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", CASES)
def test_restatement_and_host_build_stop_alike(case, method):
    """``Restatement.solve`` and the host build give the same status, last_row, accepted count and NaN pattern on every case, and
    their states agree within 1e-13 (test_host_integrator_matches_restatement's bar).  A lane that stops in mid-row with a status
    other than ENDED leaves that row NaN and last_row at the last complete row."""
    init, options, status, counts = CASES[case]
    want, wm = _solve(wall_restatement(), init, method, options)
    got, gm = _solve(wall_twin(), init, method, options)
    assert wm["status"] == gm["status"] == status
    assert (gm["last_row"], gm["accepted"]) == (wm["last_row"], wm["accepted"])
    if counts is not None:
        assert (gm["last_row"], gm["accepted"]) == counts
    last = gm["last_row"]
    assert last < options["rows"] - 1 or status == COMPLETE
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isfinite(got[: last + 1]).all() and np.isnan(got[last + 1 :]).all()
    rel = np.abs(got[: last + 1] - want[: last + 1]) / np.maximum(np.abs(want[: last + 1]), 1e-3)
    assert rel.max() <= 1e-13, rel.max()
    assert math.isnan(gm["N_end"]) and math.isnan(wm["N_end"])
    if status == UNDERFLOW:
        substeps = options.get("substeps", 1)
        assert last == gm["accepted"] // substeps
        assert np.all(np.diff(got[: last + 1, 0]) < 0) and np.all(got[: last + 1, 0] > 0) and np.all(np.diff(got[: last + 1, 6]) > 0)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", CASES)
def test_statuses_do_not_depend_on_contraction(case, method):
    """The host build with FMAs (-ffp-contract=fast -mfma), which is how the device rounds, reaches the same status on every case;
    on the five arithmetic-independent cases also the same last_row and accepted count, and states within 1e-15 of the build
    without (measured: 1.1e-16 relative).  This is a condition on the inputs: one that fails it is replaced, not excused."""
    init, options, status, counts = CASES[case]
    off, om = _solve(wall_twin(), init, method, options)
    fast, fm = _solve(wall_twin("fast"), init, method, options)
    print(f"{case} {method}: accepted {om['accepted']} without contraction, {fm['accepted']} with")
    assert om["status"] == fm["status"] == status
    if counts is not None:
        assert (fm["last_row"], fm["accepted"]) == (om["last_row"], om["accepted"]) == counts
        assert np.array_equal(np.isnan(off), np.isnan(fast))
        last = om["last_row"]
        rel = np.abs(off[: last + 1] - fast[: last + 1]) / np.maximum(np.abs(off[: last + 1]), 1e-3)
        assert rel.max() <= 1e-15, rel.max()


def test_right_hand_side_at_the_accepted_state():
    """The second NONFINITE exit of a fixed step: the trial step is finite, the state it reaches has phi < 0, and the right-hand side
    there is NaN.  The restatement counts that step as accepted (it was taken) before it stops; both host builds stop with the same
    status, row 1 is NaN and last_row is 0.  One per cent further from the wall the same step completes; at phi_0 = 0.0196 a stage
    is already behind the wall and the trial itself is not finite."""
    p = wall()[1]
    want, wm = wall_restatement().solve(ACCEPTED_THEN_NAN, 4, "rk4", dt=ACCEPTED_THEN_NAN_DT)
    assert (wm["status"], wm["last_row"], wm["accepted"]) == (NONFINITE, 0, 1) and np.isnan(want[1:]).all()
    for contract in ("off", "fast"):
        got, gm = wall_twin(contract).solve(p, ACCEPTED_THEN_NAN, 4, "rk4", dt=ACCEPTED_THEN_NAN_DT)
        assert (gm["status"], gm["last_row"]) == (NONFINITE, 0) and np.isnan(got[1:]).all() and np.array_equal(got[0], want[0])
    _, far = wall_restatement().solve((ACCEPTED_THEN_NAN[0] * 1.01, 0.0, -1.0, 0.0), 2, "rk4", dt=ACCEPTED_THEN_NAN_DT)
    _, near = wall_restatement().solve((0.0196, 0.0, -1.0, 0.0), 2, "rk4", dt=ACCEPTED_THEN_NAN_DT)
    assert (far["status"], far["accepted"]) == (COMPLETE, 1) and (near["status"], near["accepted"]) == (NONFINITE, 0)


@pytest.mark.parametrize("method", METHODS)
def test_underflow_is_reached_at_the_wall(method):
    """Both host builds stop the (1e-3, 0, -1, 0) lane where the trajectory meets the wall, t = 1.001043e-3, with the last stored
    phi ~ 1e-19: the window tests/test_background_stops_gpu.py asserts on the device leaves the fourth digit of that time open."""
    init, options, _, _ = CASES["underflow"]
    for contract in ("off", "fast"):
        out, meta = _solve(wall_twin(contract), init, method, options)
        last = meta["last_row"]
        assert 1.0010e-3 <= out[last, 6] <= 1.0011e-3 and 0.0 < out[last, 0] < 1e-15, (contract, out[last])
        assert abs(out[last, 6] - 1.001043e-3) < 1e-9


@pytest.mark.parametrize("method", METHODS)
def test_away_lane_of_the_long_adaptive_calls(method):
    """The "away" lane of the GPU batches: COMPLETE over 80 rows (and 12 rows of 7 substeps) on both host builds, and still COMPLETE
    ten rows later, so that its status there does not hang on a step more or less.  While the controller's factor is clamped at 5
    -- the first seven steps -- its steps do not depend on rounding; after that dt follows an error estimate of ~1e-9 taken
    from differences of O(1) numbers, whose rounding noise is ~1e-7 relative, and the two builds drift apart (measured: 2.7e-8
    relative over 80 rows with rk4, 7e-10 with rkf).  ``CLAMPED_ROWS`` is what the GPU test compares with this build."""
    for rows, substeps in ((80, 1), (12, 7), (90, 1)):
        runs = [wall_twin(c).solve(wall()[1], AWAY, rows, method, max_err=MAX_ERR, substeps=substeps) for c in ("off", "fast")]
        for out, meta in runs:
            assert meta["status"] == COMPLETE and meta["last_row"] == rows - 1 and np.isfinite(out).all()
        if substeps == 1:
            t, dt, want_t = 0.0, 1e-10, [0.0]
            for _ in range(CLAMPED_ROWS - 1):
                t, dt = t + dt, dt * 5.0
                want_t.append(t)
            assert np.array_equal(runs[0][0][:CLAMPED_ROWS, 6], want_t) and np.array_equal(runs[1][0][:CLAMPED_ROWS, 6], want_t)
            head = np.abs(runs[0][0][:CLAMPED_ROWS] - runs[1][0][:CLAMPED_ROWS]) / np.maximum(np.abs(runs[0][0][:CLAMPED_ROWS]), 1e-3)
            assert head.max() <= 1e-15, head.max()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("lane", STOP_LANES)
def test_target_and_sampled_steppers_stop_alike(lane, method):
    """The same lanes through inflx_bg_step_target and inflx_bg_step_sampled (host builds): the status of the plain stepper, the
    samples emitted before the stop and NaN after them, with and without stop_at_end, and the sampled stepper with FMAs too."""
    init, options, status, n_stored, second_from = STOP_LANES[lane]
    art, p = wall()
    for stop_at_end in (False, True):
        _, tm = TargetTwin(art).solve(p, init, TARGET_N, MAX_STEPS, method, max_err=MAX_ERR, stop_at_end=stop_at_end, **options)
        assert tm["status"] == status
        accepted = None
        for contract in ("off", "fast"):
            out, sm = SampledTwin(art, contract=contract).solve(p, init, SAMPLES, MAX_STEPS, method, max_err=MAX_ERR, stop_at_end=stop_at_end, **options)
            assert sm["status"] == status and sm["n_stored"] == n_stored
            assert np.isfinite(out[:n_stored]).all() and np.isnan(out[n_stored:]).all()
            assert sm["step_of"][0] == 0 and np.isnan(sm["step_of"][n_stored:]).all()
            if second_from is not None:
                assert sm["step_of"][1] == second_from
            accepted = sm["accepted"] if accepted is None else accepted
        assert tm["accepted"] == accepted or status == TARGET  # (the target stepper stops at its target, the sampled one at its last sample)


def pending_inits(B=65):
    """(B, 4): the lane that ends inside a row and its neighbours, phi_0 = 1.3 + 0.002 k"""
    init = np.tile(np.array(PENDING_INIT), (B, 1))
    init[:, 0] += 0.002 * np.arange(B)
    return init


@pytest.mark.parametrize("method", METHODS)
def test_lane_that_ends_inside_a_row(method):
    """Hyperbolic model, dt = 1e-3, stop_at_end: the lane ends at accepted step 652.  With 300 substeps that is inside row 3, which
    is complete at step 899 -- on the device two launches of 256 steps later --, so the end state has to wait for its row: the
    coarse row 3 is the fine row 652 bit for bit, N_end is equal and row 4 is NaN.  Every lane of the GPU test's batch ends in
    (512, 768), and at no multiple of 300."""
    spec, art = workloads.artifact_for("hyperbolic")
    twin = BackgroundTwin(art)
    ends = []
    for k, init in enumerate(pending_inits()):
        fine, fm = twin.solve(spec.args, init, PENDING_FINE_ROWS, method, dt=PENDING_DT, stop_at_end=True)
        r = fm["last_row"]
        ends.append(r)
        assert fm["status"] == ENDED and fm["accepted"] == r and 512 < r < 768 and r % PENDING_SUBSTEPS
        if k % 16 == 0:
            coarse, cm = twin.solve(spec.args, init, PENDING_ROWS, method, dt=PENDING_DT, substeps=PENDING_SUBSTEPS, stop_at_end=True)
            row = -(-r // PENDING_SUBSTEPS)
            assert row == 3 and cm["status"] == ENDED and cm["last_row"] == row and cm["accepted"] == r
            assert np.array_equal(coarse[row], fine[r]) and cm["N_end"] == fm["N_end"]
            assert np.array_equal(coarse[:row], fine[: r : PENDING_SUBSTEPS][:row]) and np.isnan(coarse[row + 1 :]).all() and np.isnan(fine[r + 1 :]).all()
    assert ends[0] == 652
    print(f"{method}: end steps {ends}")


# ---- the steppers that borrow inflx_bg_step_taken ------------------------------------------------------------------------------------
# mu_s2 and the mass matrix hold d^2V/dphi^2 = 3 m / (4 sqrt(phi)), which is infinite on the wall itself: a lane at phi = 0 is
# NONFINITE in their init, before a step is tried.  One subnormal-free hair inside, phi = 1e-300, every quantity is finite and every
# trial step of every size the controller can reach (>= 1e-45) still has its first stage at phi < 0: REJECTED, as on the wall.
BORROWED_REJECTED = (1e-300, 0.0, -1.0, 0.0)
BORROWED_AWAY = (0.5, 0.0, 1.0, 0.0)
BORROWED_N_EXIT = (2e-4,)  # power_spectra: the mode leaves the horizon here and starts N_sub = 2e-4 before, at the initial state
BORROWED_SAMPLES = (1e-3,)  # beyond the wall for TOWARD (N = 7e-4 there): a stopped lane has emitted nothing


@pytest.mark.parametrize("method", METHODS)
def test_borrowed_steppers_stop_alike(method):
    """The transfer and the mode stepper (host builds, with and without FMAs) on the two stopping lanes and an "away" lane:
    REJECTED, UNDERFLOW, TARGET; the lane on the wall itself is NONFINITE at once."""
    from modes_reference import ModesTwin
    from transfer_reference import TransferTwin

    art, p = wall()
    lanes = np.array([BORROWED_REJECTED, TOWARD, BORROWED_AWAY, WALL_START])
    for contract in ("off", "fast"):
        sol = TransferTwin(art, contract=contract).solve(p, BORROWED_SAMPLES, lanes[:, :2], lanes[:, 2:], MAX_STEPS, MAX_ERR, method, stop_at_end=False)
        assert list(sol.status) == [REJECTED, UNDERFLOW, TARGET, NONFINITE] and list(sol.n_stored) == [0, 0, 1, 0]
        assert np.isnan(sol.T_SS[[0, 1, 3]]).all() and np.isnan(sol.T_RS[[0, 1, 3]]).all() and np.isfinite(sol.T_SS[2]).all()
        got = ModesTwin(art, contract=contract).lanes(p, lanes, 1.0, TARGET_N, MAX_STEPS, MAX_ERR, method, stop_at_end=False)
        assert list(got.status) == [REJECTED, UNDERFLOW, TARGET, NONFINITE]
        assert got.accepted[0] == 0 and got.accepted[3] == 0
        # through the front end's two stages: the REJECTED lane stops in the first, the sampled run; the UNDERFLOW lane in the second
        spectra = ModesTwin(art, contract=contract).power_spectra(p, BORROWED_N_EXIT, lanes[:, :2], lanes[:, 2:], N_eval=TARGET_N, N_sub=BORROWED_N_EXIT[0],
                                                                  max_steps=MAX_STEPS, max_err=MAX_ERR, solver=method, stop_at_end=False)  # fmt: skip
        # (the lane on the wall never reaches the second stage either: the first stage's stepper is the plain one, finite at phi = 0)
        assert list(spectra.status[:, 0]) == [REJECTED, UNDERFLOW, TARGET, REJECTED]
        assert np.isnan(spectra.P_R[[0, 1, 3]]).all() and np.isfinite(spectra.P_R[2]).all()
