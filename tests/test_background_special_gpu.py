"""Special-function models under the background solver on the GPU (``Compiler(link_gsl=True)``, csrc/inflx_sf.h): ``kinematics`` and
``masses`` against the 40-digit truth, adaptive trajectories against DOP853, every companion object of the solver built, loaded and
read for its status word, and the domain-error contract of the integrating calls -- a trial step that left a function's domain and
was retried fails nothing, a trajectory that stopped NONFINITE there does under "raise" and returns NaN rows under "nan".  Models,
lanes, truths and bounds are those tests/test_background_special.py establishes on the host builds."""

if __name__ == "__main__":  # run as a script (the profile writer at the end): the repository root on the path, as under pytest
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import math

import numpy as np
import pytest

import background_special as bs
import background_truth as bt
import kinematics_reference as kr
import masses_reference as mr
from background_reference import COMPLETE, ENDED, NONFINITE, UNDERFLOW, BackgroundTwin
from background_sampled_reference import SampledTwin
from background_target_reference import TARGET

pytestmark = pytest.mark.gpu

MODELS = bt.SPECIAL_VALUE_MODELS
MAX_ERR = 1e-8
RATIOS = {}  # worst ratio to each bar, per model and family: what `python tests/test_background_special_gpu.py` writes to profiles/


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def sf_error():
    from inflatox_amd._native import InflatoxSpecialFunctionError

    return InflatoxSpecialFunctionError


def _handle(bg, art):
    """the artefact's background handle: ``sf_status()`` reads and clears the status words of every code object it has loaded"""
    return bg._dylib(art, background=False)


@pytest.fixture
def wall(bg):
    """the ``j52_wall`` artefact with a clear status word, left under the default policy afterwards"""
    art = bt.device_artifact("j52_wall")
    bg.set_sf_errors(art, "raise")
    _handle(bg, art).sf_status()
    yield art
    bg.set_sf_errors(art, "raise")
    _handle(bg, art).sf_status()


# ---- values ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MODELS)
def test_point_level_against_truth(bg, name):
    """65 states (a wavefront and one lane), one parameter row each: the six kinematic quantities and the eight of ``masses`` within
    the project's allowances of the 40-digit truth.  First derivatives shift a Bessel order by one, second ones by two (K_nu-2 ..
    K_nu+2, J_2, I_2; 1F1 and 2F1 with both parameters raised twice): a wrong order or sign on the device fails here, as it does on
    the host build in tests/test_background_special.py."""
    art = bt.device_artifact(name)
    states, pars = (a[: bs.STATES] for a in kr.zoo_states(name))
    kin = np.stack(bg.kinematics(art, pars, states))
    mass = np.stack(bg.masses(art, pars, states))
    r_kin = kr.worst_ratios(kin, kr.zoo_truth(name, bs.STATES), states[:, 4])
    r_mass = mr.worst_ratios(mass, mr.zoo_truth(name, bs.STATES), states[:, 4])
    RATIOS[f"{name}/kinematics"], RATIOS[f"{name}/masses"] = r_kin, r_mass
    print(f"{name}: worst |GPU - truth| / allowance, kinematics {r_kin}, masses {r_mass}")
    assert kin.shape == (6, bs.STATES) and mass.shape == (8, bs.STATES) and np.isfinite(kin).all() and np.isfinite(mass).all()
    assert max(r_kin.values()) <= 1.0 and max(r_mass.values()) <= 1.0, (r_kin, r_mass)
    assert np.array_equal(mass[4], kin[0]) and np.array_equal(mass[5], kin[2])
    assert _handle(bg, art).sf_status() == 0


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", MODELS)
def test_adaptive_trajectories_against_truth(bg, name, solver):
    """16 lanes with their own parameter rows, adaptive at max_err = 1e-8.  ``solve_eom_batch``, 160 rows: every row up to T = 2
    against DOP853 at the row's own t.  ``solve_eom_sampled`` at the four times ``SAMPLES_T``.  Both with the bound of
    tests/test_background_truth_gpu.py: a lane's error is at most twice that of the host build of the same stepper with FMA
    contraction on the same lane, plus 1e-11, the bound on the truth's own error."""
    art = bt.device_artifact(name)
    init, pars = (a[: bs.LANES] for a in bt.batch(name))
    truth = bt.truths(name, bs.LANES, bt.T_ADAPTIVE)
    rows = 160
    sol = bg.solve_eom_batch(art, pars, rows, init[:, :2], init[:, 2:], MAX_ERR, solver)
    assert np.all(sol.status == COMPLETE) and np.all(sol.last_row == rows - 1)
    got = bs.rows_of(sol)
    assert np.isfinite(got).all()
    twin = BackgroundTwin(bt.host_artifact(name), contract="fast")
    err_gpu, err_host = np.empty(bs.LANES), np.empty(bs.LANES)
    for k in range(bs.LANES):
        out, meta = twin.solve(pars[k], init[k], rows, solver, max_err=MAX_ERR)
        assert meta["status"] == COMPLETE
        for rows_k, err in ((got[k], err_gpu), (out, err_host)):
            inside = rows_k[:, 6] <= bt.T_ADAPTIVE
            assert inside.sum() >= 20  # (the comparison is over a trajectory, not over its first steps)
            err[k] = bt.error_against_truth(rows_k[inside], truth[k])
    RATIOS[f"{name}/trajectory/{solver}/rows"] = float(np.max(err_gpu / (2.0 * err_host + bt.TRUTH_TOL)))
    print(f"{name} {solver} rows: error against the truth, GPU {err_gpu.max():.3e}, host build {err_host.max():.3e}")
    assert np.all(err_gpu <= 2.0 * err_host + bt.TRUTH_TOL), (int(np.argmax(err_gpu / err_host)), err_gpu.max(), err_host.max())

    sam = bg.solve_eom_sampled(art, pars, bt.SAMPLES_T, init[:, :2], init[:, 2:], solver=solver, at="t", stop_at_end=False)
    assert np.all(sam.status == TARGET) and np.all(sam.n_stored == 4), (sam.status, sam.n_stored)
    got = np.concatenate([sam.states, sam.N[..., None], sam.t[..., None]], axis=2)
    stwin = SampledTwin(bt.host_artifact(name), contract="fast")
    for k in range(bs.LANES):
        out, meta = stwin.solve(pars[k], init[k], bt.SAMPLES_T, 100_000, solver, max_err=MAX_ERR, at="t", stop_at_end=False)
        assert meta["status"] == TARGET
        err_gpu[k], err_host[k] = bt.error_against_truth(got[k], truth[k]), bt.error_against_truth(out, truth[k])
    RATIOS[f"{name}/trajectory/{solver}/sampled"] = float(np.max(err_gpu / (2.0 * err_host + bt.TRUTH_TOL)))
    print(f"{name} {solver} at SAMPLES_T: error against the truth, GPU {err_gpu.max():.3e}, host build {err_host.max():.3e}")
    assert np.all(err_gpu <= 2.0 * err_host + bt.TRUTH_TOL), (int(np.argmax(err_gpu / err_host)), err_gpu.max(), err_host.max())
    assert _handle(bg, art).sf_status() == 0


# ---- every companion object, on bessel_skew --------------------------------------------------------------------------------------
def _family_calls(art, p, init):
    """{family: (companion objects, call(lib))}: one short native call per integrating entry point on the states ``init`` (B, 4)"""
    from inflatox_amd import _native

    B = init.shape[0]
    rkf, nan = _native.EOM_RKF, math.nan
    kappa, target, shift = np.full(B, 20.0), np.full(B, 0.05), np.zeros(B)
    samples = np.array([0.01, 0.03])
    return {
        "transfer": (("transfer",), lambda lib: lib.transfer_functions(p, init, None, samples, 64, rkf, 1e-8, 0.0, 0)),
        "modes": (("modes",), lambda lib: lib.mode_spectra(p, init, kappa, target, 64, rkf, 1e-8, 0.0, 0)),
        "tensor": (("tensor",), lambda lib: lib.mode_spectra(p, init, kappa, target, 64, rkf, 1e-8, 0.0, _native.MODES_TENSOR)),
        "evolution": (("evolution",), lambda lib: lib.mode_evolution(p, init, kappa, target, shift, samples, 64, rkf, 1e-8, 0.0, 0)),
        "deltan": (("deltan",), lambda lib: lib.delta_n(p, init, None, _native.DN_FIXED, 1e-2, 1e-2, np.full(B, 0.5), 64, rkf, 1e-8, 0.0)),
        "stochastic": (("stochastic",), lambda lib: lib.stochastic_efolds(p, init, 2, None, 3, 1.0, 1.0 / 32.0, nan, 64, rkf, 1e-8, 0.0)),
        "distribution": (("distribution",), lambda lib: lib.stochastic_distribution(p, init, 4, None, 3, 0, 0, 1.0, 1.0 / 32.0, 64, rkf, 1e-8, 0.0, 8, np.array([[0.0, 1.0]]))),
        "crossing": (("crossing",), lambda lib: lib.solve_eom_crossings(p, init, np.zeros(B), np.array([0.1, 0.2]), 64, rkf, 1e-8, 0.0, 0)),
        "inflation_end": (("crossing",), lambda lib: lib.inflation_end(p, init, 64, rkf, 1e-8, 0.0)),
    }


FAMILIES = ("transfer", "modes", "tensor", "evolution", "deltan", "stochastic", "distribution", "crossing", "inflation_end")


@pytest.mark.parametrize("family", FAMILIES)
def test_every_companion_object_reports_its_status_word(bg, sf_error, family):
    """``bessel_skew``: the family's object builds for a ``link_gsl=True`` model and loads, and its INFLX_SF_STATUS word is found:
    a short call on three states inside the box leaves ``sf_status()`` at 0; the same call with a fourth state at x = -1.5, where
    K_nu(x + 1) is outside its domain, returns under "nan" with ``sf_status()`` = SF_EDOM -- the word of THIS object, the only one
    the call ran -- and raises ERRCODE 0X1 under "raise", after which the word is clear."""
    art = bt.device_artifact("bessel_skew")
    init, pars = (np.array(a[:4]) for a in bt.batch("bessel_skew"))
    objects, call = _family_calls(art, pars[:3], init[:3])[family]
    lib = bg._companion_dylib(art, *objects)
    bg.set_sf_errors(art, "raise")
    lib.sf_status()
    try:
        call(lib)
        assert lib.sf_status() == 0
        init[3, 0] = -1.5
        _objects, call = _family_calls(art, pars, init)[family]
        bg.set_sf_errors(art, "nan")
        call(lib)
        assert lib.sf_status() == bs.SF_EDOM and lib.sf_status() == 0
        bg.set_sf_errors(art, "raise")
        with pytest.raises(sf_error, match="ERRCODE 0X1"):
            call(lib)
        assert lib.sf_status() == 0
    finally:
        bg.set_sf_errors(art, "raise")
        lib.sf_status()


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_stochastic_lanes_are_the_twins(bg, solver):
    """``stochastic_efolds`` on ``bessel_skew`` -- I_0 in the Cholesky factor of the kicks, I_1 in their drift --, 3 points with their
    own parameter rows x 130 realisations, 200 steps at a fixed dt with the same Philox stream: N, the final state and the status of
    every lane are the host twin's within 1e-10 + 2 d, d the twin's difference with and without FMA contraction on this case
    (profiles/background_stochastic.json, ``d_bessel_skew``, measured by ``python tests/stochastic_reference.py``)."""
    import stochastic_reference as sr

    art = bt.device_artifact(sr.SPECIAL_MODEL)

    def device(p, pts, R, **kw):
        se = bg.stochastic_efolds(art, p, pts[:, :2], pts[:, 2:], R, return_samples=True, **kw)
        return sr.StochasticResult(se.N.reshape(-1), se.state.reshape(-1, 5), se.status.reshape(-1).astype(np.int64), None, None)

    got = sr.special_run(device, solver)
    want = sr.special_run(sr.StochasticTwin(bt.host_artifact(sr.SPECIAL_MODEL)).run, solver)
    diff = sr.lane_difference(got, want)
    RATIOS[f"{sr.SPECIAL_MODEL}/stochastic/{solver}"] = diff / sr.bound_special()
    print(f"{sr.SPECIAL_MODEL} {solver}: worst |GPU - twin| over the lanes {diff:.3e} (bound {sr.bound_special():.3e}); statuses {np.bincount(want.status)}")
    assert np.isfinite(want.N).all() and want.accepted.max() == sr.SPECIAL_STEPS and diff <= sr.bound_special()
    assert _handle(bg, art).sf_status() == 0


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("family", bs.PARITY_FAMILIES)
def test_every_family_agrees_with_its_host_twin(bg, family, solver):
    """``bessel_skew``, 8 lanes with their own parameter rows at a fixed step (``background_special.parity_results``): what the
    family's public call returns on the device is its host twin's, lane by lane and member by member, within 1e-10 + 2 d of each
    value's scale -- NaN where NaN, statuses and counts equal.  d is the twin's difference with and without FMA contraction on the
    same call, measured on the CPU by ``python tests/background_special.py`` and kept in the family's profiles/background_*.json
    under ``d_bessel_skew``.  The objects compile the equations-of-motion, kinematics, masses and noise headers with their shifted
    Bessel orders: a wrong one in any of them fails here."""
    got = bs.parity_results(family, solver, "gpu")
    want = bs.parity_results(family, solver, "off")
    diff, bar = bs.parity_difference(got, want), bs.parity_bound(family, solver)
    RATIOS[f"{bs.PARITY_MODEL}/{family}/{solver}"] = diff / bar
    print(f"{bs.PARITY_MODEL} {family} {solver}: worst |GPU - twin| {diff:.3e} of scale (bar {bar:.3e})")
    assert diff <= bar, (diff, bar)
    assert _handle(bg, bt.device_artifact(bs.PARITY_MODEL)).sf_status() == 0


# ---- domain errors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_recovered_excursions_fail_nothing(bg, wall, solver):
    """The ``WALL_RECOVERED`` lanes of the solver, adaptive, 120 rows.  Under "nan": every lane COMPLETE, every value finite and
    every phi > 0, and ``sf_status()`` = SF_EDOM: the excursion happened on the device too.  The states match the host twin's at
    matched accepted steps (``background_special.matched_difference``: row by row, the twin's state carried to the device's t with
    the twin's right-hand side) within 1e-10 + 2 d of each value's scale, d the same difference between the twin with and without
    FMA contraction, measured on the CPU by ``python tests/background_special.py`` and kept in profiles/background_special.json
    (``d_j52_wall``).  The rows' t agree to 1e-7: H = 80 and c = 1e4 make |chi''| = 3 H c = 2.5e6, t stays below 0.2, and a time
    offset of 2e-8 leaves a second-order term of 5e-10 in chi, a hundredth of the bar at |chi| = 500.  As a supplement, a lane's
    error against DOP853 at the rows' own t is at most twice that of the host build with FMA contraction, plus 1e-11
    (tests/test_background_truth_gpu.py).  Under "raise": the same call does not raise, returns the same bits, and ``sf_status()``
    reads 0 afterwards."""
    init, pars = bs.wall_lanes(bs.WALL_RECOVERED[solver])
    lib = _handle(bg, wall)
    bg.set_sf_errors(wall, "nan")
    quiet = bg.solve_eom_batch(wall, pars, bs.WALL_ROWS, init[:, :2], init[:, 2:], bs.WALL_MAX_ERR, solver)
    assert np.all(quiet.status == COMPLETE) and np.all(quiet.last_row == bs.WALL_ROWS - 1)
    got = bs.rows_of(quiet)
    assert np.isfinite(got).all() and got[:, :, 0].min() > 0.0
    assert lib.sf_status() == bs.SF_EDOM and lib.sf_status() == 0
    eom = bt.truth_rhs("j52_wall")
    off, _pars = bs.wall_recovered_twins(solver, "off")
    fast, _pars = bs.wall_recovered_twins(solver, "fast")
    assert np.isfinite(fast).all() and np.isfinite(off).all()
    pairs = [bs.matched_difference(got[k], off[k], eom, pars[k]) for k in range(init.shape[0])]
    state, time = max(s for s, _ in pairs), max(t for _, t in pairs)
    bar_state, _bar_t = bs.wall_bound(solver)
    RATIOS[f"j52_wall/recovered/{solver}/matched"] = state / bar_state
    print(f"j52_wall {solver}: GPU against the host twin at matched steps {state:.3e} of scale (bar {bar_state:.3e}), t within {time:.3e}")
    assert state <= bar_state and time <= 1e-7, (state, bar_state, time)
    err_gpu, err_host = np.empty(init.shape[0]), np.empty(init.shape[0])
    for k in range(init.shape[0]):
        truth = bt.truth_trajectory(bt.bound(eom, pars[k]), init[k], 1.01 * max(got[k, -1, 6], fast[k, -1, 6]))
        assert truth.success and truth.y[0].min() > 0.0  # (the solution itself stays inside the domain)
        err_gpu[k], err_host[k] = bt.error_against_truth(got[k], truth), bt.error_against_truth(fast[k], truth)
    RATIOS[f"j52_wall/recovered/{solver}/truth"] = float(np.max(err_gpu / (2.0 * err_host + bt.TRUTH_TOL)))
    print(f"j52_wall {solver}: error against the truth, GPU {err_gpu}, host build {err_host}")
    assert np.all(err_gpu <= 2.0 * err_host + bt.TRUTH_TOL), (err_gpu, err_host)
    bg.set_sf_errors(wall, "raise")
    loud = bg.solve_eom_batch(wall, pars, bs.WALL_ROWS, init[:, :2], init[:, 2:], bs.WALL_MAX_ERR, solver)
    for f in ("states", "t", "N", "status", "last_row"):
        assert np.array_equal(getattr(loud, f), getattr(quiet, f)), f
    assert lib.sf_status() == 0


def _exit_batch():
    """the leaving lane, then seven lanes that stay inside: (init (8, 4), pars (8, 3))"""
    x, p = bs.wall_lanes([bs.WALL_EXIT])
    xi, pi = bs.wall_inside(7)
    return np.concatenate([x, xi]), np.concatenate([p, pi])


def test_a_real_exit_raises_or_returns_nan_rows(bg, wall, sf_error):
    """The lane that reaches phi = 0 at a fixed step among seven in-domain lanes.  Under "raise" the call raises ERRCODE 0X1 and
    names the trajectories' status.  Under "nan" it returns: the leaving lane NONFINITE with NaN rows after ``last_row`` and phi > 0
    before, the seven others COMPLETE and bit-identical to the call without it; ``sf_status()`` reads SF_EDOM, then 0.  The ADAPTIVE
    run of the same lanes stops the leaving lane with UNDERFLOW (tests/test_background_special.py), no lane is NONFINITE, and the
    call does not raise under "raise" and leaves the word clear."""
    init, pars = _exit_batch()
    lib = _handle(bg, wall)
    kw = dict(solver="rkf", dt=bs.WALL_EXIT_DT)
    with pytest.raises(sf_error, match="ERRCODE 0X1") as caught:
        bg.solve_eom_batch(wall, pars, bs.WALL_ROWS, init[:, :2], init[:, 2:], **kw)
    assert "INFLX_EOM_NONFINITE" in str(caught.value) and "Those points hold NaN" not in str(caught.value)
    assert lib.sf_status() == 0
    bg.set_sf_errors(wall, "nan")
    sol = bg.solve_eom_batch(wall, pars, bs.WALL_ROWS, init[:, :2], init[:, 2:], **kw)
    assert lib.sf_status() == bs.SF_EDOM and lib.sf_status() == 0
    last = int(sol.last_row[0])
    assert sol.status[0] == NONFINITE and 0 < last < bs.WALL_ROWS - 1
    assert np.isnan(sol.states[0, last + 1 :]).all() and np.isnan(sol.t[0, last + 1 :]).all() and np.isfinite(sol.states[0, : last + 1]).all()
    assert sol.states[0, : last + 1, 0].min() > 0.0
    assert np.all(sol.status[1:] == COMPLETE)
    alone = bg.solve_eom_batch(wall, pars[1:], bs.WALL_ROWS, init[1:, :2], init[1:, 2:], **kw)
    assert lib.sf_status() == 0
    for f in ("states", "t", "N", "status", "last_row"):
        assert np.array_equal(getattr(sol, f)[1:], getattr(alone, f)), f
    bg.set_sf_errors(wall, "raise")
    adaptive = bg.solve_eom_batch(wall, pars, bs.WALL_ROWS, init[:, :2], init[:, 2:], bs.WALL_MAX_ERR, "rkf")
    assert adaptive.status[0] == UNDERFLOW and np.all(adaptive.status[1:] == COMPLETE)
    assert lib.sf_status() == 0


def test_a_real_exit_on_the_other_paths(bg, wall, sf_error):
    """The same eight lanes through ``solve_eom_batch_device``, ``state_at_efolds``, ``solve_eom_sampled`` and ``stochastic_efolds``
    (noise_scale = 0: the classical trajectories), all at the fixed step: each raises ERRCODE 0X1 under "raise" and returns under
    "nan" with the leaving lane NONFINITE, the others not, and ``sf_status()`` = SF_EDOM, then 0."""
    init, pars = _exit_batch()
    x, v = init[:, :2], init[:, 2:]
    lib = _handle(bg, wall)
    dt = bs.WALL_EXIT_DT
    n_target = 0.01  # H ~ 2: about 500 steps for the lanes that stay inside; the leaving lane meets phi = 0 after about 52
    calls = {
        "device": lambda: bg.solve_eom_batch_device(wall, pars, bs.WALL_ROWS, x, v, solver="rkf", dt=dt).status,
        "efolds": lambda: bg.state_at_efolds(wall, pars, x, v, n_target, 2000, solver="rkf", dt=dt, stop_at_end=False).status,
        "sampled": lambda: bg.solve_eom_sampled(wall, pars, [0.005, n_target], x, v, 2000, solver="rkf", dt=dt, stop_at_end=False).status,
        "stochastic": lambda: bg.stochastic_efolds(wall, pars, x, v, 2, noise_scale=0.0, max_steps=200, solver="rkf", dt=dt).counts[:, NONFINITE] // 2 * NONFINITE,
    }
    for name, call in calls.items():
        bg.set_sf_errors(wall, "raise")
        with pytest.raises(sf_error, match="ERRCODE 0X1"):
            call()
        assert lib.sf_status() == 0, name
        bg.set_sf_errors(wall, "nan")
        status = np.asarray(call())
        assert status[0] == NONFINITE and np.all(status[1:] != NONFINITE), (name, status)
        assert lib.sf_status() == bs.SF_EDOM and lib.sf_status() == 0, name


def test_recovered_excursions_on_the_other_paths(bg, wall):
    """The recovered lanes (rkf, adaptive) through ``solve_eom_batch_device``, ``state_at_efolds``, ``solve_eom_sampled`` and ``stochastic_efolds`` without
    noise or a bound on the step: under "nan" the word reads SF_EDOM after each, under "raise" none raises and the word is clear."""
    init, pars = bs.wall_lanes(bs.WALL_RECOVERED["rkf"])
    x, v = init[:, :2], init[:, 2:]
    lib = _handle(bg, wall)
    n_far = 0.05  # H ~ 80: t ~ 6e-4, past the turning point at t ~ 1e-4 near which the trial steps cross phi = 0
    calls = {
        "device": lambda: bg.solve_eom_batch_device(wall, pars, bs.WALL_ROWS, x, v, bs.WALL_MAX_ERR, "rkf").status,
        "efolds": lambda: bg.state_at_efolds(wall, pars, x, v, n_far, 2000, bs.WALL_MAX_ERR, "rkf", stop_at_end=False).status,
        "sampled": lambda: bg.solve_eom_sampled(wall, pars, [n_far], x, v, 2000, bs.WALL_MAX_ERR, "rkf", stop_at_end=False).status,
        "stochastic": lambda: bg.stochastic_efolds(wall, pars, x, v, 2, noise_scale=0.0, dN_max=math.inf, N_stop=n_far, max_steps=2000, max_err=bs.WALL_MAX_ERR, solver="rkf").counts[:, NONFINITE],
    }
    for name, call in calls.items():
        bg.set_sf_errors(wall, "nan")
        first = np.asarray(call())
        assert lib.sf_status() == bs.SF_EDOM and lib.sf_status() == 0, name
        bg.set_sf_errors(wall, "raise")
        assert np.array_equal(np.asarray(call()), first), name
        assert lib.sf_status() == 0, name
    assert np.all(first == 0)  # (the last call's: no realisation NONFINITE)


def test_efolds_map_with_a_line_outside_the_domain(bg, wall, sf_error):
    """A 16 x 16 grid of ``j52_wall`` with c = -3, b = 0.05 -- V rises with phi, the field rolls towards phi = 0 from rest and
    inflation ends before it gets there -- whose first line, phi = -0.025, lies outside the domain.  Under "raise" the map raises.
    Under "nan" it returns: NaN and NONFINITE on that line, and everywhere the values and statuses of ``solve_eom_batch`` on the same
    states, finite from the third line (phi = 0.03125) on."""
    art_host = bt.host_artifact("j52_wall")
    p = np.zeros(3)
    for name, value in (("a", 1.0), ("b", 0.05), ("c", -3.0)):
        p[int(art_host.symbol_dictionary[name][5:-1])] = value
    ss = [[-0.025, 0.425], [-1.0, 1.0]]
    lib = _handle(bg, wall)
    with pytest.raises(sf_error, match="ERRCODE 0X1"):
        bg.efolds_map(wall, p, ss, 16, 16, max_steps=20_000)
    bg.set_sf_errors(wall, "nan")
    nend, status = bg.efolds_map(wall, p, ss, 16, 16, max_steps=20_000, return_status=True)
    assert lib.sf_status() == bs.SF_EDOM and lib.sf_status() == 0
    x0, x1 = bg.grid_points(np.array(ss), 16, 16)
    assert x0[0] < 0.0 < x0[1] and x0[2] > 0.03
    assert np.isnan(nend[0]).all() and np.all(status[0] == NONFINITE)
    assert np.isfinite(nend[2:]).all() and np.all(status[2:] == ENDED) and np.all(nend[2:] > 0.0)
    X = np.stack([np.repeat(x0, 16), np.tile(x1, 16)], axis=1)
    sol = bg.solve_eom_batch(wall, p, 20_001, X[16:], np.zeros_like(X[16:]), 1e-8, stop_at_end=True)
    want = np.where(sol.status == ENDED, sol.N_end, np.nan).reshape(15, 16)
    assert np.array_equal(nend[1:], want, equal_nan=True) and np.array_equal(status[1:].reshape(-1), sol.status)


@pytest.mark.parametrize("name", MODELS)
def test_states_outside_the_domain(bg, sf_error, name):
    """``kinematics`` and ``masses`` at 65 states of which one lies outside the domain (``bessel_skew``: x = -1.5, K_nu(x + 1);
    ``kummer_curved``: y = 3.5, 2F1 at z = 7/6), which pins today's behaviour.  Under "nan": NaN there in every quantity that the
    potential enters -- eta_par, omega, V_sigma, V_N; V_TT, V_TN, V_NN, omega, M_eff2, mu_s2 -- and the host twin's value in those it
    does not (eps_H, sigma_dot and the Ricci scalar: velocities, H and the metric alone), the other states' values unchanged, and
    ``sf_status()`` = SF_EDOM; both raise ERRCODE 0X1 under "raise".  These evaluate given states: any bit fails the call."""
    art = bt.device_artifact(name)
    states, pars = (np.array(a[: bs.STATES]) for a in kr.zoo_states(name))
    good_k, good_m = np.stack(bg.kinematics(art, pars, states)), np.stack(bg.masses(art, pars, states))
    bad = 64
    states[bad, :2] = (-1.5, 0.2) if name == "bessel_skew" else (1.0, 3.5)
    lib = _handle(bg, art)
    lib.sf_status()
    try:
        host = bt.host_artifact(name)
        twins = (kr.KinematicsTwin(host).kinematics(pars, states)[:, bad], mr.MassesTwin(host).masses(pars, states)[:, bad])
        nans = ([1, 2, 4, 5], [0, 1, 2, 5, 6, 7])
        for fn, good, twin, nan in zip((bg.kinematics, bg.masses), (good_k, good_m), twins, nans):
            bg.set_sf_errors(art, "raise")
            with pytest.raises(sf_error, match="ERRCODE 0X1") as caught:
                fn(art, pars, states)
            assert "Those points hold NaN" in str(caught.value)
            assert lib.sf_status() == 0
            bg.set_sf_errors(art, "nan")
            got = np.stack(fn(art, pars, states))
            assert np.array_equal(np.flatnonzero(np.isnan(got[:, bad])), nan) and np.array_equal(np.isnan(twin), np.isnan(got[:, bad]))
            finite = ~np.isnan(twin)
            assert np.all(np.abs(got[finite, bad] - twin[finite]) <= 1e-10 * np.abs(twin[finite]))
            assert np.array_equal(got[:, :bad], good[:, :bad])
            assert lib.sf_status() == bs.SF_EDOM and lib.sf_status() == 0
    finally:
        bg.set_sf_errors(art, "raise")
        lib.sf_status()


if __name__ == "__main__":
    # the worst ratio to each bar on the device, into profiles/background_special.json under "gpu"
    import json
    import os
    import sys

    rc = pytest.main([__file__, "-q", "-s", "-p", "no:cacheprovider", *sys.argv[1:]])
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "background_special.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["gpu"] = sys.modules["test_background_special_gpu"].RATIOS if "test_background_special_gpu" in sys.modules else RATIOS
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    sys.exit(rc)
