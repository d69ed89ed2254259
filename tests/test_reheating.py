"""Reheating without a GPU (inflatox_amd.reheating, csrc/inflx_reheating.h): the host build of the lane code against a restatement of
its event rule, the exact checks (Gamma = 0 is the plain stepper; the Killing momentum; the constraint; the identities of A_shift), an
independent truth with a terminal event and at a fixed time, every stop status, the argument checks as one literal table, the public
surface, the twin under sanitizers and the cross-compiled object.

The bounds that come from a measurement are twice the worst figure of the host build (contraction off), taken when the tests were
written and recorded in profiles/reheating.json; every test prints its figure before it asserts."""

import inspect
import math
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import background_truth as bt
import reheating_reference as rr
import workloads
from background_reference import COMPLETE, NONFINITE, REJECTED, UNDERFLOW, BackgroundTwin, wall_artifact
from inflatox_amd import background as bg
from inflatox_amd import reheating as rh
from inflatox_amd._native import InflatoxShapeError
from inflatox_amd.compiler import CompilationArtifact
from reheating_reference import REHEATED, RULE_TOL, ReheatingTwin
from test_background_gpu import _hyper_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("rk4", "rkf")

#: located states against the truth at max_err = 1e-9 (``reheating_reference.located_error``): twice the host build's worst over the
#: 65 lanes -- hyperbolic: over Gamma = 0.2 and 1.0 (3.45e-7 rk4, 3.05e-6 rkf); fuzz4: 3.65e-8 rk4, 1.12e-7 rkf
LOCATED_BOUND = {("hyperbolic", "rk4"): 6.9e-7, ("hyperbolic", "rkf"): 6.1e-6, ("fuzz4", "rk4"): 7.3e-8, ("fuzz4", "rkf"): 2.3e-7}
#: rkf at max_err = 1e-10 on the 65 hyperbolic lanes, Gamma = 0.2 and 1.0: twice the worst relative drift of G_theta,theta chi^theta
#: exp(3 N + Gamma t) (4.14e-7) and of |3 H^2 - V - G chi chi / 2 - rho_r| / 3 H^2 (3.31e-8) over every accepted step
KILLING_BOUND, CONSTRAINT_BOUND = 8.3e-7, 6.7e-8
#: the models of the order test: ``background_truth.BATCH_DRAW``'s three conditions hold on all 65 lanes with Gamma on (fuzz0 and fuzz2
#: miss them: an error at n = 40 of 1.0e-10 and a ratio of 12.9); skew and shear have G_01 != 0
ORDER_MODELS = ("skew", "shear", "fuzz4")


@pytest.fixture(scope="module")
def hyper():
    art, p, _rhs = rr.hyper_case()
    return art, p, ReheatingTwin(art)


def order_gammas(name, lanes=rr.LANES):
    """the decay rate of every lane of the order test: seeded, in [0.2, 1]"""
    return np.random.default_rng(5 + sum(map(ord, name))).uniform(0.2, 1.0, lanes)


def order_truths(name, lanes=rr.LANES):
    return _order_truths(name, lanes)


_ORDER_CACHE = {}


def _order_truths(name, lanes):
    """the truth's y (7,) at T = 1 of the first lanes of ``background_truth.batch(name)`` with ``order_gammas``: computed once"""
    if (name, lanes) not in _ORDER_CACHE:
        init, pars = bt.batch(name)
        eom, gam = bt.truth_rhs(name), order_gammas(name, lanes)
        _ORDER_CACHE[name, lanes] = np.array([rr.truth_reheating(bt.bound(eom, pars[k]), init[k], gam[k], t_end=bt.T_ORDER)[0] for k in range(lanes)])
    return _ORDER_CACHE[name, lanes]


#: the components of the order test: all seven, and those a COMPLETE lane returns through ``inflatox_amd.reheating`` (not N)
ALL_COMPONENTS, RETURNED_COMPONENTS = (0, 1, 2, 3, 4, 5, 6), (0, 1, 2, 3, 4, 6)


def order_conditions(solve, name, lanes=rr.LANES, cols=ALL_COMPONENTS):
    """``background_truth.order_ratios`` on the components ``cols`` of the seven: (errors at n = 40, ratios n = 20 -> 40, the smallest
    H met) of the state after n steps of T / n against the truth; ``solve(n)`` returns (lanes, 7)"""
    truth = order_truths(name, lanes)
    errs, h_min = np.empty((2, lanes)), math.inf
    for i, n in enumerate((20, 40)):
        end = solve(n)
        errs[i] = np.max(np.abs(end[:, cols] - truth[:, cols]), axis=1)
        h_min = min(h_min, float(end[:, 4].min()))
    return errs[1], errs[0] / errs[1], h_min


# ---- the twin and the restatement of its rule ------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_twin_against_the_restated_rule(hyper, method):
    """The 65 hyperbolic end states, Gamma = 0.2 and 1.0, adaptive and at dt = 0.01, plus a lane whose radiation dominates at the start
    and a Gamma = 0 lane that runs out of steps: the same status, and every value of the returned state within RULE_TOL of its scale."""
    _art, p, twin = hyper
    ends = rr.hyper_end_states()
    worst = 0.0
    for gamma in rr.HYPER_GAMMAS:
        for dt in (None, 0.01):
            for k in range(rr.LANES):
                got, meta = twin.solve(p, ends[k], gamma, 20_000, method=method, dt=dt)
                want, status = rr.restated_reheating(twin, p, ends[k], gamma, 20_000, method=method, dt=dt)
                assert meta["status"] == status == REHEATED, (k, meta)
                worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-3))))
    for kw in (dict(gamma=0.5, rho_r0=1e3), dict(gamma=0.0, max_steps=30)):
        kw.setdefault("max_steps", 100)
        got, meta = twin.solve(p, ends[0], method=method, **kw)
        want, status = rr.restated_reheating(twin, p, ends[0], method=method, **kw)
        assert meta["status"] == status == (REHEATED if kw["gamma"] else COMPLETE)
        worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-3))))
    print(f"{method}: twin against the restated rule, worst {worst:.3e}")
    assert worst <= RULE_TOL, worst


@pytest.mark.parametrize("method", METHODS)
def test_without_decay_it_is_the_plain_stepper(hyper, method):
    """Gamma = 0 and rho_r0 = 0 at dt = 0.01: phi, chi, H, N and t of every accepted step equal ``BackgroundTwin``'s rows to 1e-12 of
    their scale, and rho_r stays 0."""
    art, p, twin = hyper
    plain = BackgroundTwin(art)
    x, v = _hyper_batch(8)
    worst = 0.0
    for k in range(8):
        init = np.concatenate([x[k], v[k]])
        want, _ = plain.solve(p, init, 41, method=method, dt=0.01)
        _, meta = twin.solve(p, init, 0.0, 40, method=method, dt=0.01, rows=64)
        rows = meta["rows"]
        assert meta["status"] == COMPLETE and meta["accepted"] == 40 and np.all(rows[:, 6] == 0.0)
        worst = max(worst, float(np.max(np.abs(rows[:, :6] - want[:, :6]) / np.maximum(np.abs(want[:, :6]), 1e-3))), float(np.max(np.abs(rows[:, 14] - want[:, 6]))))
    print(f"{method}: Gamma = 0 against the plain stepper, worst {worst:.3e}")
    assert worst <= 1e-12


def test_killing_momentum_and_constraint(hyper):
    """The hyperbolic potential does not depend on theta, so G_theta,theta chi^theta decays as exp(-3 N - Gamma t) exactly: the check
    of the decay term.  The constraint 3 H^2 = V + G chi chi / 2 + rho_r is not imposed after the start and holds along the flow."""
    _art, p, twin = hyper
    ends = rr.hyper_end_states()
    L = p[2]
    killing = constraint = 0.0
    for gamma in rr.HYPER_GAMMAS:
        for k in range(rr.LANES):
            _, meta = twin.solve(p, ends[k], gamma, 100_000, max_err=1e-10, rows=20_000)
            y, t = meta["rows"][:, :7], meta["rows"][:, 14]
            assert meta["status"] == REHEATED
            j = L**2 * np.sinh(y[:, 0] / L) ** 2 * y[:, 3] * np.exp(3.0 * y[:, 5] + gamma * t)
            killing = max(killing, float(np.max(np.abs(j / j[0] - 1.0))))
            e = twin.eom(p, y[:, :4])
            constraint = max(constraint, float(np.max(np.abs(3.0 * y[:, 4] ** 2 - e[:, 2] - 0.5 * e[:, 3] - y[:, 6]) / (3.0 * y[:, 4] ** 2))))
    print(f"Killing momentum over exp(-3 N - Gamma t): worst drift {killing:.3e} (bound {KILLING_BOUND:.1e}); constraint {constraint:.3e} (bound {CONSTRAINT_BOUND:.1e})")
    assert killing <= KILLING_BOUND and constraint <= CONSTRAINT_BOUND


def _as_result(outs, metas):
    """``inflatox_amd.reheating._result`` on twin runs: the module's own arithmetic on the states the twin returned"""
    states = np.array([o[:7] for o in outs])
    return rh._result(states, np.array([o[7] for o in outs]), np.array([m["H0"] for m in metas]), np.array([m["status"] for m in metas], dtype=np.int8))


def test_a_shift_and_offset_identities(hyper):
    """A_shift = (1 - 3 w) N_reh / 4 to 1e-12, and ``offset_from_reheating`` equals ``reheating_offset(w_reh=w, N_reh=N_reh)`` to 1e-12 on
    the lanes whose w lies in reheating_offset's range; the members against ``reheating_reference.figures``."""
    _art, p, twin = hyper
    ends = rr.hyper_end_states()
    runs = [twin.solve(p, ends[k], gamma, 100_000) for gamma in rr.HYPER_GAMMAS for k in range(rr.LANES)]
    runs.append(twin.solve(p, ends[0], 0.5, 100, rho_r0=1e3))  # reheated at the start
    runs.append(twin.solve(p, ends[0], 0.0, 30))  # never
    reh = _as_result([o for o, _ in runs], [m for _, m in runs])
    assert isinstance(reh, rh.Reheating) and reh.state.shape == (len(runs), 5) and reh.status.dtype == np.int8
    hit = reh.status == REHEATED
    assert hit[:-1].all() and not hit[-1] and reh.N_reh[-2] == 0.0 and np.isnan(reh.w_reh[-2]) and reh.A_shift[-2] == 0.0
    assert np.isnan([reh.N_reh[-1], reh.w_reh[-1], reh.A_shift[-1]]).all() and np.isfinite(reh.state[-1]).all() and reh.rho_r[-1] == 0.0
    for k, (o, m) in enumerate(runs):
        want = rr.figures(o, m["H0"], m["status"])
        assert np.allclose([reh.N_reh[k], reh.w_reh[k], reh.A_shift[k]], want, rtol=1e-14, atol=0.0, equal_nan=True), k
    ok = hit & np.isfinite(reh.w_reh)
    from_w = (1.0 - 3.0 * reh.w_reh[ok]) * reh.N_reh[ok] / 4.0
    print(f"A_shift against (1 - 3 w) N_reh / 4: worst {np.max(np.abs(reh.A_shift[ok] - from_w)):.3e}; w_reh in [{reh.w_reh[ok].min():.4f}, {reh.w_reh[ok].max():.4f}]")
    assert np.max(np.abs(reh.A_shift[ok] - from_w)) <= 1e-12
    assert np.max(np.abs(reh.omega_r[hit][:-1] - rr.HYPER_OMEGA)) <= 1e-12
    offset = rh.offset_from_reheating(reh)
    assert np.array_equal(np.isnan(offset), ~hit) and offset[-2] == bg.reheating_offset()
    inside = np.flatnonzero(ok & (reh.w_reh > -1.0 / 3.0) & (reh.w_reh <= 1.0))
    assert inside.size >= 100
    want = np.array([bg.reheating_offset(w_reh=reh.w_reh[k], N_reh=reh.N_reh[k]) for k in inside])
    assert np.max(np.abs(offset[inside] - want)) <= 1e-12
    other = rh.offset_from_reheating(reh, 0.002, g_reh=10.75, gs_reh=10.75)
    assert np.allclose(other[inside] - offset[inside], bg.reheating_offset(0.002, g_reh=10.75, gs_reh=10.75) - bg.reheating_offset(), rtol=0.0, atol=1e-12)


# ---- the independent truth -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_located_states_against_the_truth(hyper, method):
    """(a) The 65 hyperbolic end states at Gamma = 0.2 and 1.0, omega_r = 0.99, and the 65 lanes of fuzz4 at Gamma = 0.5, omega_r =
    0.002, max_err = 1e-9: the truth crosses on every lane, every lane is REHEATED, and N_reh, ln H_reh and the state are within
    LOCATED_BOUND of the truth's state at its own event."""
    _art, p, twin = hyper
    ends = rr.hyper_end_states()
    worst = 0.0
    for gamma in rr.HYPER_GAMMAS:
        truth = rr.hyper_truths(gamma)
        assert all(tr is not None and tr[1] > 0.0 for tr in truth)
        for k in range(rr.LANES):
            out, meta = twin.solve(p, ends[k], gamma, 100_000, omega_r=rr.HYPER_OMEGA, method=method, max_err=1e-9)
            assert meta["status"] == REHEATED, (gamma, k, meta)
            worst = max(worst, rr.located_error(out, truth[k]))
    print(f"hyperbolic {method}: located states against the truth, worst {worst:.3e} (bound {LOCATED_BOUND['hyperbolic', method]:.1e})")
    assert worst <= LOCATED_BOUND["hyperbolic", method]
    init, pars = bt.batch(rr.FUZZ_NAME)
    truth = rr.fuzz_truths()
    assert all(tr is not None and 0.0 < tr[1] < 0.5 for tr in truth)
    ftwin = ReheatingTwin(bt.host_artifact(rr.FUZZ_NAME))
    worst = 0.0
    for k in range(rr.LANES):
        out, meta = ftwin.solve(pars[k], init[k], rr.FUZZ_GAMMA, 100_000, omega_r=rr.FUZZ_OMEGA, method=method, max_err=1e-9)
        assert meta["status"] == REHEATED, (k, meta)
        worst = max(worst, rr.located_error(out, truth[k]))
    print(f"fuzz4 {method}: located states against the truth, worst {worst:.3e} (bound {LOCATED_BOUND['fuzz4', method]:.1e})")
    assert worst <= LOCATED_BOUND["fuzz4", method]


@pytest.mark.parametrize("name", ORDER_MODELS)
def test_fourth_order_without_the_event(name):
    """(b) Fixed dt to T = 1, Gamma per lane in [0.2, 1], no lane reheats (COMPLETE): the returned state against the truth at T.  Both
    steppers are of fourth order lane by lane under ``background_truth.BATCH_DRAW``'s conditions: the error at n = 40 above 1.2e-10, the
    ratio n = 20 -> 40 at least 14.5, H > 0.05."""
    init, pars = bt.batch(name)
    twin = ReheatingTwin(bt.host_artifact(name))
    gam = order_gammas(name)
    for method in METHODS:

        ends = {}

        def solve(n):
            if n not in ends:
                runs = [twin.solve(pars[k], init[k], gam[k], n, method=method, dt=bt.T_ORDER / n) for k in range(rr.LANES)]
                assert all(m["status"] == COMPLETE and m["accepted"] == n for _, m in runs)
                ends[n] = np.array([o for o, _ in runs])
            return ends[n]

        for cols in (ALL_COMPONENTS, RETURNED_COMPONENTS):  # (the device test sees the second set: the conditions hold on it here first)
            err, ratio, h_min = order_conditions(solve, name, cols=cols)
            print(f"{name} {method} {cols}: error at n = 40 in [{err.min():.3e}, {err.max():.3e}], ratio in [{ratio.min():.2f}, {ratio.max():.2f}], H >= {h_min:.3f}")
            assert err.min() > 1.2e-10 and ratio.min() >= 14.5 and h_min > 0.05


# ---- stops -----------------------------------------------------------------------------------------------------------------------
def test_every_stop_status(hyper):
    """Gamma = 0 runs out of steps (COMPLETE) with the last state returned; a start whose radiation already has Omega_r >= omega_r is
    REHEATED there; on ``background_reference.wall_model`` (NaN for phi < 0) a lane on the wall is REJECTED adaptively and NONFINITE at a
    fixed dt, both with the state they started from, and one that runs at the wall is UNDERFLOW -- as in test_background_stops.py."""
    _art, p, twin = hyper
    end = rr.hyper_end_states()[3]
    for method in METHODS:
        out, meta = twin.solve(p, end, 0.0, 25, method=method)
        assert meta["status"] == COMPLETE and meta["accepted"] == 25 and out[6] == 0.0 and out[7] > 0.0 and np.isfinite(out).all()
        assert np.isnan(rr.figures(out, meta["H0"], meta["status"])).all()
        e = twin.eom(p, end[None])[0]
        rho = e[2] + 0.5 * e[3]
        for rho_r0, status in ((0.49 * rho, COMPLETE), (1.001 * rho, REHEATED), (10.0 * rho, REHEATED)):  # Omega_r = 0.329, 0.50025, 0.909 at the start
            out, meta = twin.solve(p, end, 0.0, 1, rho_r0=rho_r0, omega_r=0.5, method=method, dt=1e-6)
            assert meta["status"] == status, (rho_r0, meta)
            if status == REHEATED:
                assert meta["accepted"] == 0 and out[5] == 0.0 and out[7] == 0.0 and out[6] == rho_r0 and np.array_equal(out[:4], end)
                n, w, shift = rr.figures(out, meta["H0"], status)
                assert n == 0.0 and math.isnan(w) and shift == 0.0
    wall, wp = wall_artifact()
    wtwin = ReheatingTwin(wall)
    on_wall, toward = (0.0, 0.0, -1.0, 0.0), (1e-3, 0.0, -1.0, 0.0)
    for method in METHODS:
        out, meta = wtwin.solve(wp, on_wall, 0.5, 100, method=method)
        assert meta["status"] == REJECTED and meta["accepted"] == 0 and np.array_equal(out[:4], on_wall) and out[7] == 0.0
        out, meta = wtwin.solve(wp, on_wall, 0.5, 100, method=method, dt=1e-3)
        assert meta["status"] == NONFINITE and meta["accepted"] == 0 and np.array_equal(out[:4], on_wall)
        out, meta = wtwin.solve(wp, toward, 0.5, 2000, method=method)
        assert meta["status"] == UNDERFLOW and 0.0 < out[0] < 1e-3 and np.isfinite(out).all() and out[6] > 0.0
        for contract in ("off", "fast"):  # (the device contracts a*b+c: the statuses must not depend on it)
            assert ReheatingTwin(wall, contract=contract).solve(wp, toward, 0.5, 2000, method=method)[1]["status"] == UNDERFLOW


# ---- the argument checks: one literal table --------------------------------------------------------------------------------------
A = types.SimpleNamespace(n_fields=2, n_parameters=3)
A3 = types.SimpleNamespace(n_fields=3, n_parameters=3)
P = [1.0, 2.0, 3.0]
X = [[1.0, 2.0], [3.0, 4.0]]
V = [[0.0, 0.0], [0.0, 0.0]]
SS = [[0.0, 1.0], [2.0, 3.0]]
P13, P33, P63 = np.ones((1, 3)), np.ones((3, 3)), np.ones((6, 3))
FIELDS = "fields_init and derivatives_init must both have shape (B, 2) (got (2,) and (2, 2))"
START_STOP = "start_stop must be [[x0_start, x0_stop], [x1_start, x1_stop]] (got shape (2,))"

# fmt: off
CASES = [
    # ---- reheating: the common options, omega_r, fields, Gamma, rho_r_init, parameter rows -- in that order
    (lambda: rh.reheating(A3, P, 0.2, X, V), InflatoxShapeError, "the background solver requires a 2-field model (model has 3 fields)"),
    (lambda: rh.reheating(A, P, 0.2, X, V, max_steps=0), ValueError, "steps must be at least 1 (got 0)"),
    (lambda: rh.reheating(A, P, 0.2, X, V, max_steps=1.5), ValueError, "steps and substeps must be integers"),
    (lambda: rh.reheating(A, P, 0.2, X, V, max_err=0.0), ValueError, "max_err must be a positive finite number (got 0.0)"),
    (lambda: rh.reheating(A, P, 0.2, X, V, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),
    (lambda: rh.reheating(A, P, 0.2, X, V, dt=-1.0), ValueError, "dt must be None (adaptive) or a positive finite step (got -1.0)"),
    (lambda: rh.reheating(A, P, 0.2, X, V, omega_r="x"), ValueError, "omega_r must be a number"),
    (lambda: rh.reheating(A, P, 0.2, X, V, omega_r=0.0), ValueError, "omega_r must be in (0, 1) (got 0.0)"),
    (lambda: rh.reheating(A, P, 0.2, X, V, omega_r=1.0), ValueError, "omega_r must be in (0, 1) (got 1.0)"),
    (lambda: rh.reheating(A, P, 0.2, X, V, omega_r=math.nan), ValueError, "omega_r must be in (0, 1) (got nan)"),
    (lambda: rh.reheating(A, P, 0.2, [1.0, 2.0], V), InflatoxShapeError, FIELDS),
    (lambda: rh.reheating(A, P, 0.2, X, [[0.0, 0.0]]), InflatoxShapeError, "fields_init and derivatives_init must both have shape (B, 2) (got (2, 2) and (1, 2))"),
    (lambda: rh.reheating(A, P, "x", X, V), ValueError, "Gamma must be a number or an array of numbers"),
    (lambda: rh.reheating(A, P, [0.1, 0.2, 0.3], X, V), InflatoxShapeError, "Gamma must be a scalar or have shape (2,) (got (3,))"),
    (lambda: rh.reheating(A, P, -0.1, X, V), ValueError, "Gamma must be finite and >= 0"),
    (lambda: rh.reheating(A, P, [0.1, math.inf], X, V), ValueError, "Gamma must be finite and >= 0"),
    (lambda: rh.reheating(A, P, [0.1, math.nan], X, V), ValueError, "Gamma must be finite and >= 0"),
    (lambda: rh.reheating(A, P, 0.2, X, V, rho_r_init="x"), ValueError, "rho_r_init must be a number or an array of numbers"),
    (lambda: rh.reheating(A, P, 0.2, X, V, rho_r_init=[[0.0, 0.0]]), InflatoxShapeError, "rho_r_init must be a scalar or have shape (2,) (got (1, 2))"),
    (lambda: rh.reheating(A, P, 0.2, X, V, rho_r_init=-1.0), ValueError, "rho_r_init must be finite and >= 0"),
    (lambda: rh.reheating(A, [1.0, 2.0], 0.2, X, V), InflatoxShapeError, "model has 3 parameters (got 2)"),
    (lambda: rh.reheating(A, P33, 0.2, X, V), InflatoxShapeError, "pars must have shape (3,) or (2, 3) (got (3, 3))"),
    (lambda: rh.reheating(A, P, 0.2, X, V, omega_r=2.0, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),  # two faults: solver before omega_r
    (lambda: rh.reheating(A, P, 0.2, [1.0, 2.0], V, omega_r=2.0), ValueError, "omega_r must be in (0, 1) (got 2.0)"),  # two faults: omega_r before fields
    (lambda: rh.reheating(A, P, -0.1, [1.0, 2.0], V), InflatoxShapeError, FIELDS),  # two faults: fields before Gamma
    (lambda: rh.reheating(A, P, -0.1, X, V, rho_r_init=-1.0), ValueError, "Gamma must be finite and >= 0"),  # two faults: Gamma before rho_r_init
    (lambda: rh.reheating(A, P33, 0.2, X, V, rho_r_init=-1.0), ValueError, "rho_r_init must be finite and >= 0"),  # two faults: rho_r_init before pars
    # ---- reheating_map: the common options, omega_r, the grid, Gamma (N0, N1), one parameter row
    (lambda: rh.reheating_map(A3, P, 0.2, SS, 3, 2), InflatoxShapeError, "the background solver requires a 2-field model (model has 3 fields)"),
    (lambda: rh.reheating_map(A, P, 0.2, SS, 3, 2, max_steps=0), ValueError, "steps must be at least 1 (got 0)"),
    (lambda: rh.reheating_map(A, P, 0.2, SS, 3, 2, omega_r=-0.5), ValueError, "omega_r must be in (0, 1) (got -0.5)"),
    (lambda: rh.reheating_map(A, P, 0.2, [0.0, 1.0], 3, 2), InflatoxShapeError, START_STOP),
    (lambda: rh.reheating_map(A, P, 0.2, SS, 0, 2), ValueError, "the grid needs at least one point per axis (got 0 x 2)"),
    (lambda: rh.reheating_map(A, P, 0.2, SS, 1.5, 2), TypeError, "'float' object cannot be interpreted as an integer"),
    (lambda: rh.reheating_map(A, P, 0.2, SS, 3, 2, derivatives_init=(0.0,)), InflatoxShapeError, "derivatives_init must hold two velocities (got 1)"),
    (lambda: rh.reheating_map(A, P, "x", SS, 3, 2), ValueError, "Gamma must be a number or an array of numbers"),
    (lambda: rh.reheating_map(A, P, np.ones(6), SS, 3, 2), InflatoxShapeError, "Gamma must be a scalar or have shape (3, 2) (got (6,))"),
    (lambda: rh.reheating_map(A, P, np.full((3, 2), -1.0), SS, 3, 2), ValueError, "Gamma must be finite and >= 0"),
    (lambda: rh.reheating_map(A, P63, 0.2, SS, 3, 2), InflatoxShapeError, "pars must have shape (3,) or (1, 3) (got (6, 3))"),
    (lambda: rh.reheating_map(A, P13, 0.2, SS, 3, 2), InflatoxShapeError, "the reheating maps take one parameter row"),
    (lambda: rh.reheating_map(A, P, 0.2, [0.0, 1.0], 3, 2, omega_r=2.0), ValueError, "omega_r must be in (0, 1) (got 2.0)"),  # two faults: omega_r before start_stop
    (lambda: rh.reheating_map(A, P, 0.2, [0.0, 1.0], 0, 2), InflatoxShapeError, START_STOP),  # two faults: start_stop before N0
    (lambda: rh.reheating_map(A, P, -1.0, SS, 3, 2, derivatives_init=(0.0,)), InflatoxShapeError, "derivatives_init must hold two velocities (got 1)"),  # two faults: derivatives_init before Gamma
    (lambda: rh.reheating_map(A, P13, -1.0, SS, 3, 2), ValueError, "Gamma must be finite and >= 0"),  # two faults: Gamma before the parameter row
    # ---- pivot_observables_map_reheated: k_mpc and the degrees of freedom, N_sub, dlnk, then reheating_map's checks
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, 0.0), ValueError, "k_mpc must be finite and > 0 (got 0.0)"),
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, "x"), ValueError, "reheating_offset takes numbers"),
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, g_reh=-1.0), ValueError, "g_reh must be finite and > 0 (got -1.0)"),
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, gs_reh=math.inf), ValueError, "gs_reh must be finite and > 0 (got inf)"),
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, N_sub=0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, dlnk=0.0), ValueError, "dlnk must be finite and > 0 (got 0.0)"),
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, solver="euler"), ValueError, "unknown solver 'euler': choose 'rk4' or 'rkf'"),
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, omega_r=1.5), ValueError, "omega_r must be in (0, 1) (got 1.5)"),
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 0), ValueError, "the grid needs at least one point per axis (got 3 x 0)"),
    (lambda: rh.pivot_observables_map_reheated(A, P, np.ones((2, 3)), SS, 3, 2), InflatoxShapeError, "Gamma must be a scalar or have shape (3, 2) (got (2, 3))"),
    (lambda: rh.pivot_observables_map_reheated(A, P13, 0.2, SS, 3, 2), InflatoxShapeError, "the reheating maps take one parameter row"),
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, 0.0, N_sub=0.0), ValueError, "k_mpc must be finite and > 0 (got 0.0)"),  # two faults: k_mpc before N_sub
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, N_sub=0.0, dlnk=0.0), ValueError, "N_sub must be finite and > 0 (got 0.0)"),  # two faults: N_sub before dlnk
    (lambda: rh.pivot_observables_map_reheated(A, P, 0.2, SS, 3, 2, dlnk=0.0, solver="euler"), ValueError, "dlnk must be finite and > 0 (got 0.0)"),  # two faults: dlnk before solver
    (lambda: rh.pivot_observables_map_reheated(A, P, -1.0, [0.0, 1.0], 3, 2), InflatoxShapeError, START_STOP),  # two faults: start_stop before Gamma
    # ---- offset_from_reheating: reheating_offset's own checks
    (lambda: rh.offset_from_reheating(rh.Reheating(*[np.zeros(1)] * 9), -1.0), ValueError, "k_mpc must be finite and > 0 (got -1.0)"),
    (lambda: rh.offset_from_reheating(rh.Reheating(*[np.zeros(1)] * 9), g_reh=0.0), ValueError, "g_reh must be finite and > 0 (got 0.0)"),
]
# fmt: on


def _called(case):
    return next(name for name in case[0].__code__.co_names if name in rh.__all__ and name != "Reheating")


@pytest.fixture
def no_device(monkeypatch):
    def touched(*args, **kwargs):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(bg, "_dylib", touched)
    monkeypatch.setattr(bg, "_crossing_dylib", touched)
    monkeypatch.setattr(rh, "_reheating_dylib", touched)
    assert callable(CompilationArtifact.ensure_reheating)
    for name in dir(CompilationArtifact):
        if name.startswith("ensure_"):
            monkeypatch.setattr(CompilationArtifact, name, touched)
    return touched


@pytest.mark.parametrize("case", range(len(CASES)), ids=lambda i: f"{i}-{_called(CASES[i])}")
def test_bad_arguments(no_device, case):
    call, error, message = CASES[case]
    with pytest.raises(error) as caught:
        call()
    assert type(caught.value) is error and str(caught.value) == message


def test_every_checking_function_is_in_the_table():
    """Every function of ``reheating.__all__`` that takes an artefact, and the pure function that checks its arguments."""
    checking = {name for name in rh.__all__ if inspect.isfunction(getattr(rh, name)) and "artifact" in inspect.signature(getattr(rh, name)).parameters}
    assert checking == {"reheating", "reheating_map", "pivot_observables_map_reheated"}
    checking |= {"offset_from_reheating"}
    assert checking <= {_called(case) for case in CASES}, checking - {_called(case) for case in CASES}


def test_good_arguments_reach_the_device(no_device):
    art = types.SimpleNamespace(n_fields=2, n_parameters=3, **{name: no_device for name in dir(CompilationArtifact) if name.startswith("ensure_")})
    for call in (lambda: rh.reheating(art, P, 0.2, X, V), lambda: rh.reheating(art, np.ones((2, 3)), [0.0, 1.0], X, V, rho_r_init=[0.0, 2.0], omega_r=0.5, dt=0.1),
                 lambda: rh.reheating_map(art, P, np.ones((3, 2)), SS, 3, 2), lambda: rh.pivot_observables_map_reheated(art, P, 0.2, SS, 3, 2, 0.002)):  # fmt: skip
        with pytest.raises(AssertionError, match="the device was touched"):
            call()


# ---- the surface -----------------------------------------------------------------------------------------------------------------
BACKGROUND_ALL = ["solve_eom", "solve_eom_batch", "solve_eom_batch_device", "efolds_map", "state_at_efolds", "horizon_exit_map", "solve_eom_sampled", "EoMSolution", "EfoldsState",
                  "SampledSolution", "STATUS", "kinematics", "turn_rate_map", "Kinematics", "masses", "mass_map", "Masses", "transfer_functions", "transfer_map",
                  "TransferSolution", "power_spectra", "spectrum_map", "PowerSpectra", "tensor_spectra", "TensorSpectra", "observables", "Observables", "observables_map",
                  "delta_N", "DeltaN", "fnl_map", "delta_N_status", "spectra_evolution", "SpectraEvolution", "evolution_map", "transfer_from_spectra",
                  "stochastic_efolds", "stochastic_map", "StochasticEfolds", "stochastic_distribution", "stochastic_distribution_map", "StochasticDistribution",
                  "distribution_pdf", "distribution_survival", "distribution_mean", "distribution_tail_rate", "horizon_crossings", "CrossingSolution", "inflation_end",
                  "InflationEnd", "power_spectra_at_k", "tensor_spectra_at_k", "ExitPoints", "observables_at_k", "reheating_offset", "pivot_exit_map",
                  "pivot_observables_map", "OUTSIDE_AT_START", "set_sf_errors"]  # fmt: skip


def test_public_names_and_unchanged_surface():
    import ctypes

    import inflatox_amd
    import inflatox_amd.compiler as compiler
    from inflatox_amd import _native

    assert rh.__all__ == ["reheating", "reheating_map", "offset_from_reheating", "pivot_observables_map_reheated", "Reheating", "REHEATED", "STATUS"]
    assert rh.REHEATED == 10 and set(rh.STATUS) == set(bg.STATUS) | {10} and all(rh.STATUS[k] == v for k, v in bg.STATUS.items())
    assert bg.__all__ == BACKGROUND_ALL and sorted(bg.STATUS) == list(range(10)) and "reheating" not in inflatox_amd.__all__
    assert rh.Reheating._fields == ("state", "rho_r", "N_reh", "t_reh", "H_start", "w_reh", "A_shift", "omega_r", "status")
    keyword = inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(rh.reheating)
    assert list(sig.parameters) == ["artifact", "pars", "Gamma", "fields_init", "derivatives_init", "omega_r", "rho_r_init", "max_steps", "max_err", "solver", "dt"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[5:]] == [0.99, 0.0, 100_000, 1e-8, "rkf", None] and all(sig.parameters[n].kind is keyword for n in list(sig.parameters)[5:])
    sig = inspect.signature(rh.reheating_map)
    assert list(sig.parameters)[:7] == ["artifact", "pars", "Gamma", "start_stop", "N0", "N1", "derivatives_init"] and sig.parameters["derivatives_init"].kind is keyword
    assert tuple(sig.parameters["derivatives_init"].default) == (0, 0) and sig.parameters["omega_r"].default == 0.99
    sig = inspect.signature(rh.offset_from_reheating)
    assert list(sig.parameters) == ["reh", "k_mpc", "g_reh", "gs_reh"] and [q.default for q in list(sig.parameters.values())[1:]] == [0.05, 106.75, 106.75]
    assert sig.parameters["g_reh"].kind is keyword
    sig = inspect.signature(rh.pivot_observables_map_reheated)
    assert list(sig.parameters) == ["artifact", "pars", "Gamma", "start_stop", "N0", "N1", "k_mpc", "g_reh", "gs_reh", "omega_r", "dlnk", "N_sub", "derivatives_init", "max_steps",
                                    "max_err", "solver", "return_status"]  # fmt: skip
    assert sig.parameters["k_mpc"].default == 0.05 and sig.parameters["return_status"].default is False and all(sig.parameters[n].kind is keyword for n in list(sig.parameters)[7:])
    for helper in ("_check_common", "_pars", "_check_fields", "_check_grid", "_parameter_row", "_grid_init", "_second_stage"):
        assert getattr(rh, helper) is getattr(bg, helper), helper  # imported, not copied
    # the twelfth companion object
    new = ("inflx_reheating_kernels.hip", "inflx_reheating.h", "inflx_reheating_abi.h")
    assert compiler._REHEATING_SOURCES == (*new, "inflx_deltan.h", "inflx_background.h", "inflx_background_abi.h")
    csrc = os.path.join(ROOT, "inflatox_amd", "csrc")
    assert all(os.path.exists(os.path.join(csrc, f)) for f in compiler._REHEATING_SOURCES)
    for name, sources in vars(compiler).items():
        if name.endswith("_SOURCES") and name != "_REHEATING_SOURCES":
            assert not set(sources) & set(new), name  # no other object is built from the new files: every existing object keeps its hash
    assert callable(CompilationArtifact.ensure_reheating) and "reheating" not in compiler.KERNEL_GROUPS
    text = open(os.path.join(csrc, "inflx_reheating.h")).read()
    declared = set(re.findall(r"^INFLX_FN \w+ (inflx_rh_\w+)\(", text, flags=re.M))
    assert declared == {"inflx_rh_rhs", "inflx_rh_finite7", "inflx_rh_event", "inflx_rh_init", "inflx_rh_resume", "inflx_rh_rk4", "inflx_rh_rkf", "inflx_rh_norm",
                        "inflx_rh_trial", "inflx_rh_step_taken", "inflx_rh_dense_event", "inflx_rh_locate", "inflx_rh_step"}  # fmt: skip
    assert re.search(r"INFLX_RH_REHEATED = 10\b", text) and all(f"{name}(" in text for name in ("inflx_bg_factor", "inflx_bg_hermite"))
    assert re.search(r"#define INFLX_RH_ABI_VERSION 1\b", open(os.path.join(csrc, "inflx_reheating_abi.h")).read())
    assert "asm" not in open(os.path.join(csrc, "inflx_reheating_kernels.hip")).read()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inflx_hip_reheating.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(inflx_[a-z_0-9]+)\s*\(", header))) == ["inflx_reheating"] and "INFLX_RH_STATUS_REHEATED = 10" in header
    assert '#include "inflx_hip_reheating.h"' in open(os.path.join(ROOT, "include", "inflx_hip.h")).read()
    assert list(_native.REHEATING_SIGNATURES) == ["inflx_reheating"] and len(_native.REHEATING_SIGNATURES["inflx_reheating"][1]) == 17
    others = (set(_native.SIGNATURES) | set(_native.DELTAN_SIGNATURES) | set(_native.EVOLUTION_SIGNATURES) | set(_native.STOCHASTIC_SIGNATURES)
              | set(_native.DISTRIBUTION_SIGNATURES) | set(_native.CROSSING_SIGNATURES))  # fmt: skip
    assert not set(_native.REHEATING_SIGNATURES) & others
    _native.build_library()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "inflx_reheating") and callable(_native.InflatoxDevLib.reheating)


def test_twin_program_under_address_and_ub_sanitizers(tmp_path, hyper):
    """tests/reheating_twin.cpp as a stand-alone program (REHEATING_TWIN_MAIN) under ASan + UBSan on the CPU: two lanes, one of them
    reheated at the start, both steppers, adaptive and at a fixed dt whose 40 steps run out."""
    gxx = shutil.which("g++")
    assert gxx is not None
    _art, p, twin = hyper
    exe = str(tmp_path / "reheating_twin")
    cmd = [gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DREHEATING_TWIN_MAIN",
           *ReheatingTwin.compile_options(*twin.headers), ReheatingTwin.SOURCES[-1], "-o", exe]  # fmt: skip
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe, *map(repr, p.tolist())], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 8, run.stdout[-3000:]
    first, second = lines[:4], lines[4:]
    assert all("fixed 0: status 10," in ln and "Omega_r 0.900000" in ln for ln in first[0::2]) and all("fixed 1: status 0, accepted 40, rows 41," in ln for ln in first[1::2])
    assert all("status 10, accepted 0, rows 1, N 0.000000" in ln for ln in second)


def test_cross_compiled_object(hyper):
    """``ensure_reheating()`` for the hyperbolic and the D5 artefact: a gfx950 code object beside the artefact with the three kernels and
    the layout word."""
    from inflatox_amd.compiler import hipcc_path

    tool = os.path.join(os.path.dirname(os.path.realpath(hipcc_path())), "..", "lib", "llvm", "bin", "llvm-readelf")
    if not os.path.exists(tool):
        tool = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    for name in ("hyperbolic", "d5"):
        _spec, art = workloads.artifact_for(name)
        path = art.ensure_reheating()
        assert path == art.shared_object_path + ".reheating" and os.path.getsize(path) > 0
        symbols = subprocess.run([tool, "--symbols", "--notes", path], capture_output=True, text=True, timeout=120).stdout
        for symbol in ("inflx_rh_init", "inflx_rh_advance_rk4", "inflx_rh_advance_rkf", "INFLX_RH_ABI", "VERSION", "MODEL_TAG"):
            assert re.search(rf"\s{symbol}\s*$", symbols, flags=re.M), (name, symbol)
        assert "gfx950" in symbols
