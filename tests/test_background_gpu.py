"""Background trajectories on the GPU (inflatox_amd.background): analytic and scipy solutions, convergence order, a conserved
momentum, the Friedmann constraint, determinism and lane independence, the end of inflation, stopped lanes, a special-function
model and the lifecycle of the background code object."""

import math
import os

import numpy as np
import pytest

import workloads
from background_reference import (
    COMPLETE,
    ENDED,
    NONFINITE,
    BackgroundTwin,
    Restatement,
    model_functions,
    power_law_artifact,
    power_law_exact,
    power_law_init,
    solve_ivp_reference,
)
from test_background import initial_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def power_law():
    return power_law_artifact()


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_power_law_attractor(bg, power_law, method):
    art, p = power_law
    x0 = power_law_init()
    sol = bg.solve_eom_batch(art, p, 400, [x0[:2]], [x0[2:]], max_err=1e-10, solver=method)
    assert sol.status[0] == COMPLETE and sol.last_row[0] == 399
    exact = power_law_exact(sol.t[0])
    got = np.concatenate([sol.states[0], sol.N[0][:, None]], axis=1)
    rel = np.abs(got - exact) / np.maximum(np.abs(exact), 1.0)
    assert rel.max() <= 1e-8, rel.max(axis=0)
    assert sol.t[0, -1] > 1e-2


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_convergence_order(bg, power_law, method):
    """Fixed dt to the same end time: halving dt cuts the end-point error by >= 14 (fourth order: 16)."""
    art, p = power_law
    x0 = power_law_init()
    T, errs = 2.0, []
    for n in (40, 80):
        sol = bg.solve_eom_batch(art, p, n + 1, [x0[:2]], [x0[2:]], solver=method, dt=T / n)
        end = np.concatenate([sol.states[0, -1], [sol.N[0, -1]]])
        errs.append(np.max(np.abs(end - power_law_exact(sol.t[0, -1]))))
    assert errs[0] / errs[1] >= 14.0, errs


def test_killing_momentum_is_conserved(bg):
    """Hyperbolic: V depends on phi only, so J = a^3 L^2 sinh^2(phi/L) thetadot = e^(3N) L^2 sinh^2(phi/L) thetadot is conserved."""
    spec, art = workloads.artifact_for("hyperbolic")
    L = spec.args[2]
    sol = bg.solve_eom_batch(art, spec.args, 300, [[3.0, 0.5]], [[0.0, 0.3]], max_err=1e-12, solver="rkf", substeps=4)
    assert sol.status[0] == COMPLETE
    phi, thetadot, N = sol.states[0, :, 0], sol.states[0, :, 3], sol.N[0]
    J = np.exp(3 * N) * L**2 * np.sinh(phi / L) ** 2 * thetadot
    assert np.max(np.abs(J / J[0] - 1)) <= 1e-8


# fixed-dt GPU run against the restatement on the same generated model function (twin): hipcc contracts a*b+c into FMAs inside the
# generated code and the integrator, the host twin does not, so the two differ by rounding that the trajectory carries along;
# EGNO's eom^a cancel to ~1e-7 relative at some points (test_background.py) and D5's are long sums, which amplifies those roundings.
# Measured on MI355X: hyperbolic 2.6e-16, doc 1.3e-16, angular 3.3e-21, EGNO 1.2e-13, D5 6.8e-12; the bounds leave a factor ~10
RESTATEMENT_TOL = {"hyperbolic": 1e-12, "doc": 1e-12, "angular": 1e-12, "egno": 1e-12, "d5": 1e-10}


@pytest.mark.parametrize("name", ["hyperbolic", "doc", "angular", "egno", "d5"])
def test_friedmann_constraint_and_restatement(bg, name):
    spec, art = workloads.artifact_for(name)
    twin = BackgroundTwin(art)
    init = np.array([initial_state(name, seed=s) for s in range(8)])
    if name == "angular":  # V ~ 1e-12: velocities of the same energy, not a kinetic-dominated collapse that runs H down by decades
        init[:, 2:] *= 1e-6
    # the error bound is absolute (the reference's norm): scaled to the model's Hubble rate (angular: V ~ 1e-12, D5: ~ 1e-6)
    e0 = twin.eom(spec.args, init)
    max_err = 1e-10 * float(np.min(np.sqrt((e0[:, 2] + 0.5 * e0[:, 3]) / 3)))
    sol = bg.solve_eom_batch(art, spec.args, 200, init[:, :2], init[:, 2:], max_err=max_err, solver="rkf")
    # (a trajectory may run into a point where the model is not finite -- the angular model's field space has one --: it stops
    # with NONFINITE and NaN rows; the others must complete)
    assert np.isin(sol.status, (COMPLETE, NONFINITE)).all() and (sol.status == COMPLETE).sum() >= 6, sol.status
    st = sol.states.reshape(-1, 5)
    h0 = np.repeat(sol.states[:, 0, 4], sol.states.shape[1])
    keep = np.isfinite(st).all(axis=1)
    st, h0 = st[keep], h0[keep]
    pts = np.ascontiguousarray(st[:, :4])
    vals = twin.eom(spec.args, pts)
    H = st[:, 4]
    # relative to the trajectory's initial energy scale 3 H0^2: the error bound is absolute and scaled to H0, and in the kinetic-dominated
    # runs (EGNO's V is negative in its box) H falls by decades, so that 3H^2 alone would measure the bound, not the integration
    resid = np.abs(3 * H**2 - vals[:, 2] - 0.5 * vals[:, 3]) / (3 * h0**2)
    print(f"{name}: Friedmann residual, max {resid.max():.3e}")
    assert resid.max() <= 1e-6, resid.max()

    def eom(a, b, c, d, p):
        return tuple(twin.eom(p, np.array([[a, b, c, d]]))[0])

    k = int(np.argmax(sol.status == COMPLETE))
    fixed = bg.solve_eom_batch(art, spec.args, 60, init[k : k + 1, :2], init[k : k + 1, 2:], solver="rk4", dt=1e-3)
    want, meta = Restatement(eom, spec.args).solve(init[k], 60, "rk4", dt=1e-3)
    got = np.concatenate([fixed.states[0], fixed.N[0][:, None], fixed.t[0][:, None]], axis=1)
    rel = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-3))
    print(f"{name}: fixed-dt GPU vs restatement, max relative difference {rel:.3e}")
    assert rel <= RESTATEMENT_TOL[name], rel


def _hyper_batch(B, seed=0):
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(1.5, 4.0, B), rng.uniform(-1, 1, B)], axis=1)
    v = rng.uniform(-0.2, 0.2, (B, 2))
    return x, v


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_determinism_and_lane_independence(bg, solver):
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = _hyper_batch(257)
    one = bg.solve_eom(art, p, 40, x[5], v[5], solver=solver)
    b1 = bg.solve_eom_batch(art, p, 40, x[5:6], v[5:6], solver=solver)
    assert one.flags.c_contiguous and one.shape == (40, 5)
    assert np.array_equal(one, b1.states[0])
    full = bg.solve_eom_batch(art, p, 40, x, v, solver=solver)
    perm = np.random.default_rng(1).permutation(257)
    shuffled = bg.solve_eom_batch(art, p, 40, x[perm], v[perm], solver=solver)
    for f in ("states", "t", "N", "status", "last_row"):
        assert np.array_equal(getattr(full, f)[perm], getattr(shuffled, f), equal_nan=True), f
    for B in (1, 63):
        part = bg.solve_eom_batch(art, p, 40, x[:B], v[:B], solver=solver)
        assert np.array_equal(part.states, full.states[:B], equal_nan=True)
    # per-lane parameter rows equal separate calls
    pars = np.stack([p * (1 + 0.1 * k) for k in range(3)])
    rows = bg.solve_eom_batch(art, pars, 40, x[:3], v[:3], solver=solver)
    for k in range(3):
        sep = bg.solve_eom_batch(art, pars[k], 40, x[k : k + 1], v[k : k + 1], solver=solver)
        assert np.array_equal(rows.states[k], sep.states[0], equal_nan=True) and np.array_equal(rows.t[k], sep.t[0])


@pytest.mark.parametrize("dt", [None, 2e-3])
def test_substeps_reproduce_every_kth_row(bg, dt):
    """substeps = k > 256 (a row spans launches of at most 256 steps) records exactly every k-th row of a substeps = 1 run."""
    spec, art = workloads.artifact_for("hyperbolic")
    x, v = _hyper_batch(40, seed=5)
    k, R = 300, 4
    fine = bg.solve_eom_batch(art, spec.args, (R - 1) * k + 1, x, v, max_err=1e-9, dt=dt)
    coarse = bg.solve_eom_batch(art, spec.args, R, x, v, max_err=1e-9, dt=dt, substeps=k)
    assert np.array_equal(coarse.states, fine.states[:, ::k], equal_nan=True)
    assert np.array_equal(coarse.t, fine.t[:, ::k], equal_nan=True) and np.array_equal(coarse.N, fine.N[:, ::k], equal_nan=True)
    assert np.array_equal(coarse.status, fine.status)
    done = fine.status == COMPLETE
    assert done.any() and np.array_equal(coarse.last_row[done], fine.last_row[done] // k)


def test_row_buffer_drains_and_lane_chunks(bg):
    """B = 100 003 with 60 rows fills the device row buffer (47 rows) and drains it inside the call; B = 2^20 + 3 takes two passes of
    lanes.  Both equal calls on a few of their lanes alone."""
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = _hyper_batch(100_003, seed=6)
    big = bg.solve_eom_batch(art, p, 60, x, v, substeps=2)
    for sl in (slice(0, 64), slice(100_003 - 77, None)):
        small = bg.solve_eom_batch(art, p, 60, x[sl], v[sl], substeps=2)
        assert np.array_equal(big.states[sl], small.states, equal_nan=True) and np.array_equal(big.t[sl], small.t, equal_nan=True)
    B = (1 << 20) + 3
    x, v = _hyper_batch(B, seed=7)
    big = bg.solve_eom_batch(art, p, 3, x, v, dt=1e-3)
    for sl in (slice(0, 5), slice((1 << 20) - 2, None)):
        small = bg.solve_eom_batch(art, p, 3, x[sl], v[sl], dt=1e-3)
        assert np.array_equal(big.states[sl], small.states) and np.array_equal(big.status[sl], small.status)


def test_large_batch_and_launch_boundaries(bg):
    """B = 100 003 against the first lanes run alone, and the first R rows of a 2R-row call (several launches of 256 steps) equal an
    R-row call."""
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = _hyper_batch(100_003, seed=2)
    big = bg.solve_eom_batch(art, p, 20, x, v, substeps=3)
    small = bg.solve_eom_batch(art, p, 20, x[-257:], v[-257:], substeps=3)
    assert np.array_equal(big.states[-257:], small.states, equal_nan=True)
    R = 300
    long = bg.solve_eom_batch(art, p, 2 * R, x[:64], v[:64], max_err=1e-9)
    short = bg.solve_eom_batch(art, p, R, x[:64], v[:64], max_err=1e-9)
    assert np.array_equal(long.states[:, :R], short.states, equal_nan=True)
    assert np.array_equal(long.t[:, :R], short.t, equal_nan=True)


def test_end_of_inflation_and_efolds_map(bg):
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    eom = model_functions(workloads.model_for("hyperbolic"), art.symbol_dictionary)
    for init in ([3.0, 0.5, 0.0, 0.1], [4.0, -0.3, 0.1, 0.0]):
        # N_end is linear in epsilon_H across the last step: its error goes with the square of that step's dN, so a fixed small dt
        # (adaptive steps near the end span dN ~ 1e-2 and put N_end ~ 3e-5 off)
        sol = bg.solve_eom_batch(art, p, 50_000, [init[:2]], [init[2:]], solver="rk4", dt=1e-3, stop_at_end=True)
        assert sol.status[0] == ENDED
        last = sol.last_row[0]
        assert np.all(np.isnan(sol.states[0, last + 1 :]))
        ref = solve_ivp_reference(eom, p, init, 1e4, end_event=True)
        n_ref = ref.y_events[0][0][5]
        assert abs(sol.N_end[0] - n_ref) <= 1e-6 * n_ref, (sol.N_end[0], n_ref)
    ss = np.array([[1.0, 5.0], [-1.0, 1.0]])
    N0, N1 = 24, 8
    nend, status = bg.efolds_map(art, p, ss, N0, N1, max_steps=20_000, max_err=1e-9, return_status=True)
    x0, x1 = bg.grid_points(ss, N0, N1)
    X = np.stack([np.repeat(x0, N1), np.tile(x1, N0)], axis=1)
    sol = bg.solve_eom_batch(art, p, 20_001, X, np.zeros_like(X), max_err=1e-9, stop_at_end=True)
    want = np.where(sol.status == ENDED, sol.N_end, np.nan).reshape(N0, N1)
    assert np.array_equal(nend, want, equal_nan=True)
    assert np.array_equal(status.reshape(-1), sol.status)
    # at phi = phi0 (= 1) the field sits at the minimum: V = 0, no inflation, no end
    assert np.isnan(nend[0]).all() and np.isfinite(nend[-1]).all()
    # accuracy of the default, adaptive e-fold map against DOP853: N_end is linear in epsilon_H across the last accepted step
    # (measured with the host build of the integrator at max_err = 1e-8: <= 6e-4 e-folds off on hyperbolic)
    nend = bg.efolds_map(art, p, ss, N0, N1)
    for i, j in ((6, 1), (12, 4), (18, 6), (23, 7)):
        init = [x0[i], x1[j], 0.0, 0.0]
        n_ref = solve_ivp_reference(eom, p, init, 1e4, end_event=True).y_events[0][0][5]
        assert abs(nend[i, j] - n_ref) <= 2e-3, (i, j, nend[i, j], n_ref)
    # a state already past the end of inflation ends at once: N_end = 0, row 0 is its last row
    sol = bg.solve_eom_batch(art, p, 10, [[3.0, 0.0]], [[5.0, 0.0]], stop_at_end=True)
    assert sol.status[0] == ENDED and sol.N_end[0] == 0.0 and sol.last_row[0] == 0 and np.isnan(sol.states[0, 1:]).all()


def test_stopped_lane(bg):
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = _hyper_batch(64, seed=4)
    ok = bg.solve_eom_batch(art, p, 50, x, v)
    x2 = x.copy()
    x2[10, 0] = np.nan
    bad = bg.solve_eom_batch(art, p, 50, x2, v)
    assert bad.status[10] == NONFINITE and np.all(np.isnan(bad.states[10, 1:])) and bad.last_row[10] == 0
    keep = np.arange(64) != 10
    assert np.array_equal(bad.states[keep], ok.states[keep]) and np.array_equal(bad.status[keep], ok.status[keep])


def test_special_function_model(bg):
    from inflatox_amd import Compiler, InflationModelBuilder
    from workloads import example_models

    fields, metric, potential = example_models.bessel_toy()
    model = InflationModelBuilder.new(fields, metric, potential, model_name="bessel_toy", init_sympy_printing=False, silent=True).build()
    art = Compiler(model, silent=True, link_gsl=True).compile()
    p = np.array([1.3, 0.7])
    eom = model_functions(model, art.symbol_dictionary, modules=("scipy", "numpy"))
    init = [2.0, 0.3, 0.05, -0.05]
    sol = bg.solve_eom_batch(art, p, 60, [init[:2]], [init[2:]], solver="rk4", dt=1e-2)
    want, meta = Restatement(eom, p).solve(init, 60, "rk4", dt=1e-2)
    assert sol.status[0] == meta["status"] == COMPLETE
    got = np.concatenate([sol.states[0], sol.N[0][:, None], sol.t[0][:, None]], axis=1)
    assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-3)) <= 1e-11


def test_background_object_lifecycle(bg):
    from inflatox_amd import _native

    spec, art = workloads.artifact_for("doc")
    path = art.ensure_background()
    assert path == art.shared_object_path + ".background"
    lib = _native.InflatoxDevLib(art.shared_object_path)
    groups = lib.groups
    init = np.array([[2.0, 0.8, 0.0, 0.0]])
    states, t, n_end, status, last_row = lib.solve_eom(spec.args, init, 10, 1, _native.EOM_RKF, 1e-6, 0.0, 0)
    assert status[0] == COMPLETE and lib.groups == groups
    want = bg.solve_eom_batch(art, spec.args, 10, init[:, :2], init[:, 2:])
    assert np.array_equal(states[0, :, :5], want.states[0])
    # another model's background object is refused
    _, other = workloads.artifact_for("hyperbolic")
    _, victim = workloads.artifact_for("doc")
    import shutil

    foreign = victim.shared_object_path + ".background"
    shutil.copyfile(other.ensure_background(), foreign)
    try:
        lib2 = _native.InflatoxDevLib(victim.shared_object_path)
        with pytest.raises(SystemError, match="does not belong"):
            lib2.solve_eom(spec.args, init, 10, 1, _native.EOM_RKF, 1e-6, 0.0, 0)
        lib2.close()
    finally:
        os.remove(foreign)  # (the artefact did not build it and does not remove it)
    lib.close()
