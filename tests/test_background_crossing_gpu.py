"""Horizon crossings on the GPU (inflatox_amd.background.horizon_crossings, inflation_end and what stands on them): located states against
state_at_efolds, launch boundaries and several crossings per step against the host build of the same code, an independent truth on
curved and non-diagonal field spaces, the located end of inflation, spectra on a common k-grid against power_spectra and
tensor_spectra row by row, the observables on the power law, the pivot maps against their halves, lane chunks, the heavy-register
models and the refusal of an object of another layout."""

import math
import os
import subprocess

import numpy as np
import pytest

import background_truth as bt
import modes_reference as mo
import tensor_reference as tn
import workloads
from background_reference import COMPLETE, ENDED, P_POW, model_functions, power_law_artifact, power_law_init, solve_ivp_reference
from background_sampled_reference import EGNO_SEEDS
from background_target_reference import TARGET
from crossing_reference import CrossingTwin
from test_background import initial_state
from test_background_gpu import RESTATEMENT_TOL, _hyper_batch

pytestmark = pytest.mark.gpu

FIELDS = ("states", "N", "t", "eps_H", "ln_aH", "n_stored", "n_before", "N_end", "status")
LANES = 65
TRUTH_LN_K = np.array([0.2, 0.5, 0.8, 1.0])


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return np.asarray(spec.args, dtype=np.float64), art


def _ln_h0(bg, art, p, x, v):
    """ln H_0 of every trajectory: row 0 of a one-row run"""
    return np.log(bg.solve_eom_batch(art, p, 1, x, v).states[:, 0, 4])


def _planes(sol):
    """(B, S, 8): y[0..4], N, t, epsilon_H -- the twin's layout"""
    return np.concatenate([sol.states, sol.N[..., None], sol.t[..., None], sol.eps_H[..., None]], axis=2)


def _emitted(sol):
    j = np.arange(sol.N.shape[1])[None, :]
    return (j >= sol.n_before[:, None]) & (j < (sol.n_before + sol.n_stored)[:, None])


def _against_the_twin(sol, twin, p, x, v, offset, samples, max_steps, tol, **kw):
    """test_background_sampled_gpu._against_the_twin for crossings: every lane against the host build of the same code: the same
    status, counts and NaN pattern, N_end and every emitted value within `tol`, relative with a floor of 1e-3.  Returns the worst
    figure and the twin's step_of rows."""
    got = _planes(sol)
    worst, steps = 0.0, []
    for k in range(x.shape[0]):
        want, meta = twin.solve(p if np.ndim(p) == 1 else p[k], np.concatenate([x[k], v[k]]), samples, max_steps, offset=offset[k], **kw)
        assert (sol.status[k], sol.n_stored[k], sol.n_before[k]) == (meta["status"], meta["n_stored"], meta["n_before"]), (k, sol.status[k], sol.n_stored[k], meta)
        assert np.array_equal(np.isnan(got[k]), np.isnan(want)), k
        lo, n = meta["n_before"], meta["n_stored"]
        assert np.isnan(want[:lo]).all() and np.isfinite(want[lo : lo + n]).all() and np.isnan(want[lo + n :]).all()
        if n:
            worst = max(worst, float(np.max(np.abs(got[k, lo : lo + n] - want[lo : lo + n]) / np.maximum(np.abs(want[lo : lo + n]), 1e-3))))
        if meta["status"] == ENDED:
            assert abs(sol.N_end[k] - meta["N_end"]) <= tol * max(meta["N_end"], 1e-3)
        else:
            assert np.isnan(sol.N_end[k])
        steps.append(meta["step_of"])
    return worst, np.array(steps)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_located_states_are_state_at_efolds_at_the_located_n(bg, hyper, solver):
    """B = 96 (a wavefront and a half), S = 7 targets relative to every lane's own ln H_0, one of them before the start (a target AT
    ln H_0 would hang on the last bit of the device's logarithm: the host tests cover it), adaptive, stop_at_end.  Every emitted sample, passed to state_at_efolds at its located N, returns the same state, t and epsilon_H to
    1e-12 relative: the same interpolant of the same step, theta from two iterations that each stop at 1e-15.  The NaN pattern is
    exactly n_before and n_stored, and the residual N + ln H - target is at rounding."""
    p, art = hyper
    x, v = _hyper_batch(96)
    ln_k = np.array([-0.5, 0.005, 0.01, 0.03, 0.06, 0.1, 0.2])
    offset = _ln_h0(bg, art, p, x, v)
    sol = bg.horizon_crossings(art, p, ln_k, x, v, offset=offset, solver=solver)
    assert sol.states.shape == (96, 7, 5) and sol.t.shape == sol.N.shape == sol.eps_H.shape == sol.ln_aH.shape == (96, 7)
    assert sol.n_stored.dtype == sol.n_before.dtype == np.uint32 and sol.status.dtype == np.int8
    assert np.isin(sol.status, (TARGET, ENDED)).all() and (sol.status == TARGET).any() and (sol.status == ENDED).any(), np.bincount(sol.status)
    emitted = _emitted(sol)
    for member in (sol.N, sol.t, sol.eps_H, sol.ln_aH, *np.moveaxis(sol.states, 2, 0)):
        assert np.array_equal(emitted, ~np.isnan(member))
    assert np.all(sol.n_before == 1) and np.array_equal(sol.status == TARGET, sol.n_stored == 6) and np.array_equal(np.isnan(sol.N_end), sol.status == TARGET)
    tau = offset[:, None] + ln_k[None, :]
    residual = np.abs(sol.ln_aH - tau)[emitted] / np.maximum(1.0, np.abs(tau[emitted]))
    print(f"{solver}: status {np.bincount(sol.status)}, emitted per sample {emitted.sum(axis=0)}, worst residual {residual.max():.3e}")
    assert residual.max() <= 1e-12
    worst = 0.0
    for s in range(1, 7):
        e = emitted[:, s]
        assert e.any()
        one = bg.state_at_efolds(art, p, x[e], v[e], sol.N[e, s], solver=solver)
        assert np.all(one.status == TARGET) and np.array_equal(one.N, sol.N[e, s])
        for got, want in ((sol.states[e, s], one.state), (sol.t[e, s], one.t), (sol.eps_H[e, s], one.eps_H)):
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-3))))
    print(f"{solver}: located states against state_at_efolds at the located N, max relative difference {worst:.3e}")
    assert worst <= 1e-12, worst


def test_launch_boundaries_and_crossings_in_one_step(bg, hyper):
    """Fixed dt = 1e-3: more than 256 accepted steps (a launch) lie between two crossings, and 1000 steps do not reach the last one;
    then dt = 0.5 with three crossings inside the first step.  Against the host build of the same code, which differs by FMA
    contraction only."""
    p, art = hyper
    twin = CrossingTwin(art)
    x, v = _hyper_batch(8, seed=3)
    offset = _ln_h0(bg, art, p, x, v)
    tol = RESTATEMENT_TOL["hyperbolic"]
    samples = np.array([0.02, 0.15, 0.4, 50.0])
    sol = bg.horizon_crossings(art, p, samples, x, v, offset=offset, max_steps=1000, solver="rk4", dt=1e-3)
    worst, steps = _against_the_twin(sol, twin, p, x, v, offset, samples, 1000, tol, method="rk4", dt=1e-3, stop_at_end=True)
    print(f"dt = 1e-3: GPU vs host build, max relative difference {worst:.3e}; emitted in steps {steps[1]}")
    assert worst <= tol, worst
    assert np.nanmax(np.diff(steps[:, :3], axis=1)) > 256 and (sol.status == COMPLETE).any() and (sol.n_stored >= 2).sum() >= 4
    samples = np.array([1e-3, 2e-3, 3e-3])
    sol = bg.horizon_crossings(art, p, samples, x, v, offset=offset, max_steps=10, solver="rkf", dt=0.5)
    worst, steps = _against_the_twin(sol, twin, p, x, v, offset, samples, 10, tol, method="rkf", dt=0.5, stop_at_end=True)
    print(f"dt = 0.5: GPU vs host build, max relative difference {worst:.3e}")
    assert worst <= tol, worst
    assert (steps == 1).all(axis=1).any(), steps


def _truth_crossings(truth, tau):
    """(S, 7): the truth's y[0..5] and t where its N + ln H crosses every tau -- a bracketed root on the dense output --, or None when
    the lane does not take part: L must be strictly increasing on [0, T] (a grid of 2001 points) and span more than 1.0"""
    from scipy.optimize import brentq

    grid = np.linspace(0.0, bt.T_ADAPTIVE, 2001)
    y = truth.sol(grid)
    if not (y[4] > 0.0).all():
        return None
    L = y[5] + np.log(y[4])
    if not ((np.diff(L) > 0.0).all() and L[-1] - L[0] > 1.0):
        return None
    rows = np.empty((len(tau), 7))
    for s, target in enumerate(tau):
        g = lambda t, target=target: truth.sol(t)[5] + math.log(truth.sol(t)[4]) - target  # noqa: E731
        t_star = brentq(g, 0.0, bt.T_ADAPTIVE, xtol=1e-15, rtol=4 * np.finfo(float).eps)
        rows[s, :6], rows[s, 6] = truth.sol(t_star), t_star
    return rows


@pytest.mark.parametrize("name", ["fuzz2", "fuzz4", "fuzz5", "skew", "shear"])
def test_crossings_against_an_independent_truth(bg, name):
    """65 lanes with per-lane parameter rows, stop_at_end=False, offset = every lane's ln H_0, ln_k = [0.2, 0.5, 0.8, 1.0], T = 2.  The
    truth (DOP853 on the Euler-Lagrange derivation) is read where its own N + ln H crosses the target.  err_gpu <= 2 err_host +
    TRUTH_TOL per lane, as in test_adaptive_runs_against_truth.  A lane takes part only if the truth's L is strictly increasing on
    [0, T] and spans more than 1.0; at most 2 of 65 may drop out."""
    art = bt.device_artifact(name)
    init, pars = (a[:LANES] for a in bt.batch(name))
    truth = bt.truths(name, LANES, bt.T_ADAPTIVE)
    h0 = np.array([tr.sol(0.0)[4] for tr in truth])
    offset = np.log(h0)
    wanted = [_truth_crossings(truth[k], offset[k] + TRUTH_LN_K) for k in range(LANES)]
    lanes = [k for k in range(LANES) if wanted[k] is not None]
    print(f"{name}: {len(lanes)} of {LANES} lanes take part")
    assert len(lanes) >= LANES - 2
    twin = CrossingTwin(bt.host_artifact(name), contract="fast")
    for solver in ("rk4", "rkf"):
        sol = bg.horizon_crossings(art, pars, TRUTH_LN_K, init[:, :2], init[:, 2:], offset=offset, solver=solver, stop_at_end=False)
        got = np.concatenate([sol.states, sol.N[..., None], sol.t[..., None]], axis=2)
        err_gpu, err_host = np.empty(len(lanes)), np.empty(len(lanes))
        for i, k in enumerate(lanes):
            assert sol.status[k] == TARGET and sol.n_stored[k] == 4 and sol.n_before[k] == 0, (k, sol.status[k], sol.n_stored[k], sol.n_before[k])
            out, meta = twin.solve(pars[k], init[k], TRUTH_LN_K, 100_000, offset=offset[k], method=solver, max_err=1e-8, stop_at_end=False)
            assert meta["status"] == TARGET
            err_gpu[i], err_host[i] = np.max(np.abs(got[k] - wanted[k])), np.max(np.abs(out[:, :7] - wanted[k]))
        print(f"{name} {solver}: error against the truth's crossings, GPU {err_gpu.max():.3e}, host build {err_host.max():.3e}, worst GPU-to-host ratio {np.max(err_gpu / err_host):.6f}")
        assert np.all(err_gpu <= 2.0 * err_host + bt.TRUTH_TOL), (lanes[int(np.argmax(err_gpu / err_host))], err_gpu.max(), err_host.max())


def test_inflation_end(bg, hyper):
    """The hyperbolic batch against the host build within RESTATEMENT_TOL, rk4 and rkf; then against DOP853 with an exact event: within
    1e-6 N_end at rk4 with dt = 1e-3, the bound test_end_of_inflation_and_efolds_map asserts of the linear rule there, and within its
    2e-3 e-folds at the adaptive default."""
    p, art = hyper
    twin = CrossingTwin(art)
    x, v = _hyper_batch(96)
    tol = RESTATEMENT_TOL["hyperbolic"]
    for solver in ("rk4", "rkf"):
        end = bg.inflation_end(art, p, x, v, solver=solver)
        assert end.state.shape == (96, 5) and end.N_end.shape == end.t_end.shape == end.eps_H.shape == (96,) and end.status.dtype == np.int8
        assert np.all(end.status == ENDED) and np.max(np.abs(end.eps_H - 1.0)[end.N_end > 0.0]) <= 1e-12 and (end.N_end == 0.0).any()
        got = np.concatenate([end.state, end.N_end[:, None], end.t_end[:, None], end.eps_H[:, None]], axis=1)
        want = np.array([twin.end(p, np.concatenate([x[k], v[k]]), 100_000, method=solver)[0] for k in range(96)])
        worst = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-3)))
        print(f"{solver}: located end of inflation, GPU vs host build {worst:.3e}")
        assert worst <= tol, worst
    short = bg.inflation_end(art, p, x[:4], v[:4], max_steps=3)
    assert np.array_equal(short.status == ENDED, short.N_end == 0.0) and np.all(short.status[short.N_end != 0.0] == COMPLETE) and np.isnan(short.state[short.status == COMPLETE]).all()
    eom = model_functions(workloads.model_for("hyperbolic"), art.symbol_dictionary)
    inits = np.array([[3.0, 0.5, 0.0, 0.1], [4.0, -0.3, 0.1, 0.0]])
    fixed = bg.inflation_end(art, p, inits[:, :2], inits[:, 2:], max_steps=50_000, solver="rk4", dt=1e-3)
    adaptive = bg.inflation_end(art, p, inits[:, :2], inits[:, 2:])
    for k, init in enumerate(inits):
        ref = solve_ivp_reference(eom, p, init, 1e4, end_event=True)
        n_ref = ref.y_events[0][0][5]
        print(f"N_end: DOP853 {n_ref:.9f}, rk4 dt = 1e-3 {fixed.N_end[k]:.9f}, adaptive {adaptive.N_end[k]:.9f}")
        assert fixed.status[k] == ENDED and abs(fixed.N_end[k] - n_ref) <= 1e-6 * n_ref, (fixed.N_end[k], n_ref)
        assert adaptive.status[k] == ENDED and abs(adaptive.N_end[k] - n_ref) <= 2e-3, (adaptive.N_end[k], n_ref)


def _same_members(a, b, rows=slice(None), cols=slice(None)):
    return all(np.array_equal(u[rows][:, cols], w, equal_nan=True) for u, w in zip(a, b))


@pytest.mark.parametrize("tensor", [False, True])
def test_spectra_at_k_are_the_spectra_at_the_located_exits(bg, hyper, tensor):
    """B = 5 trajectories high on the hyperbolic potential, K = 4 wavenumbers shared by all: one outside the horizon at every start, one
    that leaves it fewer than N_sub = 3 e-folds later, two whose ln k lies 3.2 and 3.4 above the latest start's ln H_0 (they leave after 3.4 to 3.8 e-folds: d ln(a H) / dN = 1 - epsilon_H).  For each trajectory alone,
    power_spectra / tensor_spectra with N_exit = its own located N equals its row bit for bit in every member; the first two columns
    are OUTSIDE_AT_START and NaN; rows are invariant under a permutation of the batch."""
    p, art = hyper
    x, v = mo.hyper_states()
    l0 = _ln_h0(bg, art, p, x, v)
    ln_k = np.array([l0.min() - 1.0, l0.max() + 0.5, l0.max() + 3.2, l0.max() + 3.4])
    at_k, plain = (bg.tensor_spectra_at_k, bg.tensor_spectra) if tensor else (bg.power_spectra_at_k, bg.power_spectra)
    kw = dict(N_eval=mo.HYPER_N_EVAL, N_sub=3.0)
    got, exits = at_k(art, p, ln_k, x, v, **kw)
    assert isinstance(got, bg.TensorSpectra if tensor else bg.PowerSpectra) and isinstance(exits, bg.ExitPoints)
    assert np.array_equal(exits.ln_k, ln_k) and exits.N_exit.shape == (5, 4)
    assert np.isnan(exits.N_exit[:, 0]).all() and np.all(exits.N_exit[:, 1] < 3.0) and np.all(exits.N_exit[:, 2:] > 3.2) and np.all(exits.N_exit[:, 2:] < 4.0)
    assert np.all(got.status[:, :2] == bg.OUTSIDE_AT_START) and np.all(got.status[:, 2:] == TARGET), got.status
    for field, member in zip(got._fields[:-1], got[:-1]):
        assert np.isnan(member[:, :2]).all(), field
        assert np.isnan(member[:, 2:]).all() if field == "N_end" else np.isfinite(member[:, 2:]).all(), field  # (N_eval: no lane ENDED)
    assert np.allclose(np.log(got.k[:, 2:]), np.broadcast_to(ln_k[2:], (5, 2)), rtol=0.0, atol=1e-12)
    for b in range(5):
        alone = plain(art, p, exits.N_exit[b, 2:], x[b : b + 1], v[b : b + 1], **kw)
        assert _same_members(got, alone, slice(b, b + 1), slice(2, 4)), b
    perm = np.array([3, 0, 4, 2, 1])
    shuffled, exits2 = at_k(art, p, ln_k, x[perm], v[perm], **kw)
    assert all(np.array_equal(u[perm], w, equal_nan=True) for u, w in zip(got, shuffled)) and np.array_equal(exits.N_exit[perm], exits2.N_exit, equal_nan=True)
    if not tensor:
        tens, exits3 = bg.tensor_spectra_at_k(art, p, ln_k, x, v, **kw)
        assert np.array_equal(tens.k, got.k, equal_nan=True) and np.array_equal(exits3.N_exit, exits.N_exit, equal_nan=True)


def test_observables_at_k_on_the_power_law(bg):
    """The pivot that leaves the horizon at N = 3.5 on the attractor -- L = N (1 - 1 / p) + ln p --, dlnk = 0.4375 so that its
    neighbours leave at N = 3 and N = 4, N_sub = 3, N_eval = 10: n_s - 1 = n_t = -2 / 7, r = 16 / p, alpha_s = 0, each within
    tensor_reference.stencil_bounds for the uniform stencil."""
    art, p, init, _h = mo.power_law_case()
    slope = 1.0 - 1.0 / P_POW
    obs = bg.observables_at_k(art, p, [3.5 * slope], init[None, :2], init[None, 2:], dlnk=0.5 * slope, offset=math.log(P_POW), N_eval=mo.POWER_N_EVAL, N_sub=tn.N_SUB,
                              stop_at_end=False)  # fmt: skip
    assert isinstance(obs, bg.Observables) and obs.n_s.shape == (1, 1) and obs.status[0, 0] == TARGET
    eps = 1.0 / P_POW
    tilt = -2.0 * eps / (1.0 - eps)
    ln_k3 = math.log(P_POW) + slope * np.array([3.0, 3.5, 4.0])
    b_ns, b_alpha, b_nt, b_r = tn.stencil_bounds(np.exp(ln_k3), mo.power_law_bound(), tn.power_law_bound())
    print(f"power law at fixed k: n_s - 1 {obs.n_s[0, 0] - 1:.6f} and n_t {obs.n_t[0, 0]:.6f} (exact {tilt:.6f}; bounds {b_ns:.2e}, {b_nt:.2e}), r {obs.r[0, 0]:.6f} "
          f"(bound {b_r:.2e} of 2), alpha_s {obs.alpha_s[0, 0]:.2e} (bound {b_alpha:.2e})")  # fmt: skip
    assert abs(obs.n_s[0, 0] - 1.0 - tilt) <= b_ns and abs(obs.n_t[0, 0] - tilt) <= b_nt and abs(obs.alpha_s[0, 0]) <= b_alpha
    assert abs(obs.r[0, 0] / (16.0 * eps) - 1.0) <= b_r and np.isclose(math.log(obs.k[0, 0]), ln_k3[1], rtol=0.0, atol=1e-7)
    lone = bg.observables_at_k(art, p, [-3.0], init[None, :2], init[None, 2:], dlnk=0.5 * slope, offset=math.log(P_POW), N_eval=mo.POWER_N_EVAL, N_sub=tn.N_SUB, stop_at_end=False)
    assert lone.status[0, 0] == bg.OUTSIDE_AT_START and np.isnan(lone.n_s[0, 0]) and np.isnan(lone.r[0, 0])


def test_pivot_maps_are_their_halves(bg, hyper):
    """The 6 x 5 hyperbolic grid from rest with A = reheating_offset(): 0.05 / Mpc and instant reheating.  The rows low on the potential
    inflate too briefly for that scale.  pivot_exit_map equals inflation_end followed by horizon_crossings bit for bit, N_star equals
    ln H_star - ln(H_end) / 2 - A to 1e-12, pivot_observables_map equals the restart at L_star - (dlnk + N_sub) followed by
    observables_at_k bit for bit, and both are NaN exactly where nothing was found.  n_s, r and N_star of the grid are printed."""
    p, art = hyper
    ss, N0, N1 = [[14.0, 19.0], [-1.0, 1.0]], 6, 5
    A = bg.reheating_offset()
    state, n_star, n_end, status = bg.pivot_exit_map(art, p, ss, N0, N1, A, return_status=True)
    short = bg.pivot_exit_map(art, p, ss, N0, N1, np.full((N0, N1), A))
    assert len(short) == 3 and all(np.array_equal(u, w, equal_nan=True) for u, w in zip(short, (state, n_star, n_end)))
    x0, x1 = bg.grid_points(ss, N0, N1)
    x = np.stack([np.repeat(x0, N1), np.tile(x1, N0)], axis=1)
    v = np.zeros_like(x)
    end = bg.inflation_end(art, p, x, v)
    assert np.all(end.status == ENDED) and np.array_equal(end.N_end.reshape(N0, N1), n_end)
    pivot = end.N_end + 0.5 * np.log(end.state[:, 4]) + A
    cr = bg.horizon_crossings(art, p, [0.0], x, v, offset=pivot)
    found = (cr.n_stored == 1).reshape(N0, N1)
    assert 0 < found.sum() < 30, found.sum()
    assert np.array_equal(status == TARGET, found) and np.array_equal(status == bg.ENDED_SHORT, (cr.n_before == 1).reshape(N0, N1)) and np.array_equal(status == bg.ENDED_SHORT, ~found)
    assert np.array_equal(state, cr.states[:, 0].reshape(N0, N1, 5), equal_nan=True) and np.array_equal(n_star, (end.N_end - cr.N[:, 0]).reshape(N0, N1), equal_nan=True)
    assert np.isfinite(state[found]).all() and np.isfinite(n_star[found]).all() and np.isnan(state[~found]).all() and np.isnan(n_star[~found]).all()
    from_h = np.log(state[..., 4]) - 0.5 * np.log(end.state[:, 4]).reshape(N0, N1) - A
    assert np.max(np.abs(n_star - from_h)[found]) <= 1e-12 * np.max(np.abs(pivot)), np.max(np.abs(n_star - from_h)[found])

    obs, restart, n_star2, n_end2, status2 = bg.pivot_observables_map(art, p, ss, N0, N1, A, return_status=True)
    assert np.array_equal(n_end2, n_end) and isinstance(obs, bg.Observables) and all(member.shape == (N0, N1) for member in obs)
    back = bg.horizon_crossings(art, p, [-5.5], x, v, offset=pivot)
    found2 = (back.n_stored == 1).reshape(N0, N1)
    assert 0 < found2.sum() < found.sum() and not (found2 & ~found).any()
    assert np.array_equal(restart, back.states[:, 0].reshape(N0, N1, 5), equal_nan=True)
    run = np.flatnonzero(found2.reshape(-1))
    half = bg.observables_at_k(art, p, [0.0], back.states[run, 0, :2], back.states[run, 0, 2:4], offset=pivot[run] - back.N[run, 0], max_steps=100_000)
    with np.printoptions(precision=5, linewidth=200):
        print(f"n_s:\n{obs.n_s}\nr:\n{obs.r}\nN_star (pivot_exit_map):\n{n_star}\nN_star (pivot_observables_map):\n{n_star2}")
    for grid, member in zip(obs[:-1], half[:-1]):
        assert np.array_equal(grid[found2], member[:, 0], equal_nan=True) and np.isnan(grid[~found2]).all()
    assert np.array_equal(obs.status, status2) and np.array_equal(status2[found2], half.status[:, 0]) and np.all(status2[found2] == ENDED)
    assert all(np.isfinite(member[found2]).all() for member in obs[:-1]) and np.isnan(n_star2[~found2]).all()
    # the restart takes H from the Friedmann constraint again: the pivot's exit moves by that state's own error, not by more
    assert np.max(np.abs(n_star2 - n_star)[found2]) <= 1e-6


def test_lane_independence_and_lane_chunks(bg, hyper):
    """S = 64 crossings are 64 x 8 doubles per lane, so the 256 MiB sample buffer holds 65 536 lanes: B = 65 541 takes two passes, and
    the second one's five lanes land behind the first one's in every plane of the result.  Bit for bit calls on a few lanes alone."""
    p, art = hyper
    B = 65_536 + 5
    x, v = _hyper_batch(B, seed=8)
    offset = _ln_h0(bg, art, p, x, v)
    samples = np.linspace(1e-5, 4.5e-4, 64)
    kw = dict(max_steps=5, solver="rkf", dt=1e-3, stop_at_end=False)
    big = bg.horizon_crossings(art, p, samples, x, v, offset=offset, **kw)
    assert np.isin(big.status, (TARGET, COMPLETE)).all() and (big.status == TARGET).sum() > B // 2 and np.array_equal(big.n_stored == 64, big.status == TARGET)
    assert np.array_equal(_emitted(big), np.isfinite(big.N)) and np.all(big.n_before == 0)
    for sl in (slice(0, 5), slice(65_534, 65_538), slice(B - 5, None)):
        small = bg.horizon_crossings(art, p, samples, x[sl], v[sl], offset=offset[sl], **kw)
        for f in FIELDS:
            assert np.array_equal(getattr(big, f)[sl], getattr(small, f), equal_nan=True), (sl, f)
    perm = np.random.default_rng(1).permutation(300)
    shuffled = bg.horizon_crossings(art, p, samples, x[perm], v[perm], offset=offset[perm], **kw)
    for f in FIELDS:
        assert np.array_equal(getattr(big, f)[perm], getattr(shuffled, f), equal_nan=True), f


@pytest.mark.parametrize("name", ["egno", "d5"])
def test_heavy_models(bg, name):
    """B = 64, 50 fixed steps, five targets relative to every lane's ln H_0 (one before the start): the kernels with the most registers
    against the host build, crossings and the end of inflation.  EGNO (dt = 1e-3) runs the initial states of
    background_sampled_reference.EGNO_SEEDS, at which the host build itself carries the rounding of an FMA within a tenth of the bound;
    at its example parameters EGNO's potential is negligible beside the kinetic energy (epsilon_H = 3 throughout), so ln(a H) falls and
    no lane emits a crossing: what is compared there are the statuses and the counts, and the end of inflation at the start.
    D5 has H ~ 1e-3, so ln(a H) ~ -7 is known to 8e-16 while a lane gains 2e-4 at most before its epsilon_H passes 1: the time of
    a crossing is fixed to about 1e-12 and no better, whatever computes it -- the host build with and without FMA contraction differs
    by that.  With dt = 0.1 and targets 1e-4 to 2e-4 above ln H_0 the crossings lie at t > 0.1, where this is 2.6e-11 of the values
    between the two host builds (with dt = 1e-3 and t ~ 1e-3 it is 2.5e-9, above the bound itself)."""
    spec, art = workloads.artifact_for(name)
    p = np.asarray(spec.args, dtype=np.float64)
    twin = CrossingTwin(art)
    init = np.array([initial_state(name, seed=s) for s in (EGNO_SEEDS if name == "egno" else range(64))])
    if name == "d5":  # V ~ 1e-6: velocities of the same energy
        init[:, 2:] *= 1e-3
    x, v = np.ascontiguousarray(init[:, :2]), np.ascontiguousarray(init[:, 2:])
    offset = _ln_h0(bg, art, p, x, v)
    dt = 1e-3 if name == "egno" else 0.1
    samples = np.array([-1e-3, 1e-4, 1.3e-4, 1.6e-4, 2e-4])
    for solver in ("rk4", "rkf"):
        sol = bg.horizon_crossings(art, p, samples, x, v, offset=offset, max_steps=50, solver=solver, dt=dt, stop_at_end=False)
        worst, _ = _against_the_twin(sol, twin, p, x, v, offset, samples, 50, RESTATEMENT_TOL[name], method=solver, dt=dt, stop_at_end=False)
        print(f"{name} {solver}: GPU vs host build, max relative difference {worst:.3e}; status {np.bincount(sol.status)}; emitted {np.bincount(sol.n_stored)}")
        assert np.all(sol.n_before == 1) and worst <= RESTATEMENT_TOL[name], worst
        assert np.all(sol.n_stored == 0) if name == "egno" else (sol.n_stored >= 2).sum() >= 12
        end = bg.inflation_end(art, p, x, v, max_steps=50, solver=solver, dt=dt)
        want = [twin.end(p, init[k], 50, method=solver, dt=dt) for k in range(64)]
        assert np.array_equal(end.status, [m["status"] for _o, m in want]) and (end.status == ENDED).sum() >= 32
        hit = end.status == ENDED
        got = np.concatenate([end.state, end.N_end[:, None], end.t_end[:, None], end.eps_H[:, None]], axis=1)[hit]
        ref = np.array([o for o, _m in want])[hit]
        assert np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)) <= RESTATEMENT_TOL[name]


def test_crossing_object_of_another_layout_is_refused():
    """A crossing object built with INFLX_HX_ABI = 2 is refused by both entry points."""
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".crossing"
    hdr, eom_hdr = stale + ".model.h", stale + ".eom.h"
    try:
        for path, text in ((hdr, header_text), (eom_hdr, art.eom_header_text())):
            with open(path, "w") as fh:
                fh.write(text)
        cmd = [hipcc_path(), *options, "-DINFLX_HX_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', os.path.join(_CSRC, "inflx_crossing_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        init = np.array([power_law_init()])
        with pytest.raises(SystemError, match="does not belong"):
            lib.solve_eom_crossings(p, init, np.zeros(1), np.array([2.5]), 100, _native.EOM_RKF, 1e-6, 0.0, 0)
        with pytest.raises(SystemError, match="does not belong"):
            lib.inflation_end(p, init, 100, _native.EOM_RKF, 1e-6, 0.0)
        lib.close()
    finally:
        for path in (stale, hdr, eom_hdr):
            if os.path.exists(path):
                os.remove(path)
