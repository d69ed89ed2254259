"""The background solver against an independent truth, without a GPU (tests/background_truth.py): ``eom_fields`` against an
Euler-Lagrange derivation in 40-digit arithmetic, the generated equations-of-motion header against that derivation, DOP853 against
30-digit Taylor integration, and the host build of the steppers against DOP853 on curved and non-diagonal field spaces --
convergence order at a fixed dt and the error of adaptive, sampled runs.  The lanes and bounds of tests/test_background_truth_gpu.py
are established here."""

import numpy as np
import pytest

import background_truth as bt
import workloads
from background_reference import COMPLETE, BackgroundTwin
from background_sampled_reference import SampledTwin
from background_target_reference import TARGET
from test_background import MODELS as WORKLOADS
from test_background import _points
from test_model_fuzz import SEEDS

FUZZ = tuple(f"fuzz{s}" for s in SEEDS)
MAX_ERR = 1e-8  # solve_eom_sampled's default
LANES = 65


def _mp_points(fn, pts, pars):
    import mpmath

    return np.array([fn(*[mpmath.mpf(float(v)) for v in pt], [mpmath.mpf(float(v)) for v in p]) for pt, p in zip(pts, pars)], dtype=object)


def _model_and_points(name, n):
    """(model, parameter slots, points (n, 4), parameter rows (n, n_par)): 20 seeded points inside the model's box"""
    if name in WORKLOADS:
        spec, art = workloads.artifact_for(name)
        return workloads.model_for(name), art.symbol_dictionary, _points(name, n, seed=11), np.tile(spec.args, (n, 1))
    z = bt.zoo_model(name)
    rng = np.random.default_rng(500 + sum(map(ord, name)))
    x0, x1, y0, y1 = z.box
    pts = np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)], axis=1)
    return z.model, None, pts, rng.uniform(0.5, 1.8, (n, 3))


@pytest.mark.parametrize("name", FUZZ + WORKLOADS + bt.NONDIAGONAL)
def test_eom_fields_equal_the_euler_lagrange_derivation(name):
    """The symbolic stage: ``model.eom_fields`` (Christoffel symbols, inverse metric) and the Euler-Lagrange derivation (neither) are
    the same functions -- at 20 seeded points in 40-digit arithmetic they agree to 1e-30 of the value's scale."""
    import mpmath

    model, slots, pts, pars = _model_and_points(name, 20)
    with mpmath.workdps(40):
        want = _mp_points(bt.truth_functions(model, slots, modules="mpmath"), pts, pars)[:, :2]
        got = _mp_points(bt.model_eom_functions(model, slots, modules="mpmath"), pts, pars)
        scale = np.maximum(abs(want), abs(want).max(axis=0) * mpmath.mpf("1e-3"))
        err = (abs(got - want) / scale).max()
    assert err <= 1e-30, (name, float(err))


@pytest.mark.parametrize("name", FUZZ[:12] + bt.NONDIAGONAL)
def test_generated_eom_matches_the_derivation(name):
    """The emitter: ``inflx_eom_point`` compiled for the host against the derivation in 40-digit arithmetic, with the criterion of
    test_background.py::test_generated_eom_matches_sympy -- within four times the error of lambdify's own float64 evaluation of the
    project's expressions, or 1e-12 of the value's scale -- on all 257 lanes of the model's batch, each with its own parameter row."""
    import mpmath

    from background_reference import model_functions

    z, art = bt.zoo_model(name), bt.host_artifact(name)
    twin = BackgroundTwin(art)
    init, pars = bt.batch(name)
    got = np.array([twin.eom(pars[k], init[k : k + 1])[0] for k in range(init.shape[0])])
    float_fn = model_functions(z.model, art.symbol_dictionary)
    plain = np.array([float_fn(*pt, p) for pt, p in zip(init, pars)])
    with mpmath.workdps(40):
        exact = _mp_points(bt.truth_functions(z.model, art.symbol_dictionary, modules="mpmath"), init, pars).astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(exact))
    scale = np.maximum(np.abs(exact), np.max(np.abs(exact), axis=0) * 1e-3)
    err_got = (np.abs(got - exact) / scale).max(axis=0)
    err_plain = (np.abs(plain - exact) / scale).max(axis=0)
    print(f"{name}: generated code {err_got}, lambdify {err_plain}")
    assert np.all(err_got <= np.maximum(4 * err_plain, 1e-12)), (name, err_got, err_plain)


@pytest.mark.parametrize("name", ["fuzz2", "shear"])
def test_truth_trajectory_against_30_digit_integration(name):
    """DOP853 at rtol = 1e-13, atol = 1e-15 against mpmath's Taylor-series integrator at 30 digits on one lane of a curved diagonal
    and of a non-diagonal model, at the sample times up to T = 2: within 1e-11 absolute, what the tolerances imply.  Measured:
    see profiles/background_truth.json; every bound asserted against the truth is more than 100 times the measured figure."""
    z, art = bt.zoo_model(name), bt.host_artifact(name)
    init, pars = bt.batch(name)
    times = [0.5, 1.0, 2.0]
    truth = bt.truths(name, LANES, bt.T_ADAPTIVE)[0]
    rhs_mp = bt.bound(bt.truth_functions(z.model, art.symbol_dictionary, modules="mpmath"), [float(v) for v in pars[0]])
    want = np.array(bt.taylor_trajectory(rhs_mp, init[0], times), dtype=np.float64)
    err = float(np.max(np.abs(truth.sol(np.array(times)).T - want)))
    print(f"{name}: DOP853 against 30-digit integration, max absolute difference {err:.3e}")
    assert err <= bt.TRUTH_TOL, err
    assert err * 100 <= 1e-10  # the smallest figure a later test asks of an error against the truth


@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_every_lane_has_positive_energy_and_a_finite_truth(name):
    """All 257 lanes start with 3 H0^2 = V + G chi chi / 2 > 0; the 65 lanes that are integrated have a finite truth up to T = 2 along
    which H stays positive, so that N rises and every e-fold sample is reached."""
    init, pars = bt.batch(name)
    eom = bt.truth_rhs(name)
    vals = np.array([eom(*pt, p) for pt, p in zip(init, pars)])
    assert init.shape == (257, 4) and pars.shape[0] == 257 and len({tuple(p) for p in pars}) == 257
    assert np.all(np.isfinite(vals)) and np.all(vals[:, 2] + 0.5 * vals[:, 3] > 0)
    for tr in bt.truths(name, LANES, bt.T_ADAPTIVE):
        assert tr.success and tr.t[-1] == bt.T_ADAPTIVE and np.all(np.isfinite(tr.y)) and tr.y[4].min() > 0.05


@pytest.mark.parametrize("method", ["rk4", "rkf"])
@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_host_steppers_are_fourth_order_on_curved_spaces(name, method):
    """Fixed dt = 1/n to T = 1: halving dt cuts the end-point error against the truth by >= 14 on every lane, and the error at
    n = 40 is above 1e-10 -- ten times the bound on the truth's own error, a thousand times what was measured.  The batches
    (background_truth.BATCH_DRAW) were chosen for this to hold on the host build; the GPU runs the same lanes."""
    twin = BackgroundTwin(bt.host_artifact(name))
    init, pars = bt.batch(name)

    def solve(n):
        runs = [twin.solve(pars[k], init[k], n + 1, method, dt=bt.T_ORDER / n) for k in range(LANES)]
        assert all(meta["status"] == COMPLETE for _, meta in runs)
        return np.array([out[-1] for out, _ in runs])

    e40, ratios = bt.order_ratios(solve, name)
    print(f"{name} {method}: error at n = 40 {e40.min():.2e} .. {e40.max():.2e}, ratios {ratios.min():.2f} .. {ratios.max():.2f}")
    assert e40.min() > 1e-10 and ratios.min() >= 14.0, (e40.min(), ratios.min(), int(np.argmin(ratios)))


RESTATEMENT_RATIOS = {}


@pytest.mark.parametrize("at", ["t", "N"])
@pytest.mark.parametrize("method", ["rk4", "rkf"])
@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_adaptive_host_runs_against_truth(name, method, at):
    """``SampledTwin`` at max_err = 1e-8 (the API's default), four samples up to T = 2: every lane's error against the truth at the
    returned times is at most K max_err, K = four times the worst error-to-max_err ratio of the pure-Python ``Restatement`` on the
    independent right-hand side over the same lanes, read at the same samples with the dense output the API documents
    (background_truth.restatement_at_samples); the factor covers libm's pow in the step-size controller, which can move a step
    boundary.  The ratios are recorded in profiles/background_truth.json."""
    art = bt.host_artifact(name)
    init, pars = bt.batch(name)
    truth = bt.truths(name, LANES, bt.T_ADAPTIVE)
    samples = bt.samples_for(name, at)
    twin = SampledTwin(art)
    ref, got = np.empty(LANES), np.empty(LANES)
    for k in range(LANES):
        rows = bt.restatement_at_samples(name, k, samples, at, method, MAX_ERR, bt.T_ADAPTIVE)
        ref[k] = bt.error_against_truth(rows, truth[k]) / MAX_ERR
        out, meta = twin.solve(pars[k], init[k], samples, 100_000, method, max_err=MAX_ERR, at=at, stop_at_end=False)
        assert meta["status"] == TARGET and meta["n_stored"] == 4 and np.all(out[:, 6] <= bt.T_ADAPTIVE * (1 + 1e-12))
        got[k] = bt.error_against_truth(out, truth[k]) / MAX_ERR
    RESTATEMENT_RATIOS[f"{name}/{method}/{at}"] = dict(restatement=float(ref.max()), host_build=float(got.max()))
    print(f"{name} {method} at {at}: error / max_err, restatement {ref.max():.2f}, host build {got.max():.2f}")
    assert ref.max() * MAX_ERR >= 100 * bt.TRUTH_TOL  # what is bounded is well clear of the truth's own error
    assert got.max() <= 4.0 * ref.max(), (got.max(), ref.max(), int(np.argmax(got)))
