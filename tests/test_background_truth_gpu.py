"""The background kernels against an independent truth (tests/background_truth.py) on fuzzed curved field spaces and on metrics
with G_01 != 0: the device's model function lane by lane with per-lane parameter rows, the convergence order of the device's
steppers against DOP853, adaptive sampled runs against DOP853, and state_at_efolds on a non-diagonal model.  Lanes, truth and
bounds are those tests/test_background_truth.py establishes on the host build."""

import mpmath
import numpy as np
import pytest

import background_truth as bt
from background_reference import COMPLETE, Restatement
from background_sampled_reference import SampledTwin
from background_target_reference import TARGET

pytestmark = pytest.mark.gpu

RESTATEMENT_TOL = 1e-12  # tests/test_background_gpu.py: a fixed-dt run against the restatement, of each value's scale
DT, STEPS = 1e-2, 8
LANES = 65


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module", params=bt.GPU_MODELS)
def zoo(request):
    """(name, artefact with its background object built): six fuzzed models, three of them cse=True, and the non-diagonal ones"""
    art = bt.device_artifact(request.param)
    art.ensure_background()
    return request.param, art


def test_device_model_function_lane_by_lane(bg, zoo):
    """B = 257 (a 256-lane workgroup and one lane), every lane its own parameter row.  Row 0's H is the Friedmann constraint of the
    derivation in 40-digit arithmetic to 1e-14; 8 fixed steps of rk4 and of rkf equal the restatement run on the INDEPENDENT
    right-hand side to 1e-12 of each value's scale: the symbolic stage, the emitter, hipcc's build, the pow rewrites and the stride of
    the parameter rows are all inside this comparison."""
    name, art = zoo
    z = bt.zoo_model(name)
    init, pars = bt.batch(name)
    assert pars.shape == (257, art.n_parameters) and art.symbol_dictionary == bt.host_artifact(name).symbol_dictionary
    energy = bt.point_function(z.model.coordinates, z.model.coordinate_tangents, bt._derivation(z.model)[1:], art.symbol_dictionary, modules="mpmath")
    with mpmath.workdps(40):
        h0 = np.array([float(mpmath.sqrt((V + kin / 2) / 3)) for V, kin in (energy(*[mpmath.mpf(float(v)) for v in pt], [mpmath.mpf(float(v)) for v in p]) for pt, p in zip(init, pars))])
    eom = bt.truth_rhs(name)
    for solver in ("rk4", "rkf"):
        sol = bg.solve_eom_batch(art, pars, STEPS + 1, init[:, :2], init[:, 2:], solver=solver, dt=DT)
        assert np.all(sol.status == COMPLETE) and np.all(sol.last_row == STEPS)
        rel_h0 = np.max(np.abs(sol.states[:, 0, 4] - h0) / h0)
        got = np.concatenate([sol.states, sol.N[..., None], sol.t[..., None]], axis=2)
        want = np.array([Restatement(eom, pars[k]).solve(init[k], STEPS + 1, solver, dt=DT)[0] for k in range(257)])
        rel = np.abs(got - want) / bt.scale_of(want)
        print(f"{name} {solver}: H0 against the 40-digit derivation {rel_h0:.3e}; GPU against the restatement on the independent right-hand side {rel.max():.3e} (lane {int(np.argmax(rel.max(axis=(1, 2))))})")
        assert rel_h0 <= 1e-14, rel_h0
        assert rel.max() <= RESTATEMENT_TOL, rel.max()


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_convergence_order_on_the_device(bg, zoo, solver):
    """B = 65 (a wavefront and one lane), per-lane parameter rows, fixed dt = 1/n to T = 1: halving dt cuts the end-point error
    against DOP853 by >= 14 on every lane -- the lanes for which tests/test_background_truth.py shows it on the host build."""
    name, art = zoo
    init, pars = (a[:LANES] for a in bt.batch(name))

    def solve(n):
        sol = bg.solve_eom_batch(art, pars, n + 1, init[:, :2], init[:, 2:], solver=solver, dt=bt.T_ORDER / n)
        assert np.all(sol.status == COMPLETE)
        return np.concatenate([sol.states[:, -1], sol.N[:, -1:], sol.t[:, -1:]], axis=1)

    e40, ratios = bt.order_ratios(solve, name)
    print(f"{name} {solver}: error at n = 40 {e40.min():.2e} .. {e40.max():.2e}, ratios {ratios.min():.2f} .. {ratios.max():.2f}")
    assert ratios.min() >= 14.0, (ratios.min(), int(np.argmin(ratios)))


@pytest.mark.parametrize("at", ["t", "N"])
@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_adaptive_runs_against_truth(bg, zoo, solver, at):
    """solve_eom_sampled at its default max_err, four samples up to T = 2, B = 65: every lane emits every sample, and its error
    against DOP853 at the returned t is at most twice that of the host build of the same stepper with FMA contraction on the same
    lane, plus 1e-11 (the bound on the truth's own error); the factor allows an accept / reject decision to fall the other way
    under OCML's pow."""
    name, art = zoo
    init, pars = (a[:LANES] for a in bt.batch(name))
    truth = bt.truths(name, LANES, bt.T_ADAPTIVE)
    samples = bt.samples_for(name, at)
    sol = bg.solve_eom_sampled(art, pars, samples, init[:, :2], init[:, 2:], solver=solver, at=at, stop_at_end=False)
    assert np.all(sol.status == TARGET) and np.all(sol.n_stored == 4), (sol.status, sol.n_stored)
    got = np.concatenate([sol.states, sol.N[..., None], sol.t[..., None]], axis=2)
    assert np.isfinite(got).all() and np.all(sol.t <= bt.T_ADAPTIVE * (1 + 1e-12))
    twin = SampledTwin(bt.host_artifact(name), contract="fast")
    err_gpu, err_host = np.empty(LANES), np.empty(LANES)
    for k in range(LANES):
        out, meta = twin.solve(pars[k], init[k], samples, 100_000, solver, max_err=1e-8, at=at, stop_at_end=False)
        assert meta["status"] == TARGET
        err_gpu[k], err_host[k] = bt.error_against_truth(got[k], truth[k]), bt.error_against_truth(out, truth[k])
    print(f"{name} {solver} at {at}: error against the truth, GPU {err_gpu.max():.3e}, host build {err_host.max():.3e}, worst GPU-to-host ratio {np.max(err_gpu / err_host):.6f}")
    assert np.all(err_gpu <= 2.0 * err_host + bt.TRUTH_TOL), (int(np.argmax(err_gpu / err_host)), err_gpu.max(), err_host.max())


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_state_at_efolds_on_a_nondiagonal_model(bg, solver):
    """G_01 != 0: the state located at N = the second sample is the sampled run's, bit for bit."""
    name = "skew"
    art = bt.device_artifact(name)
    init, pars = (a[:LANES] for a in bt.batch(name))
    samples = bt.samples_for(name, "N")
    sol = bg.solve_eom_sampled(art, pars, samples, init[:, :2], init[:, 2:], solver=solver, stop_at_end=False)
    one = bg.state_at_efolds(art, pars, init[:, :2], init[:, 2:], samples[1], solver=solver, stop_at_end=False)
    assert np.all(sol.status == TARGET) and np.all(one.status == TARGET) and np.all(one.N == samples[1]) and np.all(sol.N[:, 1] == samples[1])
    assert np.array_equal(sol.states[:, 1], one.state) and np.array_equal(sol.t[:, 1], one.t) and np.array_equal(sol.eps_H[:, 1], one.eps_H)
    assert np.isfinite(one.state).all()
