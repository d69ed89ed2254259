"""A target on N without a GPU: the host build of the target stepper (csrc/inflx_background.h: inflx_bg_step_target) against the
analytic power-law attractor and against a numpy Hermite evaluation over the ordinary run's rows, its edge cases, and the argument
checks of ``state_at_efolds`` and ``horizon_exit_map``."""

import math

import numpy as np
import pytest

import workloads
from background_reference import COMPLETE, ENDED, BackgroundTwin, power_law_artifact, power_law_exact, power_law_init
from background_target_reference import TARGET, TargetTwin, hermite_state_at, rhs


@pytest.fixture(scope="module")
def power_law():
    art, p = power_law_artifact()
    return art, p, TargetTwin(art)


def _power_law_error(out, n_target):
    """error of the located state and t against the attractor at N = n_target, relative with a floor of 1"""
    t_exact = math.exp(n_target / 8.0) - 1.0  # N = p ln(1 + t), p = 8
    exact = np.append(power_law_exact(t_exact), t_exact)
    return float(np.max(np.abs(out[:7] - exact) / np.maximum(np.abs(exact), 1.0)))


@pytest.mark.parametrize("n_target", [0.37, 2.0])
@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_located_state_is_fourth_order(power_law, method, n_target):
    """Fixed dt = 2/n: halving dt cuts the error of the located state by >= 14 (fourth order: 16) -- a linear interpolant does not."""
    art, p, twin = power_law
    errs = []
    for n in (40, 80):
        out, meta = twin.solve(p, power_law_init(), n_target, 10_000, method, dt=2.0 / n)
        assert meta["status"] == TARGET and out[5] == n_target
        errs.append(_power_law_error(out, n_target))
    print(f"{method} N_t = {n_target}: errors {errs[0]:.3e} {errs[1]:.3e}, ratio {errs[0] / errs[1]:.1f}")
    assert errs[0] / errs[1] >= 14.0, errs


@pytest.mark.parametrize("n_target", [0.37, 2.0, 8.0])
@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_adaptive_located_state_on_the_power_law(power_law, method, n_target):
    art, p, twin = power_law
    out, meta = twin.solve(p, power_law_init(), n_target, 100_000, method, max_err=1e-10)
    assert meta["status"] == TARGET and out[5] == n_target
    err = _power_law_error(out, n_target)
    print(f"{method} N_t = {n_target}: error {err:.3e} after {meta['accepted']} steps")
    assert err <= 1e-8, err
    # epsilon_H of the attractor is 1/p
    assert abs(out[7] - 1.0 / 8.0) <= 1e-8


@pytest.mark.parametrize("dt", [None, 2e-3])
@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_stops_in_the_ordinary_runs_step(method, dt):
    """The lane takes the steps of the ordinary run (substeps = 1) and stops in the step from row k to row k + 1, k the last row with
    N[k] < N_t; its located state is the Hermite interpolant built from those two rows and the model function, evaluated in numpy."""
    spec, art = workloads.artifact_for("hyperbolic")
    plain, twin = BackgroundTwin(art), TargetTwin(art)
    init = np.array([3.0, 0.5, 0.0, 0.1])
    rows, meta = plain.solve(spec.args, init, 400, method, max_err=1e-9, dt=dt)
    assert meta["status"] == COMPLETE
    worst = 0.0
    for n_target in (0.3 * rows[-1, 5], 0.77 * rows[-1, 5], rows[200, 5]):  # (the last: N_t = a row's N exactly, theta = 1)
        k = int(np.flatnonzero(rows[:, 5] < n_target)[-1])
        out, tm = twin.solve(spec.args, init, n_target, 10_000, method, max_err=1e-9, dt=dt)
        assert tm["status"] == TARGET and tm["accepted"] == k + 1
        y0, y1 = rows[k, :6], rows[k + 1, :6]
        h = rows[k + 1, 6] - rows[k, 6]
        e = plain.eom(spec.args, np.array([y0[:4], y1[:4]]))
        theta, want = hermite_state_at(y0, rhs(e[0], y0), y1, rhs(e[1], y1), h, n_target)
        want = np.append(want, rows[k, 6] + theta * h)
        assert rows[k, 6] <= out[6] <= rows[k + 1, 6]
        worst = max(worst, float(np.max(np.abs(out[:7] - want) / np.maximum(np.abs(want), 1.0))))
        eps = 0.5 * plain.eom(spec.args, out[None, :4])[0, 3] / out[4] ** 2
        assert out[7] == eps
    print(f"{method} dt = {dt}: located state vs numpy Hermite, worst {worst:.3e}")
    # rounding only (h is t[k+1] - t[k] here and the step size itself in the stepper; the root by numpy.roots).  Measured with the
    # host build: rk4 3.3e-16 (adaptive) and 1.1e-16 (fixed dt), rkf 6.1e-16 and 1.6e-16; the bound is 16 times the worst
    assert worst <= 1e-14, worst


def test_edge_cases():
    spec, art = workloads.artifact_for("hyperbolic")
    twin = TargetTwin(art)
    init = np.array([3.0, 0.5, 0.0, 0.1])
    first, _ = BackgroundTwin(art).solve(spec.args, init, 1)
    # a target <= 0 is reached by the initial state, in init
    for n_target in (0.0, -1.5):
        out, meta = twin.solve(spec.args, init, n_target, 100, stop_at_end=True)
        assert meta["status"] == TARGET and meta["accepted"] == 0
        assert np.array_equal(out[:7], first[0]) and math.isfinite(out[7])
    # a target beyond the end of inflation: ENDED, with N_end
    out, meta = twin.solve(spec.args, init, 1e3, 100_000, stop_at_end=True)
    assert meta["status"] == ENDED and math.isfinite(meta["N_end"]) and 0 < meta["N_end"] < 1e3 and math.isnan(out[7])
    # the end of inflation itself is a target that is reached: epsilon_H = 1 there, up to the interpolation of N_end
    out2, meta2 = twin.solve(spec.args, init, meta["N_end"], 100_000, stop_at_end=True)
    assert meta2["status"] == TARGET and meta2["accepted"] == meta["accepted"] and abs(out2[7] - 1.0) <= 1e-2
    # a target that max_steps do not reach: the lane is still running (COMPLETE)
    out, meta = twin.solve(spec.args, init, 1e3, 20, stop_at_end=True)
    assert meta["status"] == COMPLETE and meta["accepted"] == 20 and math.isnan(out[7])
    # already past the end of inflation: ends in init, whatever the target
    out, meta = twin.solve(spec.args, [3.0, 0.0, 5.0, 0.0], -1.0, 100, stop_at_end=True)
    assert meta["status"] == ENDED and meta["N_end"] == 0.0


def test_status_constants():
    from inflatox_amd import _native, background

    assert background.TARGET == TARGET == 5 and background.TARGET in background.STATUS
    assert background.ENDED_SHORT in background.STATUS and background.ENDED_SHORT not in range(6)
    assert {"state_at_efolds", "horizon_exit_map"} <= set(background.__all__)
    assert callable(_native.InflatoxDevLib.solve_eom_to_efolds)


def test_bad_arguments_raise_before_the_device(monkeypatch):
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = np.zeros((3, 2)) + 2.0, np.zeros((3, 2))
    ss = [[1.0, 5.0], [-1.0, 1.0]]
    shape, value = _native.InflatoxShapeError, ValueError
    sae, hem = background.state_at_efolds, background.horizon_exit_map
    with pytest.raises(shape):
        sae(art, p[:2], x, v, 1.0)
    with pytest.raises(shape):
        sae(art, np.zeros((2, p.size)), x, v, 1.0)
    with pytest.raises(shape):
        sae(art, p, x, v[:2], 1.0)
    with pytest.raises(shape):
        sae(art, p, np.zeros((3, 3)), np.zeros((3, 3)), 1.0)
    with pytest.raises(shape):
        sae(art, p, x, v, [1.0, 2.0])
    with pytest.raises(shape):
        sae(art, p, x, v, np.ones((3, 1)))
    for bad in (float("nan"), float("inf"), [1.0, float("nan"), 2.0]):
        with pytest.raises(value):
            sae(art, p, x, v, bad)
    for steps in (0, -1, 2.5):
        with pytest.raises(value):
            sae(art, p, x, v, 1.0, max_steps=steps)
    for err in (0.0, -1e-6, float("nan")):
        with pytest.raises(value):
            sae(art, p, x, v, 1.0, max_err=err)
    with pytest.raises(value):
        sae(art, p, x, v, 1.0, solver="euler")
    with pytest.raises(value):
        sae(art, p, x, v, 1.0, dt=0.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(value):
            hem(art, p, ss, 4, 4, N_star=bad)
    with pytest.raises(shape):
        hem(art, p, [0, 1, 0], 4, 4)
    with pytest.raises(shape):
        hem(art, p[:2], ss, 4, 4)
    with pytest.raises(shape):
        hem(art, p, ss, 4, 4, derivatives_init=(0.0, 0.0, 0.0))
    with pytest.raises(value):
        hem(art, p, ss, 0, 4)
    with pytest.raises(value):
        hem(art, p, ss, 4, 4, max_steps=0)
    with pytest.raises(value):
        hem(art, p, ss, 4, 4, max_err=0.0)
    with pytest.raises(value):
        hem(art, p, ss, 4, 4, solver="euler")
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    with pytest.raises(shape):
        sae(three, p, x, v, 1.0)
    with pytest.raises(shape):
        hem(three, p, ss, 4, 4)
