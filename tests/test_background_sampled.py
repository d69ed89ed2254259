"""Samples without a GPU: the host build of the sampled stepper (csrc/inflx_background.h: inflx_bg_step_sampled) against the analytic
power-law attractor and against the target stepper run once per sample, its edge cases, and the argument checks of
``solve_eom_sampled``."""

import math

import numpy as np
import pytest

import workloads
from background_reference import COMPLETE, ENDED, BackgroundTwin, power_law_artifact, power_law_exact, power_law_init
from background_sampled_reference import EGNO_SEEDS, HEAVY_SAMPLES, SampledTwin
from background_target_reference import TARGET, TargetTwin

HYPER_INIT = np.array([3.0, 0.5, 0.0, 0.1])


@pytest.fixture(scope="module")
def power_law():
    art, p = power_law_artifact()
    return art, p, SampledTwin(art)


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return spec.args, BackgroundTwin(art), TargetTwin(art), SampledTwin(art)


N_SAMPLES = np.array([0.37, 1.1, 2.0])
T_SAMPLES = np.exp(N_SAMPLES / 8.0) - 1.0  # the same points in t: N = p ln(1 + t), p = 8


def _power_law_errors(out):
    """error of every sample's state, N and t against the attractor at the sample's own t, relative with a floor of 1"""
    exact = np.concatenate([power_law_exact(T_SAMPLES), T_SAMPLES[:, None]], axis=1)
    return np.max(np.abs(out[:, :7] - exact) / np.maximum(np.abs(exact), 1.0), axis=1)


@pytest.mark.parametrize("at", ["N", "t"])
@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_samples_are_fourth_order(power_law, method, at):
    """Fixed dt = 2/n: halving dt cuts the error of every sample by >= 14 (fourth order: 16), the bound of
    test_background_target.py::test_located_state_is_fourth_order."""
    art, p, twin = power_law
    samples = N_SAMPLES if at == "N" else T_SAMPLES
    errs = []
    for n in (40, 80):
        out, meta = twin.solve(p, power_law_init(), samples, 10_000, method, dt=2.0 / n, at=at)
        assert meta["status"] == TARGET and meta["n_stored"] == 3
        assert np.array_equal(out[:, 5 if at == "N" else 6], samples)  # the sampled variable is the sample exactly
        errs.append(_power_law_errors(out))
    ratios = errs[0] / errs[1]
    print(f"{method} at {at}: errors {errs[0]} {errs[1]}, ratios {ratios}")
    assert np.all(ratios >= 14.0), (errs, ratios)


@pytest.mark.parametrize("dt", [None, 2e-3])
@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_same_steps_as_the_ordinary_run(hyper, method, dt):
    """Every emitted sample is, bit for bit, what the target stepper returns when run to that one target: the same accepted step, the
    same located state, t and epsilon_H.  The last samples lie beyond the end of inflation (adaptive) or beyond max_steps (fixed dt)."""
    p, plain, target, twin = hyper
    max_steps = 100_000 if dt is None else 600
    _, end = target.solve(p, HYPER_INIT, 1e3, max_steps, method, max_err=1e-9, dt=dt, stop_at_end=True)
    rows, _ = plain.solve(p, HYPER_INIT, end["accepted"] + 1, method, max_err=1e-9, dt=dt, stop_at_end=True)
    reach = end["N_end"] if dt is None else rows[end["accepted"], 5]
    samples = np.concatenate([[0.0], reach * np.array([1e-6, 0.01, 0.013, 0.2, 0.5, 0.77, 0.999, 1.0, 1.001, 1.5])])
    out, meta = twin.solve(p, HYPER_INIT, samples, max_steps, method, max_err=1e-9, dt=dt, stop_at_end=True)
    assert meta["status"] == (ENDED if dt is None else COMPLETE) and meta["n_stored"] == 9 and meta["accepted"] == end["accepted"]
    assert np.isnan(out[9:]).all() and np.isfinite(out[:9]).all()
    if dt is None:
        assert meta["N_end"] == end["N_end"]
    for k in range(9):
        want, tm = target.solve(p, HYPER_INIT, samples[k], max_steps, method, max_err=1e-9, dt=dt, stop_at_end=True)
        assert tm["status"] == TARGET and tm["accepted"] == meta["step_of"][k], k
        assert np.array_equal(out[k], want), (k, out[k], want)
    for k in (9, 10):  # not emitted: the single-target run does not reach them either
        _, tm = target.solve(p, HYPER_INIT, samples[k], max_steps, method, max_err=1e-9, dt=dt, stop_at_end=True)
        assert tm["status"] == meta["status"], k


def test_time_samples_lie_on_the_ordinary_runs_steps(hyper):
    """at="t": theta = (t_s - t0) / h in the ordinary run's step [t0, t0 + h] that contains t_s, t = t_s exactly; a sample at a row's
    own t is that row (theta = 1) to rounding: t1 = fl(t0 + h), so theta is off 1 by <= ulp(t1) / (2 h) and the state by that times
    h |f| ~ 1e-16 t1 |f|, plus the rounding of the four basis terms; 1e-14 is ten times that for t1 ~ 10, |f| ~ 1."""
    p, plain, _, twin = hyper
    rows, _ = plain.solve(p, HYPER_INIT, 300, "rkf", max_err=1e-9)
    samples = np.array([0.5 * rows[150, 6], rows[200, 6], 0.5 * (rows[250, 6] + rows[251, 6])])
    out, meta = twin.solve(p, HYPER_INIT, samples, 10_000, "rkf", max_err=1e-9, at="t")
    assert meta["status"] == TARGET and np.array_equal(out[:, 6], samples) and list(meta["step_of"][1:]) == [200, 251]
    assert np.max(np.abs(out[1, :6] - rows[200, :6]) / np.maximum(np.abs(rows[200, :6]), 1.0)) <= 1e-14
    assert rows[250, 5] < out[2, 5] < rows[251, 5]


def test_edge_cases(hyper):
    p, plain, target, twin = hyper
    first, _ = plain.solve(p, HYPER_INIT, 2, "rkf", dt=0.5)
    # a sample at 0 is the initial state, emitted in init; three samples inside the one step that follows
    samples = np.concatenate([[0.0], first[1, 5] * np.array([0.25, 0.5, 0.75])])
    for at, pts in (("N", samples), ("t", np.array([0.0, 0.125, 0.25, 0.375]))):
        out, meta = twin.solve(p, HYPER_INIT, pts, 100, "rkf", dt=0.5, stop_at_end=True, at=at)
        assert meta["status"] == TARGET and meta["n_stored"] == 4 and meta["accepted"] == 1 and list(meta["step_of"]) == [0, 1, 1, 1]
        assert np.array_equal(out[0, :7], first[0]) and math.isfinite(out[0, 7])
        assert np.all(np.diff(out[:, 5]) > 0) and np.all(np.diff(out[:, 6]) > 0) and np.all(out[:, 5:7] < first[1, 5:7])
    # only a sample at 0: reached in init
    out, meta = twin.solve(p, HYPER_INIT, [0.0], 100, stop_at_end=True)
    assert meta["status"] == TARGET and meta["accepted"] == 0 and meta["n_stored"] == 1
    # already past the end of inflation: ends in init and emits only a sample at 0
    past = [3.0, 0.0, 5.0, 0.0]
    out, meta = twin.solve(p, past, [0.0, 0.5], 100, stop_at_end=True)
    assert meta["status"] == ENDED and meta["N_end"] == 0.0 and meta["n_stored"] == 1 and meta["accepted"] == 0
    assert np.isfinite(out[0]).all() and out[0, 7] >= 1.0 and np.isnan(out[1]).all()
    out, meta = twin.solve(p, past, [0.5], 100, stop_at_end=True)
    assert meta["status"] == ENDED and meta["n_stored"] == 0 and np.isnan(out).all()
    # max_steps run out: COMPLETE with the samples passed so far
    rows, _ = plain.solve(p, HYPER_INIT, 21, "rkf", dt=1e-2)
    out, meta = twin.solve(p, HYPER_INIT, [0.5 * rows[20, 5], 2.0 * rows[20, 5], 1e3], 20, "rkf", dt=1e-2, stop_at_end=True)
    assert meta["status"] == COMPLETE and meta["accepted"] == 20 and meta["n_stored"] == 1
    assert np.isfinite(out[0]).all() and np.isnan(out[1:]).all()


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_samples_on_both_sides_of_the_end_of_inflation(hyper, method):
    """epsilon_H = 1 inside a step [N0, N1]: a sample in [N0, N_end] is emitted, one in (N_end, N1] is not, and the lane is ENDED --
    in t as well, where the end is at t0 + f h with N_end's fraction f."""
    p, plain, target, twin = hyper
    _, end = target.solve(p, HYPER_INIT, 1e3, 100_000, method, max_err=1e-9, stop_at_end=True)
    rows, _ = plain.solve(p, HYPER_INIT, end["accepted"] + 1, method, max_err=1e-9, stop_at_end=True)
    (n0, t0), (n1, t1), n_end = rows[-2, 5:7], rows[-1, 5:7], end["N_end"]
    assert n0 < n_end < n1
    f = (n_end - n0) / (n1 - n0)
    for at, pts in (("N", [0.5 * (n0 + n_end), n_end, 0.5 * (n_end + n1), n1]),
                    ("t", [t0 + 0.5 * f * (t1 - t0), t0 + 0.999 * f * (t1 - t0), t0 + 0.5 * (1.0 + f) * (t1 - t0), t1])):  # fmt: skip
        out, meta = twin.solve(p, HYPER_INIT, pts, 100_000, method, max_err=1e-9, stop_at_end=True, at=at)
        assert meta["status"] == ENDED and meta["N_end"] == n_end and meta["n_stored"] == 2 and meta["accepted"] == end["accepted"]
        assert list(meta["step_of"][:2]) == [end["accepted"]] * 2
        assert np.isfinite(out[:2]).all() and np.isnan(out[2:]).all()
        assert out[0, 7] < out[1, 7] and abs(out[1, 7] - 1.0) <= 1e-2  # epsilon_H rises to 1 (up to the interpolation of N_end)
        # without stop_at_end the same step emits all four
        out, meta = twin.solve(p, HYPER_INIT, pts, 100_000, method, max_err=1e-9, stop_at_end=False, at=at)
        assert meta["status"] == TARGET and meta["n_stored"] == 4 and np.isfinite(out).all()
    # the end of inflation itself as the last sample is reached: TARGET
    out, meta = twin.solve(p, HYPER_INIT, [0.5 * n_end, n_end], 100_000, method, max_err=1e-9, stop_at_end=True)
    assert meta["status"] == TARGET and meta["n_stored"] == 2


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as fh:
            return any(line.startswith("flags") and " fma " in line + " " for line in fh)
    except OSError:
        return False


@pytest.mark.skipif(not _cpu_has_fma(), reason="needs a CPU with FMA instructions")
def test_egno_lanes_of_the_gpu_test_are_well_conditioned():
    """The lanes that test_background_sampled_gpu.py runs on EGNO: the host build with contraction on and the one with contraction off
    (the kernel and the host build differ in just that) agree within 1e-13, a tenth of RESTATEMENT_TOL["egno"], at every sample."""
    from test_background import initial_state

    spec, art = workloads.artifact_for("egno")
    off, fused = SampledTwin(art), SampledTwin(art, contract="fast")
    assert len(set(EGNO_SEEDS)) == 64
    worst = 0.0
    for seed in EGNO_SEEDS:
        init = initial_state("egno", seed=seed)
        for method in ("rk4", "rkf"):
            a, b = (twin.solve(spec.args, init, HEAVY_SAMPLES, 50, method=method, dt=1e-3, at="t")[0] for twin in (off, fused))
            assert np.isfinite(a).all() and np.isfinite(b).all()
            worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-3))))
    print(f"EGNO, contraction on vs off on the host: max relative difference {worst:.3e}")
    assert worst <= 1e-13, worst


def test_public_names():
    from inflatox_amd import _native, background

    assert {"solve_eom_sampled", "SampledSolution"} <= set(background.__all__)
    assert background.SampledSolution._fields == ("states", "t", "N", "eps_H", "n_stored", "N_end", "status")
    assert _native.EOM_SAMPLE_T == 4 and callable(_native.InflatoxDevLib.solve_eom_sampled)


def test_bad_arguments_raise_before_the_device(monkeypatch):
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = np.zeros((3, 2)) + 2.0, np.zeros((3, 2))
    good = [0.0, 0.5, 1.0]
    shape, value = _native.InflatoxShapeError, ValueError
    ses = background.solve_eom_sampled
    for bad in ([0.5, 0.2, 1.0], [0.5, 0.5], [-0.1, 0.5], [0.1, float("nan")], [0.1, float("inf")], [], "abc"):
        with pytest.raises(value):
            ses(art, p, bad, x, v)
    with pytest.raises(shape):
        ses(art, p, [[0.1, 0.2]], x, v)
    for at in ("n", "efolds", None):
        with pytest.raises(value):
            ses(art, p, good, x, v, at=at)
    with pytest.raises(shape):
        ses(art, p[:2], good, x, v)
    with pytest.raises(shape):
        ses(art, np.zeros((2, p.size)), good, x, v)
    with pytest.raises(shape):
        ses(art, p, good, x, v[:2])
    with pytest.raises(shape):
        ses(art, p, good, np.zeros((3, 3)), np.zeros((3, 3)))
    for steps in (0, -1, 2.5):
        with pytest.raises(value):
            ses(art, p, good, x, v, max_steps=steps)
    for err in (0.0, -1e-6, float("nan")):
        with pytest.raises(value):
            ses(art, p, good, x, v, max_err=err)
    with pytest.raises(value):
        ses(art, p, good, x, v, solver="euler")
    with pytest.raises(value):
        ses(art, p, good, x, v, dt=0.0)
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    with pytest.raises(shape):
        ses(three, p, good, x, v)
