"""Samples on the GPU (inflatox_amd.background.solve_eom_sampled): bit-equality with state_at_efolds sample by sample, launch
boundaries and several samples per step against the host build of the same stepper, lane chunks, time samples on the analytic
power-law attractor, the refusal of a background object of the previous layout, and the heavy-register models."""

import os
import subprocess

import numpy as np
import pytest

import workloads
from background_reference import COMPLETE, ENDED, power_law_artifact, power_law_exact, power_law_init
from background_sampled_reference import EGNO_SEEDS, HEAVY_SAMPLES, SampledTwin
from background_target_reference import TARGET
from test_background import initial_state
from test_background_gpu import RESTATEMENT_TOL, _hyper_batch

pytestmark = pytest.mark.gpu

FIELDS = ("states", "t", "N", "eps_H", "n_stored", "N_end", "status")


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


def _planes(sol):
    """(B, S, 8): y[0..4], N, t, epsilon_H -- the twin's layout"""
    return np.concatenate([sol.states, sol.N[..., None], sol.t[..., None], sol.eps_H[..., None]], axis=2)


def _against_the_twin(sol, twin, p, x, v, samples, max_steps, tol, **kw):
    """Every lane against the host build of the stepper: the same status, samples emitted and NaN pattern, N_end and every emitted
    value within `tol`, relative with a floor of 1e-3 (the comparison of test_background_target_gpu.py).  Returns the worst figure and
    the twin's step_of rows."""
    got = _planes(sol)
    worst, steps = 0.0, []
    for k in range(x.shape[0]):
        want, meta = twin.solve(p, np.concatenate([x[k], v[k]]), samples, max_steps, **kw)
        assert sol.status[k] == meta["status"] and sol.n_stored[k] == meta["n_stored"], (k, sol.status[k], meta)
        assert np.array_equal(np.isnan(got[k]), np.isnan(want)), k
        n = meta["n_stored"]
        assert np.isfinite(want[:n]).all() and np.isnan(want[n:]).all()
        if n:
            worst = max(worst, float(np.max(np.abs(got[k, :n] - want[:n]) / np.maximum(np.abs(want[:n]), 1e-3))))
        if meta["status"] == ENDED:
            assert abs(sol.N_end[k] - meta["N_end"]) <= tol * max(meta["N_end"], 1e-3)
        else:
            assert np.isnan(sol.N_end[k])
        steps.append(meta["step_of"])
    return worst, np.array(steps)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_bit_equal_to_state_at_efolds(bg, solver):
    """B = 96 (one and a half wavefronts), S = 7, adaptive, stop_at_end: sample s of every lane is state_at_efolds with the target
    samples[s] bit for bit where it was emitted, and that call ENDED with the same N_end where it was not."""
    spec, art = workloads.artifact_for("hyperbolic")
    x, v = _hyper_batch(96)
    samples = np.array([0.02, 0.1, 0.25, 0.5, 0.9, 1.4, 2.5])
    sol = bg.solve_eom_sampled(art, spec.args, samples, x, v, solver=solver)
    assert sol.states.shape == (96, 7, 5) and sol.t.shape == sol.N.shape == sol.eps_H.shape == (96, 7)
    assert sol.states.base is sol.t.base is sol.N.base is sol.eps_H.base is not None and sol.n_stored.dtype == np.uint32  # views of one array
    assert np.isin(sol.status, (TARGET, ENDED)).all() and (sol.status == TARGET).any() and (sol.status == ENDED).any(), np.bincount(sol.status)
    emitted = np.arange(7)[None, :] < sol.n_stored[:, None]
    assert np.array_equal(emitted, ~np.isnan(sol.N)) and np.array_equal(sol.status == TARGET, sol.n_stored == 7)
    assert np.array_equal(np.isnan(sol.N_end), sol.status == TARGET)
    assert 0 < emitted[:, 3].sum() < 96  # both outcomes inside one sample
    for s in range(7):
        one = bg.state_at_efolds(art, spec.args, x, v, samples[s], solver=solver)
        e = emitted[:, s]
        assert np.array_equal(one.status == TARGET, e) and np.all(one.status[~e] == ENDED)
        assert np.all(sol.N[e, s] == samples[s])
        assert np.array_equal(sol.states[e, s], one.state[e]) and np.array_equal(sol.t[e, s], one.t[e]) and np.array_equal(sol.eps_H[e, s], one.eps_H[e])
        assert np.array_equal(sol.N_end[~e], one.N_end[~e]) and np.isfinite(one.N_end[~e]).all()
        assert np.isnan(sol.states[~e, s]).all() and np.isnan(sol.t[~e, s]).all() and np.isnan(sol.eps_H[~e, s]).all()


@pytest.mark.parametrize("at", ["N", "t"])
def test_launch_boundaries_and_samples_in_one_step(bg, at):
    """Fixed dt = 1e-3: more than 256 accepted steps (a launch) lie between two samples, and 1000 steps do not reach the last one;
    then dt = 0.5 with three samples inside the first step.  Against the host build of the stepper, which differs by FMA contraction
    only."""
    spec, art = workloads.artifact_for("hyperbolic")
    twin = SampledTwin(art)
    x, v = _hyper_batch(8, seed=3)
    tol = RESTATEMENT_TOL["hyperbolic"]
    samples = np.array([0.05, 0.4, 0.9, 5.0]) if at == "t" else np.array([0.02, 0.15, 0.4, 50.0])
    sol = bg.solve_eom_sampled(art, spec.args, samples, x, v, max_steps=1000, solver="rk4", at=at, dt=1e-3)
    worst, steps = _against_the_twin(sol, twin, spec.args, x, v, samples, 1000, tol, method="rk4", dt=1e-3, stop_at_end=True, at=at)
    print(f"at {at}, dt = 1e-3: GPU vs host stepper, max relative difference {worst:.3e}; emitted in steps {steps[0]}")
    assert worst <= tol, worst
    gaps = np.diff(steps[:, :3], axis=1)
    # (one of the eight lanes starts past the end of inflation and emits nothing; two end before the third sample)
    assert np.nanmax(gaps) > 256 and (sol.status == COMPLETE).any() and (sol.n_stored >= 2).sum() >= 6 and (sol.n_stored == 3).any()
    samples = np.array([0.125, 0.25, 0.375]) if at == "t" else np.array([1e-3, 2e-3, 3e-3])
    sol = bg.solve_eom_sampled(art, spec.args, samples, x, v, max_steps=10, solver="rkf", at=at, dt=0.5)
    worst, steps = _against_the_twin(sol, twin, spec.args, x, v, samples, 10, tol, method="rkf", dt=0.5, stop_at_end=True, at=at)
    print(f"at {at}, dt = 0.5: GPU vs host stepper, max relative difference {worst:.3e}")
    assert worst <= tol, worst
    assert (steps == 1).all(axis=1).any(), steps


def test_edge_cases(bg):
    spec, art = workloads.artifact_for("hyperbolic")
    x, v = np.array([[3.0, 0.5], [3.0, 0.0]]), np.array([[0.0, 0.1], [5.0, 0.0]])  # (the second starts past the end of inflation)
    sol = bg.solve_eom_sampled(art, spec.args, [0.0, 0.5, 1e3], x, v)
    assert list(sol.status) == [ENDED, ENDED] and list(sol.n_stored) == [2, 1] and sol.N_end[1] == 0.0 and sol.N_end[0] > 0.5
    first = bg.solve_eom_batch(art, spec.args, 1, x, v)
    for k in (0, 1):  # a sample at 0: the initial state, t = 0
        assert np.array_equal(sol.states[k, 0], first.states[k, 0]) and sol.t[k, 0] == 0.0 and sol.N[k, 0] == 0.0 and np.isfinite(sol.eps_H[k, 0])
    assert sol.eps_H[1, 0] >= 1.0 and np.isnan(sol.states[1, 1:]).all() and np.isnan(sol.states[0, 2]).all() and sol.N[0, 1] == 0.5
    only = bg.solve_eom_sampled(art, spec.args, [0.0], x, v)
    assert list(only.status) == [TARGET, ENDED] and list(only.n_stored) == [1, 1]
    # max_steps run out first: 300 fixed steps (two launches, 256 + 44) reach t = 0.3
    short = bg.solve_eom_sampled(art, spec.args, [0.1, 0.2, 0.4], x[:1], v[:1], max_steps=300, solver="rk4", at="t", dt=1e-3)
    assert short.status[0] == COMPLETE and short.n_stored[0] == 2 and np.array_equal(short.t[0, :2], [0.1, 0.2]) and np.isnan(short.t[0, 2])


def test_lane_independence_and_lane_chunks(bg):
    """S = 64 samples are 64 x 8 doubles per lane, so the 256 MiB sample buffer holds 65 536 lanes: B = 65 541 takes two passes, and
    the second one's five lanes land behind the first one's in every plane of the result.  Bit for bit calls on a few lanes alone."""
    spec, art = workloads.artifact_for("hyperbolic")
    B = 65_536 + 5
    x, v = _hyper_batch(B, seed=8)
    samples = np.linspace(0.0, 4.5e-3, 64)
    kw = dict(max_steps=5, solver="rkf", at="t", dt=1e-3, stop_at_end=False)
    big = bg.solve_eom_sampled(art, spec.args, samples, x, v, **kw)
    assert np.all(big.status == TARGET) and np.all(big.n_stored == 64) and np.isfinite(big.states).all()
    assert np.array_equal(big.t, np.broadcast_to(samples, (B, 64)))
    for sl in (slice(0, 5), slice(65_534, 65_538), slice(B - 5, None)):
        small = bg.solve_eom_sampled(art, spec.args, samples, x[sl], v[sl], **kw)
        for f in FIELDS:
            assert np.array_equal(getattr(big, f)[sl], getattr(small, f), equal_nan=True), (sl, f)
    # lanes do not see each other: a permutation of the first 300 permutes the result
    perm = np.random.default_rng(1).permutation(300)
    shuffled = bg.solve_eom_sampled(art, spec.args, samples, x[perm], v[perm], **kw)
    for f in FIELDS:
        assert np.array_equal(getattr(big, f)[perm], getattr(shuffled, f), equal_nan=True), f


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_time_samples_on_the_power_law(bg, method):
    """at="t", adaptive, against the attractor with the bound of test_adaptive_located_state_on_the_power_law; N = p ln(1 + t)."""
    art, p = power_law_artifact()
    x0 = power_law_init()
    n_exact = np.array([0.37, 2.0, 8.0])
    samples = np.exp(n_exact / 8.0) - 1.0
    sol = bg.solve_eom_sampled(art, p, samples, x0[None, :2], x0[None, 2:], max_err=1e-10, solver=method, at="t")
    assert sol.status[0] == TARGET and sol.n_stored[0] == 3 and np.array_equal(sol.t[0], samples) and np.isnan(sol.N_end[0])
    exact = power_law_exact(samples)
    got = np.concatenate([sol.states[0], sol.N[0][:, None]], axis=1)
    errs = np.max(np.abs(got - exact) / np.maximum(np.abs(exact), 1.0), axis=1)
    n_err = np.abs(sol.N[0] - 8.0 * np.log1p(samples))
    print(f"{method}: errors {errs}, N errors {n_err}")
    assert errs.max() <= 1e-8 and n_err.max() <= 1e-8, (errs, n_err)
    assert np.max(np.abs(sol.eps_H[0] - 1.0 / 8.0)) <= 1e-8  # epsilon_H of the attractor is 1/p


def test_background_object_of_layout_3_is_refused():
    """A background object of the previous layout version (INFLX_BG_ABI = 3: no sampled kernels, no `samples` in the arguments) is
    refused by the new entry point."""
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".background"
    hdr, eom_hdr = stale + ".model.h", stale + ".eom.h"
    try:
        for path, text in ((hdr, header_text), (eom_hdr, art.eom_header_text())):
            with open(path, "w") as fh:
                fh.write(text)
        cmd = [hipcc_path(), *options, "-DINFLX_BG_ABI_VERSION=3", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', os.path.join(_CSRC, "inflx_background_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        init = np.array([power_law_init()])
        with pytest.raises(SystemError, match="does not belong"):
            lib.solve_eom_sampled(p, init, np.array([0.5]), 100, _native.EOM_RKF, 1e-6, 0.0, 0)
        lib.close()
    finally:
        for path in (stale, hdr, eom_hdr):
            if os.path.exists(path):
                os.remove(path)


@pytest.mark.parametrize("name", ["egno", "d5"])
def test_heavy_models(bg, name):
    """B = 64, S = 4 (one of them the initial state), 50 fixed steps: the kernels with the most registers against the host build.
    EGNO runs the 64 initial states at which the host build itself carries the rounding of an FMA within a tenth of the bound
    (background_sampled_reference.EGNO_SEEDS): from others, such as seed 34, contraction alone moves the host build by 2.8e-8."""
    spec, art = workloads.artifact_for(name)
    twin = SampledTwin(art)
    init = np.array([initial_state(name, seed=s) for s in (EGNO_SEEDS if name == "egno" else range(64))])
    if name == "d5":  # V ~ 1e-6: velocities of the same energy (with the box's own, a third of the lanes run into a non-finite point)
        init[:, 2:] *= 1e-3
    x, v = np.ascontiguousarray(init[:, :2]), np.ascontiguousarray(init[:, 2:])
    samples = np.array(HEAVY_SAMPLES)
    for solver in ("rk4", "rkf"):
        sol = bg.solve_eom_sampled(art, spec.args, samples, x, v, max_steps=50, solver=solver, at="t", dt=1e-3, stop_at_end=False)
        worst, _ = _against_the_twin(sol, twin, spec.args, x, v, samples, 50, RESTATEMENT_TOL[name], method=solver, dt=1e-3, stop_at_end=False, at="t")
        print(f"{name} {solver}: GPU vs host stepper, max relative difference {worst:.3e}; status {np.bincount(sol.status)}")
        assert np.all(sol.status == TARGET), sol.status
        assert worst <= RESTATEMENT_TOL[name], worst
