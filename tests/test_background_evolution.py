"""Spectra sampled along a mode's evolution on the host build (tests/evolution_twin.cpp compiles csrc/inflx_evolution.h for the CPU):
samples do not change the run and equal the runs that stop there, bit for bit; truth (b) at every sample; the shift; two samples inside
one step; what every stop status keeps; ``transfer_from_spectra`` and its cross-check with ``transfer_functions``; the surface and the
argument checks; and the stand-alone twin program under AddressSanitizer and UBSan.  The bounds against the truth are 1e-10 plus twice
the twin's own recorded error (profiles/background_evolution.json, written by ``python tests/evolution_reference.py``).

The hyperbolic example model is no zoo model, so ``modes_reference.zoo_lanes`` has no lanes for it: its 65 lanes are
``evolution_reference.hyper_lanes``, built the same way (kappa = H0 e^3) from ``modes_reference.hyper_states``."""

import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

import evolution_reference as er
import modes_reference as mo
import transfer_reference as tr
import workloads
from modes_reference import COMPLETE, ENDED, NONFINITE, TARGET

ROOT = er.ROOT
PLANES = [0, 1, 2, 19, 20, 21]  # what a sample keeps of the 22 values


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return np.asarray(spec.args, dtype=np.float64), er.twin_for("hyperbolic"), er.modes_twin_for("hyperbolic")


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", er.CPU_MODELS)
def test_samples_do_not_change_the_run(name, solver):
    """65 lanes, five samples at 0, 1/4, 1/2, 3/4 and 1 x the target: the final 22 planes, N_end, the status and the accepted steps are
    those of the lane without samples, bit for bit; every sample's six values are the planes (0, 1, 2, 19, 20, 21) of the run whose
    target is that sample, bit for bit -- the last sample, the target itself, among them; the sample at 0 is the vacuum."""
    init, pars, kappa, target = er.lanes_of(name)
    pts = er.samples_of(name)
    assert pts[0] == 0.0 and pts[-1] == target and init.shape == (er.LANES, 4)
    got = er.twin_for(name).lanes(pars, init, kappa, target, 0.0, pts, solver=solver, stop_at_end=False)
    plain = er.modes_twin_for(name).lanes(pars, init, kappa, target, solver=solver, stop_at_end=False)
    assert np.all(got.status == TARGET) and np.array_equal(got.status, plain.status) and np.array_equal(got.accepted, plain.accepted)
    assert np.array_equal(got.out, plain.out) and np.array_equal(got.N_end, plain.N_end, equal_nan=True) and np.array_equal(got.final, plain.final)
    assert np.all(got.cursor == pts.size) and np.isfinite(got.sampled).all()
    for s, x in enumerate(pts):
        alone = er.modes_twin_for(name).lanes(pars, init, kappa, x, solver=solver, stop_at_end=False)
        assert np.all(alone.status == TARGET) and np.array_equal(got.sampled[s], alone.out[PLANES]), (s, x)
        assert np.all(got.sampled[s, 3] == x)
    assert np.array_equal(got.sampled[-1], got.out[PLANES])
    vac = kappa**2 / (8 * math.pi**2 * got.sampled[0, 5])
    assert np.allclose(got.sampled[0, 0], vac, rtol=1e-15, atol=0) and np.array_equal(got.sampled[0, 0], got.sampled[0, 1]) and np.all(got.sampled[0, 2] == 0.0)
    assert np.all(got.sampled[0, 4] == 0.0) and np.all(got.step_of[:, 0] == 0) and np.all(np.diff(got.step_of, axis=1) >= 0) and np.all(got.step_of[:, 1] >= 1)


@pytest.mark.parametrize("max_err", er.MAX_ERRS)
@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", er.CPU_MODELS)
def test_twin_against_truth_at_every_sample(name, solver, max_err):
    """Truth (b), ``modes_reference.truth_lane``, at each of the five samples of the same 65 lanes: no lane and no sample is left out,
    every status is TARGET, the truth is finite, and the worst relative error over the samples is within 1e-10 plus twice the value
    recorded for this model, solver and max_err."""
    init, pars, kappa, target = er.lanes_of(name)
    truth, pts = er.truth_at_samples(name), er.samples_of(name)
    assert truth.shape == (5, 5, er.LANES) and np.isfinite(truth).all()
    got = er.twin_for(name).lanes(pars, init, kappa, target, 0.0, pts, max_err=max_err, solver=solver, stop_at_end=False)
    assert np.all(got.status == TARGET) and np.isfinite(got.sampled).all()
    err, bound = er.sample_error(got.sampled, truth), er.bound(name, solver, max_err)
    each = [mo.relative_error(got.sampled[s, :3], truth[s, :3]) for s in range(5)]
    print(f"{name} {solver} max_err {max_err:g}: relative |twin - truth (b)| at the five samples {' '.join(f'{e:.3e}' for e in each)}, bound {bound:.3e}")
    assert err <= bound


def test_recorded_errors_are_anchored():
    """profiles/background_evolution.json carries the hash of the code of the three headers it was measured with, which must be the
    present code's, and every recorded value is at most 100 max_err^(4/5), the project's cap (tests/test_background_transfer.py)."""
    import background_truth as bt

    rec = er.recorded()
    assert rec["stepper_code"] == er.stepper_code_hash()
    assert sorted(rec["zoo"]) == sorted(f"{name}/{solver}/{max_err:g}" for name in ("hyperbolic", *bt.GPU_MODELS) for solver in ("rk4", "rkf") for max_err in er.MAX_ERRS)
    for key, value in rec["zoo"].items():
        max_err = float(key.rsplit("/", 1)[1])
        assert 0.0 < value <= 100.0 * max_err**0.8, (key, value)


def test_the_shift_moves_the_samples_to_each_modes_own_start(hyper):
    """``since="start"``, two wavenumbers whose modes start at N = 0 and N = 0.5: a sample before the later mode's start is NaN for it
    and finite for the earlier one, the sample exactly at a mode's start is the vacuum, and N comes back as the samples themselves.
    With neither N_eval nor stop_at_end the lanes stop with TARGET at their last sample and ``end`` is NaN."""
    p, twin, _modes = hyper
    x, v = mo.hyper_states(2)
    n_exit, samples = np.array([3.0, 3.5]), np.array([0.0, 0.25, 0.5, 1.0, 2.0])
    ev = twin.spectra_evolution(p, n_exit, samples, x, v, since="start", N_sub=mo.N_SUB, stop_at_end=False)
    assert ev.P_R.shape == ev.P_S.shape == ev.C_RS.shape == ev.N.shape == ev.eps_H.shape == (2, 2, 5) and ev.k.shape == ev.status.shape == (2, 2)
    assert np.all(ev.status == TARGET) and np.isnan(ev.end.P_R).all() and np.isnan(ev.end.N).all()
    assert np.isfinite(ev.P_R[:, 0]).all() and np.isnan(ev.P_R[:, 1, :2]).all() and np.isfinite(ev.P_R[:, 1, 2:]).all()
    for member in (ev.P_S, ev.C_RS, ev.N, ev.eps_H):
        assert np.array_equal(np.isnan(member), np.isnan(ev.P_R))
    assert np.array_equal(ev.N[:, 0], np.tile(samples, (2, 1))) and np.array_equal(ev.N[:, 1, 2:], np.tile(samples[2:], (2, 1)))
    kappa = ev.k * np.exp(-(n_exit - mo.N_SUB))[None, :]
    for j, s in ((0, 0), (1, 2)):  # (wavenumber, the sample at its start)
        vac = kappa[:, j] ** 2 / (8 * math.pi**2 * ev.eps_H[:, j, s])
        assert np.allclose(ev.P_R[:, j, s], vac, rtol=1e-14, atol=0) and np.array_equal(ev.P_R[:, j, s], ev.P_S[:, j, s]) and np.all(ev.C_RS[:, j, s] == 0.0)
    # since="exit" with the same points for the first mode: the same lane up to the rounding of the local sample
    ex = twin.spectra_evolution(p, n_exit[:1], samples - 3.0, x, v, since="exit", N_sub=mo.N_SUB, stop_at_end=False)
    assert np.array_equal(ex.P_R[:, 0], ev.P_R[:, 0]) and np.array_equal(ex.N[:, 0], 3.0 + (samples - 3.0)[None, :].repeat(2, axis=0))


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_two_samples_inside_one_step(hyper, solver):
    """Samples x and x + 1e-9 with a fixed dt: both are emitted from the same accepted step, they differ, and each equals the run
    whose target it is, bit for bit."""
    p, twin, modes = hyper
    x, v = tr.hyper_states(9)
    init = np.concatenate([x, v], axis=1)
    kappa = 20.0 * mo.friedmann_h(modes, p, init)
    pair = np.array([0.05, 0.05 + 1e-9])
    got = twin.lanes(p, init, kappa, np.nan, 0.0, pair, max_steps=2000, solver=solver, dt=2e-3, stop_at_end=False)
    assert np.all(got.status == TARGET) and np.all(got.cursor == 2) and np.isnan(got.out).all()
    assert np.array_equal(got.step_of[:, 0], got.step_of[:, 1]) and np.all(got.step_of[:, 0] >= 1) and np.array_equal(got.step_of[:, 1], got.accepted)
    assert not np.array_equal(got.sampled[0, :3], got.sampled[1, :3])
    for s in range(2):
        alone = modes.lanes(p, init, kappa, pair[s], max_steps=2000, solver=solver, dt=2e-3, stop_at_end=False)
        assert np.all(alone.status == TARGET) and np.array_equal(got.sampled[s], alone.out[PLANES]) and np.array_equal(alone.accepted, got.accepted)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_what_every_stop_keeps(hyper, solver):
    """The four kinds of tests/test_background_modes_gpu.py::test_every_status_side_by_side -- five steps of dt = 0.05, kappa = 2 H0,
    the target N = 0.2 -- with samples at 0.1, 0.2 and 0.3.  TARGET: the samples up to its target, the one at the target equal to the
    final values.  COMPLETE: the samples its five steps passed, NaN after.  ENDED: only the samples <= N_end.  NONFINITE: all NaN.
    Statuses, N_end and final values are those of the lanes without samples.  A lane with neither a target nor stop_at_end stops
    with TARGET at its last sample and its final planes stay NaN."""
    p, twin, modes = hyper
    kinds = np.array([[4.7, 0.3, 2e-3], [2.5, -0.2, 2e-2], [2.2, 0.1, 1e-2], [3.0, 0.5, 0.0]])
    x = np.tile(kinds[:, :2], (2, 1))
    H = np.sqrt((x[:, 0] - 1) ** 2 / 6)
    v = np.stack([-(x[:, 0] - 1) / (3 * H), np.tile(kinds[:, 2], 2)], axis=1)
    kind = np.arange(8) % 4
    v[kind == 3] = 0.0
    x[4:, 1] += 0.1
    init = np.concatenate([x, v], axis=1)
    kappa = 2.0 * mo.friedmann_h(modes, p, init)
    pts = np.array([0.1, 0.2, 0.3])
    got = twin.lanes(p, init, kappa, 0.2, 0.0, pts, max_steps=5, solver=solver, dt=0.05)
    plain = modes.lanes(p, init, kappa, 0.2, max_steps=5, solver=solver, dt=0.05)
    assert np.array_equal(got.status, np.array([TARGET, COMPLETE, ENDED, NONFINITE], dtype=np.int8)[kind]) and np.array_equal(got.status, plain.status)
    assert np.array_equal(got.out, plain.out, equal_nan=True) and np.array_equal(got.N_end, plain.N_end, equal_nan=True)
    emitted = np.isfinite(got.sampled[:, 0, :]).T  # (lane, sample)
    assert np.array_equal(np.isfinite(got.sampled).all(axis=1).T, emitted) and np.array_equal(np.isnan(got.sampled).all(axis=1).T, ~emitted)
    assert np.array_equal(emitted[kind == 0], np.tile([True, True, False], (2, 1))) and np.array_equal(got.sampled[1][:, kind == 0], got.out[PLANES][:, kind == 0])
    complete = kind == 1
    assert np.all(plain.final[complete, 5] < 0.2) and np.array_equal(emitted[complete], pts[None, :] <= plain.final[complete, 5][:, None])
    assert emitted[complete].any() and np.array_equal(emitted.sum(axis=1), got.cursor * (kind != 3))
    ended = kind == 2
    assert np.all(got.N_end[ended] > 0.0) and np.array_equal(emitted[ended], pts[None, :] <= got.N_end[ended][:, None])
    assert not emitted[kind == 3].any()
    for s, n in enumerate(pts):
        alone = modes.lanes(p, init, kappa, n, max_steps=5, solver=solver, dt=0.05)
        e = emitted[:, s]
        assert np.all(alone.status[e] == TARGET) and np.array_equal(got.sampled[s][:, e], alone.out[PLANES][:, e])
    free = twin.lanes(p, init[:1], kappa[:1], np.nan, 0.0, pts, max_steps=100, solver=solver, dt=0.05, stop_at_end=False)
    assert free.status[0] == TARGET and free.cursor[0] == 3 and np.isnan(free.out).all() and np.isfinite(free.sampled).all()
    assert np.array_equal(free.sampled[:2, :, 0], got.sampled[:2, :, 0]) and free.accepted[0] == free.step_of[0, 2] < 100


def test_an_ended_lane_keeps_the_samples_up_to_its_end(hyper):
    """The ENDED kind further from the end, adaptive: the samples up to N_end are emitted, those after it are NaN, and the final values
    are the run's without samples."""
    p, twin, modes = hyper
    x, v = tr.hyper_states(5)
    init = np.concatenate([x, v], axis=1)
    kappa = 20.0 * mo.friedmann_h(modes, p, init)
    pts = np.linspace(0.25, 3.0, 12)
    got = twin.lanes(p, init, kappa, np.nan, 0.0, pts)
    plain = modes.lanes(p, init, kappa, np.nan)
    assert np.all(got.status == ENDED) and np.array_equal(got.out, plain.out) and np.array_equal(got.N_end, plain.N_end)
    emitted = np.isfinite(got.sampled[:, 0, :]).T
    assert np.array_equal(emitted, pts[None, :] <= got.N_end[:, None]) and emitted.any() and not emitted.all()


def test_transfer_from_spectra_inverts_the_transfer():
    """Spectra constructed from chosen T_RS and T_SS with R = R* + T_RS S*, S = T_SS S*: both are recovered to rounding and the
    residual of the third relation is rounding; at ``ref`` itself T_SS = 1, T_RS = 0 and the residual 0 exactly."""
    from inflatox_amd import _native, background

    rng = np.random.default_rng(4)
    r0, s0 = rng.uniform(1.0, 2.0, (3, 2, 1)), rng.uniform(0.5, 1.5, (3, 2, 1))
    c0 = rng.uniform(-0.5, 0.5, (3, 2, 1)) * np.sqrt(r0 * s0)
    t_rs = np.concatenate([np.zeros((3, 2, 1)), rng.uniform(-3.0, 3.0, (3, 2, 6))], axis=2)
    t_ss = np.concatenate([np.ones((3, 2, 1)), rng.uniform(0.01, 2.0, (3, 2, 6))], axis=2)
    ev = types.SimpleNamespace(P_R=r0 + 2 * t_rs * c0 + t_rs**2 * s0, P_S=t_ss**2 * s0, C_RS=t_ss * (c0 + t_rs * s0))
    got_rs, got_ss, residual = background.transfer_from_spectra(ev, 0)
    assert got_rs.shape == got_ss.shape == residual.shape == (3, 2, 7)
    assert np.allclose(got_ss, t_ss, rtol=1e-14, atol=0) and np.allclose(got_rs, t_rs, rtol=0, atol=1e-13) and np.abs(residual).max() <= 1e-13 * ev.P_R.max()
    assert np.all(got_ss[..., 0] == 1.0) and np.all(got_rs[..., 0] == 0.0) and np.all(residual[..., 0] == 0.0)
    # another reference sample: the transfer between two later samples composes
    rs3, ss3, _ = background.transfer_from_spectra(ev, 3)
    assert np.allclose(ss3, t_ss / t_ss[..., 3:4], rtol=1e-13) and np.allclose(rs3, (t_rs - t_rs[..., 3:4]) / t_ss[..., 3:4], rtol=0, atol=1e-12)
    for bad in (7, -8):
        with pytest.raises(ValueError):
            background.transfer_from_spectra(ev, bad)
    with pytest.raises(_native.InflatoxShapeError):
        background.transfer_from_spectra(types.SimpleNamespace(P_R=ev.P_R, P_S=ev.P_S[:2], C_RS=ev.C_RS), 0)
    with pytest.raises(TypeError):
        background.transfer_from_spectra(ev, 0.5)


@pytest.fixture(scope="module")
def cross_truth():
    return er.cross_truths()


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_transfer_from_spectra_against_transfer_functions(cross_truth, solver):
    """One turning trajectory of ``modes_reference.hyper_states``, N_sub = 3, the mode that leaves the horizon at N = 3, the reference
    sample 4 e-folds after the exit: T_RS and T_SS measured from the sampled spectra of the mode functions against the super-horizon
    ``transfer_functions`` started at the reference state.  The trajectory ends inflation at N = 8.16, so the samples go to 5 e-folds
    after the exit, not to 8.  The two independent truths differ by what the super-horizon form and the default dq/dN leave
    (recorded: 0.079 in T_SS, 1.3e-6 in T_RS); the two host twins differ by at most twice that plus their own recorded errors -- a
    difference of signed values, no absolute value of either side is taken.  The lane takes >= 257 accepted steps, and at the
    reference sample itself T_SS = 1 and T_RS = 0.

    FINDING: the SIGN of T_RS does not agree between the two truths on this trajectory -- -1.3e-6 from the
    spectra against +9.8e-10 from ``transfer_functions`` at the last sample -- and it says nothing about either convention.  The
    trajectory turns at its start (omega = 2.8 per e-fold at N = 0, 3e-5 at the exit, 2e-9 at the reference sample), so the sourced
    T_RS is 1e-9, while the inversion R = R* + T_RS S*, S = T_SS S* is exact only when S is one decaying solution: the
    isocurvature mass here (mu = 1.8 H^2) gives S two decay rates, and the part of S correlated with R at the reference sample
    (C_RS* / P_S* = 4e-4) has a share of 3e-3 still on the fast one.  That floor is a thousand times the sourced T_RS.  Each twin
    has the sign of its own truth, which is what is asserted; a trajectory that still turns after horizon exit is needed to compare
    the two orientations of e_s, and none of the test fixtures does."""
    from inflatox_amd import background

    rec = er.recorded()["cross"]
    (m_rs, m_ss), (t_rs, t_ss), _spectra = cross_truth
    d_rs, d_ss = np.abs(m_rs - t_rs).max(), np.abs(m_ss - t_ss).max()
    assert d_rs <= 1.01 * rec["truth_T_RS"] + 1e-12 and d_ss <= 1.01 * rec["truth_T_SS"] + 1e-12  # (the record is this measurement)
    (a_rs, a_ss), (b_rs, b_ss), spectra = er.cross_twins(solver)
    ev = types.SimpleNamespace(P_R=spectra[0], P_S=spectra[1], C_RS=spectra[2])
    f_rs, f_ss, residual = background.transfer_from_spectra(ev, 0)
    assert np.array_equal(f_rs, a_rs) and np.array_equal(f_ss, a_ss) and f_ss[0] == 1.0 and f_rs[0] == 0.0 and residual[0] == 0.0
    e_rs, e_ss = np.abs(a_rs - b_rs).max(), np.abs(a_ss - b_ss).max()
    print(f"{solver}: T_RS from the modes {a_rs[1:]}, from transfer_functions {b_rs[1:]}; T_SS {a_ss[1:]} and {b_ss[1:]}; |difference| {e_rs:.3e}, {e_ss:.3e} "
          f"(truths: {d_rs:.3e}, {d_ss:.3e}); residual of the third relation / P_R {np.abs(residual / spectra[0]).max():.3e}")  # fmt: skip
    assert e_rs <= 2.0 * rec["truth_T_RS"] + rec[f"twin_T_RS/{solver}"] + 1e-12 and e_ss <= 2.0 * rec["truth_T_SS"] + rec[f"twin_T_SS/{solver}"] + 1e-12
    assert np.array_equal(np.sign(a_rs), np.sign(m_rs)) and np.array_equal(np.sign(b_rs), np.sign(t_rs))
    assert np.all(np.diff(a_ss) < 0) and np.all(np.diff(b_ss) < 0)  # (the isocurvature power decays on both sides)


def test_surface(monkeypatch):
    """Public names, the signature tables, the header's declared function set, the sources of the object and the layout constants."""
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import _EVOLUTION_SOURCES, _MODES_SOURCES, KERNEL_GROUPS, CompilationArtifact

    assert {"spectra_evolution", "SpectraEvolution", "evolution_map", "transfer_from_spectra"} <= set(background.__all__)
    assert all(name in background.__doc__ for name in ("spectra_evolution", "evolution_map", "transfer_from_spectra"))
    assert background.SpectraEvolution._fields == ("P_R", "P_S", "C_RS", "N", "eps_H", "k", "end", "status") == er.TwinEvolution._fields[:8]
    assert len(_native.SIGNATURES) == 57 and list(_native.EVOLUTION_SIGNATURES) == ["inflx_mode_evolution"]
    assert not set(_native.EVOLUTION_SIGNATURES) & (set(_native.SIGNATURES) | set(_native.DELTAN_SIGNATURES))
    assert len(_native.EVOLUTION_SIGNATURES["inflx_mode_evolution"][1]) == len(_native.SIGNATURES["inflx_mode_spectra"][1]) + 4 == 20
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inflx_hip_evolution.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(inflx_[a-z_0-9]+)\s*\(", text))) == ["inflx_mode_evolution"]
    assert '#include "inflx_hip_evolution.h"' in open(os.path.join(ROOT, "include", "inflx_hip.h")).read()
    _native.build_library()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "inflx_mode_evolution") and callable(_native.InflatoxDevLib.mode_evolution)
    assert _EVOLUTION_SOURCES == ("inflx_evolution_kernels.hip", "inflx_evolution.h", "inflx_evolution_abi.h", "inflx_modes.h", "inflx_modes_abi.h", "inflx_background.h",
                                  "inflx_background_abi.h")  # fmt: skip
    assert _EVOLUTION_SOURCES[3:] == _MODES_SOURCES[1:] and "evolution" not in KERNEL_GROUPS and callable(CompilationArtifact.ensure_evolution)
    abi = open(os.path.join(er.CSRC, "inflx_evolution_abi.h")).read()
    for pattern in (r"#define INFLX_EV_ABI_VERSION 1\b", r"INFLX_EV_CARRY_CURSOR = 26,", r"INFLX_EV_CARRY_PLANES = 27,", r"#define INFLX_EV_SAMPLE_PLANES 6\b",
                    r"#define INFLX_EV_OUT_PLANES 22\b", r"#define INFLX_EV_THREADS 256\b", r"sizeof\(InflxEvArgs\) == 128"):  # fmt: skip
        assert re.search(pattern, abi), pattern
    assert _native.EV_SAMPLE_PLANES == 6 and re.search(r"#define INFLX_EV_NSAMPLE 6\b", open(os.path.join(er.CSRC, "inflx_evolution.h")).read())
    kernels = open(os.path.join(er.CSRC, "inflx_evolution_kernels.hip")).read()
    assert sorted(re.findall(r"__global__ __launch_bounds__\(INFLX_EV_THREADS\) void (\w+)", kernels)) == ["inflx_ev_advance_rk4", "inflx_ev_advance_rkf", "inflx_ev_init"]
    assert "inflx_md_resume(s, p)" in kernels and kernels.count("atomicAdd") == 1 and kernels.count("__ballot") == 1 and "asm" not in kernels


def test_bad_arguments_raise_before_the_device(monkeypatch):
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    for ensure in ("ensure_evolution", "ensure_modes", "ensure_background"):
        monkeypatch.setattr(CompilationArtifact, ensure, no_device)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = np.zeros((3, 2)) + 2.0, np.zeros((3, 2)) + 0.1
    good, pts = [5.0, 6.0], [0.0, 1.0]
    shape, value = _native.InflatoxShapeError, ValueError
    se = background.spectra_evolution
    for bad in ([], [0.0, float("nan")], [1.0, 1.0], [1.0, 0.5], [float("inf")], "abc", [-5.1, 0.0]):
        with pytest.raises(value):
            se(art, p, good, bad, x, v)
    with pytest.raises(shape):
        se(art, p, good, [[0.0, 1.0]], x, v)
    with pytest.raises(value):
        se(art, p, good, pts, x, v, since="end")
    for bad in ([4.9, 6.0], [5.0, float("nan")], []):
        with pytest.raises(value):
            se(art, p, bad, pts, x, v)
    for args in ((p[:2], good, pts, x, v), (p, good, pts, x, v[:2]), (p, good, pts, np.zeros((3, 3)), np.zeros((3, 3))), (p, [[5.0]], pts, x, v)):
        with pytest.raises(shape):
            se(art, *args)
    for kw in (dict(N_sub=0.0), dict(N_eval=6.0), dict(N_eval=6.5, since="exit"), dict(N_eval=0.9, since="start"), dict(max_err=0.0), dict(solver="euler"), dict(dt=-1.0),
               dict(max_steps=0), dict(N_eval="x")):  # fmt: skip
        with pytest.raises(value):
            se(art, p, good, pts, x, v, **kw)
    # (N_eval=6.5 with since="exit": the sample 1 e-fold after the exit at N = 6 lies beyond it)
    em = background.evolution_map
    ss = [[2.0, 4.0], [-1.0, 1.0]]
    for kw in (dict(samples=[]), dict(samples=[1.0, 1.0]), dict(samples=[-0.4, 0.0], N_sub=0.3), dict(samples=pts, N_sub=-1.0), dict(samples=pts, N_star=-1.0),
               dict(samples=pts, N_star="x")):  # fmt: skip
        with pytest.raises(value):
            em(art, p, ss, 3, 3, **kw)
    # good arguments get as far as the device
    with pytest.raises(AssertionError, match="a device call"):
        se(art, p, good, pts, x, v, stop_at_end=False)
    with pytest.raises(AssertionError, match="a device call"):
        em(art, p, ss, 3, 3, pts)


def test_standalone_twin_program_is_clean_under_the_sanitizers(hyper):
    """tests/evolution_twin.cpp with -DEVOLUTION_TWIN_MAIN as a program of its own, built with -fsanitize=address,undefined and run on
    lanes of every kind -- samples before the start, at it, two inside one step, beyond the end, a lane at rest: no report, exit
    status 0, and the numbers are the shared-library twin's, bit for bit."""
    p, twin, _modes = hyper
    _spec, art = workloads.artifact_for("hyperbolic")
    x, v = tr.hyper_states(6)
    init = np.concatenate([x, v], axis=1)
    init[5, 2:] = 0.0
    kappa = 20.0 * mo.friedmann_h(er.modes_twin_for("hyperbolic"), p, init)
    shift = np.array([0.0, 0.1, -0.2, 0.3, 0.0, 0.0])
    target = np.array([np.nan, 0.5, np.nan, 0.4, 50.0, 0.5])
    pts = np.array([-0.5, 0.1, 0.3, 0.3 + 1e-9, 0.6, 40.0])
    kw = dict(max_steps=400, max_err=1e-8, solver="rkf", stop_at_end=True)
    exe = er.program(art)
    status, cursor, sampled = er.run_program(exe, p, init, kappa, target, shift, pts, **kw)
    want = twin.lanes(p, init, kappa, target, shift, pts, **kw)
    assert np.array_equal(status, want.status) and np.array_equal(cursor, want.cursor) and np.array_equal(sampled, want.sampled, equal_nan=True)
    assert set(status.tolist()) >= {TARGET, NONFINITE} and np.isfinite(sampled).any() and np.isnan(sampled).any()
