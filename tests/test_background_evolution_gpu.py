"""Spectra sampled along a mode's evolution on the GPU (inflatox_amd.background.spectra_evolution, evolution_map,
InflatoxDevLib.mode_evolution): the kernels against the host twin and truth (b) at every sample on the curved zoo; every sample and the
final values against the modes kernels' runs that stop there, bit for bit, over several launches; every stop status side by side; a
call of more than one pass, bounded by the samples; the two heaviest example models; ``evolution_map`` against its two halves; the
refusals of the evolution object; and ``inflx_mode_spectra`` untouched by an evolution call on the same handle.  Twin, truth and bounds
are those tests/test_background_evolution.py establishes on the host build (tests/evolution_reference.py,
profiles/background_evolution.json); every difference is printed."""

import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import background_truth as bt
import evolution_reference as er
import modes_reference as mo
import workloads
from modes_reference import COMPLETE, ENDED, NONFINITE, TARGET

pytestmark = pytest.mark.gpu

PLANES = [0, 1, 2, 19, 20, 21]
MEMBERS = ("P_R", "P_S", "C_RS", "k", "N", "eps_H", "modes", "N_end", "status")
SAMPLED = ("P_R", "P_S", "C_RS", "N", "eps_H")


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return np.asarray(spec.args, dtype=np.float64), art, er.twin_for("hyperbolic")


def _lib(bg, art):
    art.ensure_evolution()
    return bg._dylib(art, background=False)


def _ev(bg, art, pars, init, kappa, target, shift, samples, max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None, stop_at_end=True):
    """``InflatoxDevLib.mode_evolution`` on the artefact's handle: (out (22, n), sampled (S, 6, n), N_end, status)"""
    from inflatox_amd import _native

    n = len(init)
    b = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))  # noqa: E731
    return _lib(bg, art).mode_evolution(pars, init, b(kappa), b(target), b(shift), samples, max_steps, bg._METHODS[solver], max_err, dt or 0.0,
                                        _native.EOM_STOP_AT_END if stop_at_end else 0)  # fmt: skip


def _md(bg, art, pars, init, kappa, target, max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None, stop_at_end=True):
    """``InflatoxDevLib.mode_spectra`` likewise: (out (22, n), N_end, status)"""
    from inflatox_amd import _native

    art.ensure_modes()
    n = len(init)
    b = lambda a: np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))  # noqa: E731
    return bg._dylib(art, background=False).mode_spectra(pars, init, b(kappa), b(target), max_steps, bg._METHODS[solver], max_err, dt or 0.0,
                                                         _native.EOM_STOP_AT_END if stop_at_end else 0)  # fmt: skip


def _same_end(a, b, rows=slice(None), cols=slice(None)):
    return all(np.array_equal(getattr(a, m)[rows][:, cols], getattr(b, m), equal_nan=True) for m in MEMBERS)


def _same_samples(a, b, rows=slice(None), cols=slice(None)):
    return all(np.array_equal(getattr(a, m)[rows][:, cols], getattr(b, m), equal_nan=True) for m in SAMPLED)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_kernel_against_twin_and_truth(bg, name, solver):
    """All 257 lanes of ``background_truth.batch`` (four wavefronts and one lane), a parameter row per lane, kappa = H0 e^3, the five
    samples at 0, 1/4, 1/2, 3/4 and 1 x the target, the default max_err, at most 20 000 steps.  ``status`` is the host twin's on every
    lane; on the lanes the twin reports TARGET -- all of the first 65 and at least 250 in all -- the samples and the final values are
    within ``modes_reference.bound`` of the twin; the first 65 lanes are within the bound of truth (b) at every sample."""
    art = bt.device_artifact(name)
    init, pars, kappa, target = mo.zoo_lanes(name, 257)
    pts = er.samples_of(name)
    truth = er.truth_at_samples(name)
    out, sampled, n_end, status = _ev(bg, art, pars, init, kappa, target, 0.0, pts, max_steps=20_000, solver=solver, stop_at_end=False)
    twin = er.twin_for(name).lanes(pars, init, kappa, target, 0.0, pts, max_steps=20_000, solver=solver, stop_at_end=False)
    ok = twin.status == TARGET
    assert out.shape == (22, 257) and sampled.shape == (5, 6, 257) and np.array_equal(status, twin.status)
    assert ok[: mo.LANES].all() and ok.sum() >= 250
    bound, truth_bound = mo.bound(name, solver, 1e-8), er.bound(name, solver, 1e-8)
    diff = max(mo.relative_error(sampled[s, :3][:, ok], twin.sampled[s, :3][:, ok]) for s in range(5))
    diff_end = mo.relative_error(out[:3][:, ok], twin.out[:3][:, ok])
    err = er.sample_error(sampled[:, :, : mo.LANES], truth)
    print(f"{name} {solver}: worst relative |GPU - host twin| on {ok.sum()} TARGET lanes {diff:.3e} at the samples, {diff_end:.3e} at the target (bound {bound:.3e}); "
          f"worst relative |GPU - truth (b)| over the samples {err:.3e} (bound {truth_bound:.3e})")  # fmt: skip
    assert np.isfinite(sampled[:, :, ok]).all() and np.isfinite(out[:, ok]).all() and np.isnan(out[:, ~ok]).all()
    assert diff <= bound and diff_end <= bound and err <= truth_bound
    assert np.array_equal(np.isnan(sampled), np.isnan(twin.sampled)) and np.all(sampled[:, 3][:, ok] == pts[:, None]) and np.isnan(n_end).all()
    assert np.array_equal(sampled[-1][:, ok], out[PLANES][:, ok]) and np.all(sampled[0, 2, ok] == 0.0) and np.array_equal(sampled[0, 0, ok], sampled[0, 1, ok])


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_samples_and_end_are_the_modes_kernels_bit_for_bit(bg, hyper, solver):
    """The fixtures of tests/test_background_modes_gpu.py::test_several_launches_lane_numbering_and_lane_independence: B = 5
    trajectories, K = 52 wavenumbers, N_sub = 3, max_err = 1e-10, every lane of more than 256 accepted steps, so the cursor is carried
    across a launch boundary.  ``since="start"``: samples inside the first launch of the lanes that start late and in later launches of all (by the host twin's count
    of the step that emits each, fed the device's own first stage), a pair 1e-9 apart, and one at N_eval itself.  Every sample equals,
    bit for bit, the modes kernels' run whose target it is -- ``mode_spectra`` with the very lanes of the front end, and
    ``power_spectra(N_eval=sample)`` for the samples beyond the last exit; ``ev.end`` is ``power_spectra``'s result bit for bit, with
    N_eval and to the end of inflation, ``k`` included; a permuted batch and the sub-batches (1, 1) and (5, 13) give the same lanes."""
    p, art, twin = hyper
    x, v = mo.hyper_states()
    B, K = mo.HYPER_B, mo.HYPER_K
    kw = dict(N_sub=mo.N_SUB, max_err=mo.HYPER_MAX_ERR, solver=solver)
    samples = np.array([0.52, 0.6, 2.0, 4.0, 4.0 + 1e-9, 5.5, mo.HYPER_N_EVAL])
    ev = bg.spectra_evolution(art, p, mo.HYPER_N_EXIT, samples, x, v, since="start", N_eval=mo.HYPER_N_EVAL, **kw)
    at = bg.power_spectra(art, p, mo.HYPER_N_EXIT, x, v, N_eval=mo.HYPER_N_EVAL, **kw)
    assert isinstance(ev, bg.SpectraEvolution) and isinstance(ev.end, bg.PowerSpectra) and ev.P_R.shape == ev.N.shape == (B, K, 7)
    assert np.all(ev.status == TARGET) and _same_end(ev.end, at) and np.array_equal(ev.k, at.k) and np.array_equal(ev.status, at.status)
    for m in SAMPLED:
        assert np.isfinite(getattr(ev, m)).all(), m
    assert np.array_equal(ev.N, np.broadcast_to(samples, (B, K, 7)))
    for m in ("P_R", "P_S", "C_RS", "eps_H"):  # the sample at N_eval is the end
        assert np.array_equal(getattr(ev, m)[:, :, 6], getattr(at, m)), m
    assert not np.array_equal(ev.P_S[:, :, 3], ev.P_S[:, :, 4])
    # the lanes of the front end, and each sample as the modes kernels' own target
    args = bg._check_spectra(art, p, mo.HYPER_N_EXIT, x, v, mo.HYPER_N_EVAL, mo.N_SUB, 1_000_000, mo.HYPER_MAX_ERR, solver, None, True)
    _h, _st, run, lane_start, lane_p, init, kappa, target = bg._mode_stage1(art, *args[:4], *args[4:])
    assert run.size == B * K and np.array_equal(target, mo.HYPER_N_EVAL - lane_start)
    host = twin.lanes(lane_p, init, kappa, target, lane_start, samples, max_err=mo.HYPER_MAX_ERR, solver=solver)
    assert np.all(host.status == TARGET) and host.accepted.min() > 256
    print(f"{solver}: {host.accepted.min()} .. {host.accepted.max()} accepted steps; the samples are emitted in steps "
          + ", ".join(f"{host.step_of[:, s].min()}..{host.step_of[:, s].max()}" for s in range(7)))  # fmt: skip
    # (the later a lane starts, the sooner it meets the first samples: some lanes emit them in their first launch, others in their second)
    assert host.step_of[:, 0].min() <= 256 and (host.step_of[:, 1] <= 256).any() and host.step_of[:, 3].min() > 256
    assert np.array_equal(host.step_of[:, 3], host.step_of[:, 4])
    planes = {"P_R": 0, "P_S": 1, "C_RS": 2, "eps_H": 21}
    for s, n in enumerate(samples):
        out, _ends, st = _md(bg, art, lane_p, init, kappa, n - lane_start, max_err=mo.HYPER_MAX_ERR, solver=solver)
        assert np.all(st == TARGET)
        for m, plane in planes.items():
            assert np.array_equal(getattr(ev, m)[:, :, s].reshape(-1), out[plane]), (s, m)
        if n > mo.HYPER_N_EXIT.max() and n < mo.HYPER_N_EVAL:
            ps = bg.power_spectra(art, p, mo.HYPER_N_EXIT, x, v, N_eval=float(n), **kw)
            assert all(np.array_equal(getattr(ev, m)[:, :, s], getattr(ps, m)) for m in SAMPLED), s
    # to the end of inflation
    tail = np.array([4.0, 7.0, 7.9, 30.0])
    to_end = bg.spectra_evolution(art, p, mo.HYPER_N_EXIT, tail, x, v, since="start", **kw)
    got = bg.power_spectra(art, p, mo.HYPER_N_EXIT, x, v, **kw)
    assert np.all(to_end.status == ENDED) and _same_end(to_end.end, got) and np.array_equal(to_end.P_R[:, :, 0], ev.P_R[:, :, 3])
    assert np.isfinite(to_end.P_R[:, :, :3]).all() and np.isnan(to_end.P_R[:, :, 3]).all() and np.isnan(to_end.N[:, :, 3]).all()
    perm = np.random.default_rng(9).permutation(B)
    for rows, cols, sub in ((perm, slice(None), (mo.HYPER_N_EXIT, x[perm], v[perm])), (slice(3, 4), slice(17, 18), (mo.HYPER_N_EXIT[17:18], x[3:4], v[3:4])),
                            (slice(None), slice(39, 52), (mo.HYPER_N_EXIT[39:], x, v))):  # fmt: skip
        other = bg.spectra_evolution(art, p, sub[0], tail, sub[1], sub[2], since="start", **kw)
        assert _same_samples(to_end, other, rows, cols) and _same_end(to_end.end, other.end, rows, cols), (rows, cols)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_every_status_side_by_side(bg, hyper, solver):
    """The 257 lanes of four kinds of tests/test_background_modes_gpu.py -- five steps of dt = 0.05, kappa = 2 H0, the target N = 0.2 --
    with samples at 0.1, 0.2 and 0.3: statuses, N_end and the pattern of what is emitted are the host twin's (TARGET: the samples up
    to the target; COMPLETE: those its five steps passed; ENDED: those <= N_end; NONFINITE: none), the values within 1e-11 of each
    spectrum's scale."""
    p, art, twin = hyper
    kinds = np.array([[4.7, 0.3, 2e-3], [2.5, -0.2, 2e-2], [2.2, 0.1, 1e-2], [3.0, 0.5, 0.0]])
    x = np.tile(kinds[:, :2], (65, 1))[:257]
    H = np.sqrt((x[:, 0] - 1) ** 2 / 6)
    v = np.stack([-(x[:, 0] - 1) / (3 * H), np.tile(kinds[:, 2], 65)[:257]], axis=1)
    kind = np.arange(257) % 4
    v[kind == 3] = 0.0
    x[:, 1] += np.linspace(0.0, 0.3, 257)
    init = np.concatenate([x, v], axis=1)
    kappa = 2.0 * mo.friedmann_h(er.modes_twin_for("hyperbolic"), p, init)
    pts = np.array([0.1, 0.2, 0.3])
    out, sampled, n_end, status = _ev(bg, art, p, init, kappa, 0.2, 0.0, pts, max_steps=5, solver=solver, dt=0.05)
    want = twin.lanes(p, init, kappa, 0.2, 0.0, pts, max_steps=5, solver=solver, dt=0.05)
    assert np.array_equal(status, np.array([TARGET, COMPLETE, ENDED, NONFINITE], dtype=np.int8)[kind]) and np.array_equal(status, want.status)
    assert np.array_equal(np.isnan(sampled), np.isnan(want.sampled)) and np.array_equal(np.isnan(out), np.isnan(want.out))
    emitted = np.isfinite(sampled[:, 0, :])
    assert np.array_equal(emitted[:, kind == 0], np.tile([[True], [True], [False]], (1, (kind == 0).sum()))) and not emitted[:, kind == 3].any()
    assert emitted[:, kind == 1].any() and np.array_equal(emitted[:, kind == 2], pts[:, None] <= n_end[None, kind == 2])
    diff = max(mo.relative_error(sampled[s, :3][:, emitted[s]], want.sampled[s, :3][:, emitted[s]]) for s in range(3) if emitted[s].any())
    ends = (kind == 0) | (kind == 2)
    diff_end = mo.relative_error(out[:3][:, ends], want.out[:3][:, ends])
    print(f"{solver}: worst relative |GPU - host twin| {diff:.3e} at the samples, {diff_end:.3e} at the end")
    assert diff <= 1e-11 and diff_end <= 1e-11 and np.allclose(sampled[:, 3:][np.isfinite(sampled[:, 3:])], want.sampled[:, 3:][np.isfinite(sampled[:, 3:])], rtol=0, atol=1e-11)
    assert np.array_equal(sampled[1][:, kind == 0], out[PLANES][:, kind == 0])
    free = _ev(bg, art, p, init[:5], kappa[:5], np.nan, 0.0, pts, max_steps=100, solver=solver, dt=0.05, stop_at_end=False)
    assert free[3][0] == free[3][4] == TARGET and np.isnan(free[0]).all() and np.isfinite(free[1][:, :, [0, 4]]).all()


def test_more_than_one_pass_bounded_by_the_samples(bg, hyper):
    """S = 8192 samples over 3 e-folds and 27 x 19 = 513 lanes: a pass holds the lanes whose results -- (22 + 6 S) doubles each -- fit
    the 256 MiB result buffer, 682, rounded down to whole workgroups: 512.  The second pass holds one lane.  The result equals two
    separate calls of 512 lanes and of 1 lane, bit for bit and NaN where NaN."""
    p, art, _twin = hyper
    rows = open(os.path.join(er.CSRC, "inflx_background_rows.h")).read()
    row_bytes = int(re.search(r"kBgRowBytes = size_t\((\d+)\) << (\d+);", rows).group(1)) << int(re.search(r"kBgRowBytes = size_t\((\d+)\) << (\d+);", rows).group(2))
    S, n, threads = 8192, 27 * 19, 256
    fit = row_bytes // ((22 + 6 * S) * 8)
    per_pass = fit - fit % threads
    assert row_bytes == 268_435_456 and fit == 682 and per_pass == 512 and n - per_pass == 1
    rng = np.random.default_rng(6)
    x = np.stack([rng.uniform(4.5, 5.0, n), rng.uniform(-1.0, 1.0, n)], axis=1)
    init = np.concatenate([x, np.stack([np.full(n, -0.8), rng.uniform(-1e-3, 1e-3, n)], axis=1)], axis=1)
    kappa = rng.uniform(2.0, 6.0, n)
    shift = rng.uniform(-0.2, 0.2, n)
    pts = np.linspace(0.0, 3.0, S)
    kw = dict(max_steps=400, dt=0.01, stop_at_end=False)
    whole = _ev(bg, art, p, init, kappa, np.nan, shift, pts, **kw)
    assert whole[1].shape == (S, 6, n) and np.all(whole[3] == TARGET) and np.isnan(whole[0]).all()
    finite = np.isfinite(whole[1][:, 0, :])
    assert np.array_equal(finite, pts[:, None] - shift[None, :] >= 0.0) and finite[:, per_pass].any() and finite[:, per_pass - 1].any()
    for sl in (slice(0, per_pass), slice(per_pass, n)):
        alone = _ev(bg, art, p, init[sl], kappa[sl], np.nan, shift[sl], pts, **kw)
        for a, b in zip(whole, alone):
            assert np.array_equal(a[..., sl], b, equal_nan=True), sl


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", ["egno", "d5"])
def test_heavy_example_models_against_twin(bg, name, solver):
    """The evolution objects of the two example models with the highest register demand, the lanes and spans of
    tests/test_background_modes_gpu.py, three samples: ``status`` is the host twin's and samples and final values agree with it to
    the project's parity bar, 1e-10 of each spectrum's scale."""
    from background_sampled_reference import EGNO_SEEDS
    from test_background import VELOCITY, _points, initial_state

    spec, art = workloads.artifact_for(name)
    if name == "egno":
        init, target = np.array([initial_state("egno", seed) for seed in EGNO_SEEDS]), 0.02
    else:
        init, target = _points(name, 257) * np.array([1, 1, VELOCITY[name], VELOCITY[name]]), 2e-4
    pts = target * np.array([0.0, 0.5, 1.0])
    kappa = mo.friedmann_h(mo.ModesTwin(art), spec.args, init) * math.exp(mo.N_SUB)
    out, sampled, _n_end, status = _ev(bg, art, spec.args, init, kappa, target, 0.0, pts, solver=solver, stop_at_end=False)
    want = er.EvolutionTwin(art).lanes(spec.args, init, kappa, target, 0.0, pts, solver=solver, stop_at_end=False)
    assert np.array_equal(status, want.status) and np.all(status == TARGET) and np.isfinite(sampled).all()
    rel = max(mo.relative_error(sampled[s, :3], want.sampled[s, :3]) for s in (1, 2))  # (C_RS = 0 at the vacuum: compared below)
    rel_end = mo.relative_error(out[:3], want.out[:3])
    print(f"{name} {solver}: worst relative |GPU - host twin| {rel:.3e} at the samples, {rel_end:.3e} at the target; {want.accepted.min()} .. {want.accepted.max()} steps")
    assert rel <= 1e-10 and rel_end <= 1e-10 and np.allclose(sampled[0, :2], want.sampled[0, :2], rtol=1e-12, atol=0) and np.all(sampled[0, 2] == 0.0)
    assert np.array_equal(sampled[2], out[PLANES])


def test_evolution_map_is_its_two_halves(bg, hyper):
    """A 6 x 5 grid with N_star = 50 over a range of which only a part inflates for N_star + N_sub e-folds: ``evolution_map`` equals
    ``horizon_exit_map`` at N_star + N_sub followed by ``spectra_evolution(N_exit=[N_sub], since="exit")`` from the states found, bit for
    bit, and is NaN exactly where no exit state was found."""
    p, art, _twin = hyper
    ss, d = [[12.0, 17.5], [-1.0, 1.0]], (0.0, 0.0)
    pts = np.array([-1.0, 0.0, 2.0, 10.0])
    kw = dict(N_star=50.0, N_sub=3.0, derivatives_init=d)
    (p_r, p_s, c_rs), state, n_end, status = bg.evolution_map(art, p, ss, 6, 5, pts, return_status=True, **kw)
    short = bg.evolution_map(art, p, ss, 6, 5, pts, **kw)
    state2, n_end2, status2 = bg.horizon_exit_map(art, p, ss, 6, 5, N_star=53.0, derivatives_init=d, return_status=True)
    assert np.array_equal(state, state2, equal_nan=True) and np.array_equal(n_end, n_end2, equal_nan=True)
    found = status2 == TARGET
    assert 0 < found.sum() < 30 and p_r.shape == p_s.shape == c_rs.shape == (6, 5, 4) and status.shape == (6, 5)
    flat = state2[found]
    ev = bg.spectra_evolution(art, p, [3.0], pts, flat[:, :2], flat[:, 2:4], since="exit", N_sub=3.0, max_steps=100_000)
    assert np.all(ev.status == ENDED)
    for grid, member in ((p_r, ev.P_R), (p_s, ev.P_S), (c_rs, ev.C_RS)):
        assert np.array_equal(grid[found], member[:, 0]) and np.isfinite(grid[found]).all() and np.isnan(grid[~found]).all()
    assert np.array_equal(status[found], ev.status[:, 0]) and np.array_equal(status[~found], status2[~found])
    assert len(short) == 3 and all(np.array_equal(u, w, equal_nan=True) for u, w in zip(short[0], (p_r, p_s, c_rs)))
    assert np.all(p_s[found][:, -1] < p_s[found][:, 1])  # (the isocurvature power decays after the exit)


def test_evolution_object_refusals(bg):
    """An object built with -DINFLX_EV_ABI_VERSION=2 is refused with INFLX_ERR_VERSION, a missing one is INFLX_ERR_SYMBOL with the way
    to build it; the artefact's own build then replaces the refused file and works on the same handle."""
    from background_reference import power_law_artifact, power_law_init
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".evolution"
    headers = {stale + ".model.h": header_text, stale + ".eom.h": art.eom_header_text(), stale + ".kin.h": art.kinematics_header_text(),
               stale + ".mass.h": art.masses_header_text()}  # fmt: skip
    init = np.array([power_law_init()], dtype=np.float64)
    p = np.ascontiguousarray(p, dtype=np.float64)
    kappa, target, shift, pts = np.array([100.0]), np.array([1e-3]), np.array([0.0]), np.array([0.0, 5e-4])
    out, sampled, status = np.empty((22, 1)), np.empty((2, 6, 1)), np.empty(1, dtype=np.int8)
    dp = C.POINTER(C.c_double)

    def raw(lib):  # the C entry point's own return code
        return lib._lib.inflx_mode_evolution(lib._h, p.ctypes.data_as(dp), 1, lib.n_parameters, init.ctypes.data_as(dp), 1, kappa.ctypes.data_as(dp), target.ctypes.data_as(dp),
                                             shift.ctypes.data_as(dp), pts.ctypes.data_as(dp), 2, 1000, _native.EOM_RKF, 1e-8, 0.0, 0, out.ctypes.data_as(dp),
                                             sampled.ctypes.data_as(dp), None, status.ctypes.data_as(C.POINTER(C.c_int8)))  # fmt: skip

    call = (p, init, kappa, target, shift, pts, 1000, _native.EOM_RKF, 1e-8, 0.0, 0)
    try:
        if os.path.exists(stale):
            os.remove(stale)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        assert raw(lib) == _native.ERR_SYMBOL
        with pytest.raises(SystemError, match=r"ensure_evolution\(\)") as err:
            lib.mode_evolution(*call)
        assert ".evolution exists" in str(err.value)
        for path, text in headers.items():
            with open(path, "w") as fh:
                fh.write(text)
        hdr, eom_hdr, kin_hdr, mass_hdr = headers
        cmd = [hipcc_path(), *options, "-DINFLX_EV_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_KIN_HEADER="{kin_hdr}"', f'-DINFLX_MASS_HEADER="{mass_hdr}"',
               os.path.join(_CSRC, "inflx_evolution_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        assert raw(lib) == _native.ERR_VERSION
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.mode_evolution(*call)
        assert "INFLX_EV_ABI 2, expected 1" in str(err.value)
        os.remove(stale)
        art.ensure_evolution()
        got = lib.mode_evolution(*call)
        assert got[0].shape == (22, 1) and got[1].shape == (2, 6, 1) and got[3][0] == TARGET and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        # the checks of the samples and the shift, at the C entry point
        for bad_pts, bad_shift in (([0.0, 0.0], [0.0]), ([1.0, 0.5], [0.0]), ([0.0, np.nan], [0.0]), ([0.0, 1.0], [np.inf])):
            with pytest.raises(ValueError):
                lib.mode_evolution(p, init, kappa, target, np.array(bad_shift), np.array(bad_pts), 1000, _native.EOM_RKF, 1e-8, 0.0, 0)
        with pytest.raises(ValueError):
            lib.mode_evolution(p, init, kappa, target, shift, pts, 1000, _native.EOM_RKF, 1e-8, 0.0, _native.MODES_TENSOR)
        lib.close()
    finally:
        for path in (stale, *headers):
            if os.path.exists(path):
                os.remove(path)


def test_mode_spectra_is_untouched_by_an_evolution_call(bg, hyper):
    """``inflx_mode_spectra`` on one handle before and after ``inflx_mode_evolution`` on it: the same results, bit for bit."""
    p, art, _twin = hyper
    x, v = mo.hyper_states(3)
    init = np.concatenate([x, v], axis=1)
    kappa = 20.0 * mo.friedmann_h(er.modes_twin_for("hyperbolic"), p, init)
    before = _md(bg, art, p, init, kappa, 0.5)
    out, sampled, n_end, status = _ev(bg, art, p, init, kappa, 0.5, 0.0, np.array([0.0, 0.25, 0.5]))
    after = _md(bg, art, p, init, kappa, 0.5)
    assert np.all(before[2] == TARGET) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    assert np.array_equal(out, before[0]) and np.array_equal(status, before[2]) and np.array_equal(sampled[2], out[PLANES])
