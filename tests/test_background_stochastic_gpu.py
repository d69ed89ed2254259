"""The stochastic e-folds on the GPU (inflatox_amd.background.stochastic_efolds, stochastic_map, InflatoxDevLib.stochastic_efolds): every
lane against the host twin at a fixed dt across launch windows, reproducibility bit for bit (seed, R, streams, placement, passes), the
two exact diffusions, the moments against an independent stream of random numbers in law, the device reduction against numpy on the
returned samples, the map against the batch call, the classical limit against solve_eom_batch bit for bit, and the refusal of an
object of another layout.  Twin, restatement, cases and bounds are those tests/test_background_stochastic.py establishes on the host
build (tests/stochastic_reference.py, profiles/background_stochastic.json).  Every difference and z-score is printed."""

import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import stochastic_reference as sr
import workloads
from stochastic_reference import ENDED, TARGET

pytestmark = pytest.mark.gpu

MOMENTS = ("N_mean", "N_var", "N_m3", "N_m4", "N_min", "N_max", "n_ended", "counts", "N_classical")


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper():
    _spec, art, _model, p = sr.hyperbolic_case()
    return art, p


def _same(a, b, fields=MOMENTS, rows=slice(None)):
    return all(np.array_equal(getattr(a, f)[rows], getattr(b, f), equal_nan=True) for f in fields)


def _result(se):
    return sr.StochasticResult(se.N.reshape(-1), se.state.reshape(-1, 5), se.status.reshape(-1).astype(np.int64), None, None)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", ["hyperbolic", "egno"])
def test_every_lane_is_the_twins(bg, name, solver):
    """B = 3, R = 130 (two full wavefronts and a partial one per point, points that share wavefronts), 600 steps at a fixed dt: lanes
    cross two launch windows and the step counter goes on.  N, the state and the status of every lane within 1e-10 + 2 d of the twin's."""
    if name == "hyperbolic":
        _spec, art, _model, p = sr.hyperbolic_case()
        pts, dt, scale = sr.PARITY_POINTS, sr.PARITY_DT, sr.PARITY_SCALE
    else:
        spec, art = workloads.artifact_for("egno")
        p, pts, dt, scale = np.asarray(spec.args, dtype=np.float64), sr.EGNO_POINTS, sr.EGNO_DT, sr.EGNO_SCALE
    kw = dict(seed=sr.PARITY_SEED, noise_scale=scale, max_steps=sr.PARITY_STEPS, solver=solver, dt=dt)
    got = bg.stochastic_efolds(art, p, pts[:, :2], pts[:, 2:], sr.PARITY_R, return_samples=True, **kw)
    want = sr.StochasticTwin(art).run(p, pts, sr.PARITY_R, **kw)
    diff = sr.lane_difference(_result(got), want)
    print(f"{name} {solver}: worst |GPU - twin| over the lanes {diff:.3e} (bound {sr.bound():.3e}); statuses {np.bincount(want.status)}; steps up to {want.accepted.max()}")
    assert want.accepted.max() > 256 and diff <= sr.bound()
    assert np.array_equal(got.counts, np.stack([np.bincount(s, minlength=6) for s in want.status.reshape(3, -1)]))


def test_reproducible_bit_for_bit(bg, hyper):
    """The same seed gives the same result and another seed another; R = 64 is a prefix of R = 128; a point alone with its stream is the
    point inside a batch of 5."""
    art, p = hyper
    x, v = sr.PARITY_POINTS[:, :2], sr.PARITY_POINTS[:, 2:]
    kw = dict(noise_scale=sr.PARITY_SCALE, dN_max=0.125, return_samples=True)
    a = bg.stochastic_efolds(art, p, x, v, 128, seed=5, **kw)
    b = bg.stochastic_efolds(art, p, x, v, 128, seed=5, **kw)
    c = bg.stochastic_efolds(art, p, x, v, 128, seed=6, **kw)
    assert _same(a, b, MOMENTS + ("N", "state", "status")) and np.all(a.status == ENDED)
    assert not np.array_equal(a.N, c.N) and not np.array_equal(a.N_mean, c.N_mean) and np.array_equal(a.N_classical, c.N_classical)
    half = bg.stochastic_efolds(art, p, x, v, 64, seed=5, **kw)
    assert np.array_equal(half.N, a.N[:, :64]) and np.array_equal(half.state, a.state[:, :64]) and np.array_equal(half.status, a.status[:, :64])
    five_x, five_v = np.concatenate([x, x[:2] + 0.05]), np.concatenate([v, v[:2]])
    streams = [11, 12, 4242, 14, 15]
    batch = bg.stochastic_efolds(art, p, five_x, five_v, 128, seed=5, streams=streams, **kw)
    alone = bg.stochastic_efolds(art, p, five_x[2:3], five_v[2:3], 128, seed=5, streams=[4242], **kw)
    assert _same(batch, alone, MOMENTS + ("N", "state", "status"), rows=slice(2, 3))
    # the default stream is the point's index: the realisations of two points that start alike do not share their noise
    twice = bg.stochastic_efolds(art, p, np.repeat(x[:1], 2, axis=0), np.repeat(v[:1], 2, axis=0), 128, seed=5, **kw)
    assert np.array_equal(twice.N[0], a.N[0]) and not np.array_equal(twice.N[1], twice.N[0])


def test_two_passes_are_the_single_point_calls(bg):
    """B = 5, R = 2^18 + 3 with N_stop after 8 steps: 5 R lanes are more than a pass holds (2^20), so the call takes two passes of whole
    points; every point's moments and samples are those of the call with that point alone and its stream."""
    art, p, init, dt = sr.constant_case(True, device=True)
    R = (1 << 18) + 3
    x = np.array([[1.5, 0.25], [1.2, 0.0], [2.0, -0.5], [0.9, 1.0], [1.7, 0.3]])
    v = np.zeros_like(x)
    kw = dict(seed=77, N_stop=0.5, dt=dt, solver="rk4", return_samples=True)
    whole = bg.stochastic_efolds(art, p, x, v, R, **kw)
    assert np.all(whole.status == TARGET) and np.all(whole.counts[:, TARGET] == R) and whole.N.shape == (5, R)
    for b in range(5):
        one = bg.stochastic_efolds(art, p, x[b : b + 1], v[b : b + 1], R, streams=[b], **kw)
        assert _same(whole, one, MOMENTS + ("N", "state", "status"), rows=slice(b, b + 1)), b
    assert not np.array_equal(whole.state[0, :, 0], whole.state[4, :, 0]) and whole.state[0, :, 0].std() > 0.05


@pytest.mark.parametrize("curved", [False, True])
def test_exact_diffusion(bg, curved):
    """Items 5 and 6 of tests/test_background_stochastic.py on the device, the same 5 standard errors."""
    art, p, init, dt = sr.constant_case(curved, device=True)
    R = 1 << 16
    got = bg.stochastic_efolds(art, p, init[:, :2], init[:, 2:], R, seed=0, N_stop=sr.N_DIFFUSE, dt=dt, solver="rk4", max_steps=1000, return_samples=True)
    sr.diffusion_checks(curved, got.N[0], got.state[0], got.status[0], R)
    assert got.counts[0, TARGET] == R and got.n_ended[0] == 0 and np.isnan(got.N_mean[0])


def test_moments_against_an_independent_stream(bg, hyper):
    """Hyperbolic, adaptive rkf, three points 8 to 12 e-folds before the end, noise_scale 0.4 (std(N) / N about 10 per cent), R = 2^14,
    seed 0: N_mean within 5 combined standard errors and N_var within 5 var sqrt(4 / (R - 1)) of the restatement driven by numpy's own
    generator; every realisation ends on both sides."""
    art, p = hyper
    _spec, _art, model, _p = sr.hyperbolic_case()
    R = sr.LAW_R
    kw = dict(noise_scale=sr.LAW_SCALE, dN_max=sr.LAW_DN_MAX, max_err=1e-8, solver="rkf")
    got = bg.stochastic_efolds(art, p, sr.LAW_POINTS[:, :2], sr.LAW_POINTS[:, 2:], R, seed=0, **kw)
    want = sr.restatement_of(model, art, p).run(sr.LAW_POINTS, R, rng=np.random.default_rng(20240229), **kw)
    n = want.N.reshape(3, R)
    assert np.all(want.status == ENDED) and np.all(got.n_ended == R)
    ratio = np.sqrt(got.N_var) / got.N_mean
    z_mean = (got.N_mean - n.mean(axis=1)) / np.sqrt(got.N_var / R + n.var(axis=1) / R)
    z_var = (got.N_var - n.var(axis=1)) / (n.var(axis=1) * math.sqrt(4.0 / (R - 1)))
    print(f"std(N) / N {ratio}; classical N {got.N_classical}; N_mean {got.N_mean} against {n.mean(axis=1)}: z {z_mean}; N_var {got.N_var} against {n.var(axis=1)}: z {z_var}")
    assert np.all((ratio > 0.05) & (ratio < 0.20)) and np.all((got.N_classical > 8.0) & (got.N_classical < 12.0))
    assert np.all(np.abs(z_mean) <= 5.0) and np.all(np.abs(z_var) <= 5.0)


@pytest.mark.parametrize("B,R", [(1, 1 << 16), (1000, 3)])
def test_device_reduction_against_numpy(bg, hyper, B, R):
    """The moments the reduce kernel returns against numpy (long double) on the samples the same call returns: the mean to 1e-14
    relative, m_k to 1e-12 var^(k/2), extremes and counts exact.  One point whose 2^16 results every thread strides over, and 1000
    points of 3 (most threads idle).  max_steps leaves some realisations of the large case unfinished."""
    art, p = hyper
    rng = np.random.default_rng(B)
    x = np.stack([rng.uniform(6.8, 7.6, B), rng.uniform(-1.0, 1.0, B)], axis=1)
    v = np.tile([-0.8, 1e-4], (B, 1))
    got = bg.stochastic_efolds(art, p, x, v, R, seed=3, noise_scale=sr.LAW_SCALE, dN_max=0.125, max_steps=118 if B == 1 else 100000, return_samples=True)
    assert (got.n_ended.sum() < B * R) == (B == 1) and got.n_ended.min() >= 3
    worst = np.zeros(4)
    for b in range(B):
        ended = got.status[b] == ENDED
        mean, m2, m3, m4 = sr.exact_moments(got.N[b][ended])
        worst = np.maximum(worst, [abs(got.N_mean[b] - mean) / abs(mean), abs(got.N_var[b] - m2) / m2, abs(got.N_m3[b] - m3) / m2**1.5, abs(got.N_m4[b] - m4) / m2**2])
        assert got.N_min[b] == got.N[b][ended].min() and got.N_max[b] == got.N[b][ended].max()
        assert np.array_equal(got.counts[b], np.bincount(got.status[b], minlength=6)) and got.n_ended[b] == ended.sum()
    print(f"B = {B}, R = {R}: worst relative error of the mean {worst[0]:.2e}, of m2, m3, m4 in units of var^(k/2) {worst[1]:.2e} {worst[2]:.2e} {worst[3]:.2e}")
    assert worst[0] <= 1e-14 and np.all(worst[1:] <= 1e-12)


def test_map_is_the_batch_call_on_the_grid(bg, hyper):
    art, p = hyper
    ss = [[6.5, 7.7], [-1.0, 1.0]]
    kw = dict(seed=8, noise_scale=sr.LAW_SCALE, dN_max=0.125)
    got = bg.stochastic_map(art, p, ss, 8, 8, 16, derivatives_init=(-0.8, 0.0), **kw)
    x0, x1 = bg.grid_points(ss, 8, 8)
    x = np.stack([np.repeat(x0, 8), np.tile(x1, 8)], axis=1)
    want = bg.stochastic_efolds(art, p, x, np.tile([-0.8, 0.0], (64, 1)), 16, **kw)
    assert got.N is None and got.N_mean.shape == (8, 8) and got.counts.shape == (8, 8, 6)
    assert all(np.array_equal(getattr(got, f).reshape(getattr(want, f).shape), getattr(want, f), equal_nan=True) for f in MOMENTS)
    assert np.all(got.n_ended == 16)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_noise_scale_zero_is_solve_eom_batch(bg, hyper, solver):
    """noise_scale = 0 on the device: N_end, state and status of every realisation are solve_eom_batch(..., stop_at_end=True)'s, bit for
    bit, at a fixed dt and adaptively with dN_max = inf; with N_stop, state_at_efolds'."""
    art, p = hyper
    x, v = sr.PARITY_POINTS[:, :2], sr.PARITY_POINTS[:, 2:]
    for kw in (dict(dt=sr.PARITY_DT), dict(dt=None, dN_max=math.inf)):
        got = bg.stochastic_efolds(art, p, x, v, 3, noise_scale=0.0, solver=solver, max_err=1e-8, return_samples=True, **kw)
        sol = bg.solve_eom_batch(art, p, 1024, x, v, 1e-8, solver, dt=kw["dt"], stop_at_end=True)
        assert np.all(sol.status == ENDED) and np.all(got.status == ENDED)
        last = sol.states[np.arange(3), sol.last_row]
        assert np.array_equal(got.N, np.repeat(sol.N_end[:, None], 3, axis=1)) and np.array_equal(got.state, np.repeat(last[:, None, :], 3, axis=1))
        assert np.array_equal(got.N_classical, sol.N_end) and np.allclose(got.N_mean, sol.N_end, rtol=1e-15, atol=0.0) and np.all(np.abs(got.N_var) <= 1e-28)
    got = bg.stochastic_efolds(art, p, x, v, 2, noise_scale=0.0, solver=solver, max_err=1e-8, dN_max=math.inf, N_stop=4.0, return_samples=True)
    at = bg.state_at_efolds(art, p, x, v, 4.0, max_err=1e-8, solver=solver)
    assert np.all(got.status == TARGET) and np.all(got.N == 4.0) and np.array_equal(got.state, np.repeat(at.state[:, None, :], 2, axis=1))


def test_stochastic_object_of_another_layout_is_refused(bg):
    """An object built with -DINFLX_ST_ABI_VERSION=2 is refused with INFLX_ERR_VERSION and the "does not belong" message, a missing one
    is INFLX_ERR_SYMBOL with the way to build it; the artefact's own build then replaces the refused file and works on the same handle.
    The C function's own argument checks come before the device."""
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    import background_reference as br

    # (an artefact of its own: no other handle of this process has had its stochastic object loaded from the same path)
    art, p = br.wall_artifact()
    init, dt = np.array([[1.0, 0.0, 0.0, 0.0]]), 5e-2
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".stochastic"
    headers = {stale + ".model.h": header_text, stale + ".eom.h": art.eom_header_text(), stale + ".noise.h": art.noise_header_text()}
    args = (init, 4, None, 1, 1.0, 1.0 / 32.0, 0.25, 1000, _native.EOM_RK4, 1e-8, dt)
    try:
        if os.path.exists(stale):
            os.remove(stale)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        with pytest.raises(SystemError, match=r"ensure_stochastic\(\)") as err:
            lib.stochastic_efolds(p, *args)
        assert ".stochastic exists" in str(err.value)
        for path, text in headers.items():
            with open(path, "w") as fh:
                fh.write(text)
        hdr, eom_hdr, noise_hdr = headers
        cmd = [hipcc_path(), *options, "-DINFLX_ST_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_NOISE_HEADER="{noise_hdr}"', os.path.join(_CSRC, "inflx_stochastic_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.stochastic_efolds(p, *args)
        assert "INFLX_ST_ABI 2, expected 1" in str(err.value)
        os.remove(stale)
        art.ensure_stochastic()
        moments, samples = lib.stochastic_efolds(p, *args, want_samples=True)
        assert moments.shape == (12, 1) and moments[6 + TARGET, 0] == 4 and samples.shape == (7, 4) and np.all(samples[6] == TARGET)
        for bad, words in (((init, 0) + args[2:], "realisations"), ((init, (1 << 20) + 1) + args[2:], "realisations"), (args[:4] + (-1.0,) + args[5:], "noise_scale"),
                           (args[:5] + (0.0,) + args[6:], "dN_max"), (args[:6] + (-1.0,) + args[7:], "N_stop")):  # fmt: skip
            with pytest.raises(Exception, match=words):
                lib.stochastic_efolds(p, *bad)
        lib.close()
    finally:
        for path in (stale, *headers):
            if os.path.exists(path):
                os.remove(path)
        art._companion_paths.pop("stochastic", None)
