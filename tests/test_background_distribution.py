"""The first-passage histograms on the host build (tests/distribution_twin.cpp compiles csrc/inflx_distribution.h for the CPU and runs
the L lanes of a point serially with a shared ticket): the twin's integers against the stated bin rule applied in numpy to the samples of
the stochastic twin, lane order, offsets of the first realisation and the sum of two results, the law against independent random
numbers, the host helpers, the front end's argument checks, the public surface, and the twin under sanitizers."""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import distribution_reference as dr
import stochastic_reference as sr
import workloads
from conftest import ROOT
from stochastic_reference import ENDED

BINS = 24
NARROW, WIDE = (9.0, 10.0), (8.0, 13.5)


@pytest.fixture(scope="module")
def hyper():
    _spec, art, _model, p = sr.hyperbolic_case()
    return art, p, sr.StochasticTwin(art), dr.DistributionTwin(art)


@pytest.fixture(scope="module")
def parity_samples(hyper):
    """the samples every histogram here is a binning of, computed once: {(solver, max_steps): StochasticTwin run, R = 130}"""
    _art, p, twin, _pd = hyper
    return {(solver, ms): twin.run(p, sr.PARITY_POINTS, sr.PARITY_R, seed=sr.PARITY_SEED, noise_scale=sr.PARITY_SCALE, max_steps=ms, solver=solver, dt=sr.PARITY_DT)
            for solver in ("rk4", "rkf") for ms in (600, 320)}  # fmt: skip


def _expected(run, R, N_range, first=0, total=sr.PARITY_R):
    n, s = run.N.reshape(3, total)[:, first : first + R], run.status.reshape(3, total)[:, first : first + R]
    rows, counts = zip(*(dr.bin_samples(n[b], s[b], *N_range, BINS) for b in range(3)))
    return np.stack(rows), np.stack(counts)


def _kw(solver, max_steps):
    return dict(seed=sr.PARITY_SEED, noise_scale=sr.PARITY_SCALE, max_steps=max_steps, solver=solver, dt=sr.PARITY_DT)


@pytest.mark.parametrize("max_steps", [600, 320])
@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_the_twins_histogram_is_the_binning_of_the_samples(hyper, parity_samples, solver, max_steps):
    """R = 130 on 64 lanes (every lane is used again, and 130 is no multiple of 64) and R = 40 (24 lanes retired from the start); 600
    steps end every realisation, 320 leave some that count as RUNNING.  hist, below, above and counts are numpy's application of the
    rule to the stochastic twin's samples, exactly -- over a narrow range that leaves realisations on both sides and a wide one that
    holds at least 90 per cent of those that ended."""
    _art, p, _twin, pd = hyper
    run = parity_samples[solver, max_steps]
    for R in (130, 40):
        for N_range in (NARROW, WIDE):
            rows, counts = _expected(run, R, N_range)
            got = pd.run(p, sr.PARITY_POINTS, R, BINS, N_range, lanes_per_point=64, **_kw(solver, max_steps))
            assert np.array_equal(got.rows, rows) and np.array_equal(got.counts, counts), (R, N_range, got.rows, rows)
            assert np.all(got.counts.sum(axis=1) == R) and np.array_equal(got.rows.sum(axis=1), counts[:, ENDED])
            ended = counts[:, ENDED]
            if N_range == WIDE:
                assert np.all(got.hist.sum(axis=1) >= 0.9 * ended)
            elif max_steps == 600 and R == 130:
                assert np.any((got.below > 0) & (got.above > 0)) and got.hist.sum() > 0
            assert (max_steps == 600) == bool(np.all(ended == R)) and (max_steps == 600 or counts[:, sr.RUNNING].sum() > 0.2 * R)
    # a window of 7 units in place of 256 -- more launches, fresh starts at every offset of a window -- and 128 lanes change nothing
    rows, counts = _expected(run, 130, WIDE)
    for kw in (dict(window=7), dict(lanes_per_point=128), dict(lanes_per_point=192, window=1)):
        got = pd.run(p, sr.PARITY_POINTS, 130, BINS, WIDE, **{**_kw(solver, max_steps), **kw})
        assert np.array_equal(got.rows, rows) and np.array_equal(got.counts, counts), kw


def test_the_bin_rule_on_the_host_is_numpys(hyper):
    """inflx_pd_slot against numpy on values at, beside and far from the edges: N = lo is bin 0, N = hi is above, N < lo below."""
    pd = hyper[3]
    lo, hi, bins = 8.0, 13.5, 24
    edges = lo + np.arange(bins + 1) * ((hi - lo) / bins)
    values = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), [-1e300, 0.0, 1e300, lo - 1e-9, hi + 1e-9],
                             np.random.default_rng(5).uniform(lo - 1.0, hi + 1.0, 4000)])  # fmt: skip
    got = pd.slots(values, lo, hi, bins)
    for v, slot in zip(values, got):
        row, _ = dr.bin_samples([v], [ENDED], lo, hi, bins)
        assert row[slot] == 1, (v, slot)
    assert got[0] == 1 and got[bins] == bins + 1 and got[bins + 1] == 0 and got[2 * bins + 1] == bins


def test_lane_order_does_not_matter(hyper, parity_samples):
    """The lanes of every launch served in reversed and in a shuffled order draw other tickets and give the same integers."""
    _art, p, _twin, pd = hyper
    for solver, max_steps in (("rkf", 600), ("rk4", 320)):
        rows, counts = _expected(parity_samples[solver, max_steps], 130, WIDE)
        for order in (np.arange(64)[::-1], np.random.default_rng(11).permutation(64)):
            got = pd.run(p, sr.PARITY_POINTS, 130, BINS, WIDE, lanes_per_point=64, order=order, window=50, **_kw(solver, max_steps))
            assert np.array_equal(got.rows, rows) and np.array_equal(got.counts, counts)


def _as_result(background, got, N_range, R, first, seed=sr.PARITY_SEED):
    edges = np.tile(N_range[0] + np.arange(BINS + 1) * ((N_range[1] - N_range[0]) / BINS), (3, 1))
    return background.StochasticDistribution(got.hist, got.below, got.above, edges, got.counts, got.counts[:, ENDED], np.full(3, np.nan), R, first, seed)


def test_first_realisation_and_the_sum_of_two_results(hyper, parity_samples):
    """R = 64 from 0 plus R = 66 from 64 is R = 130 from 0, and each part is the binning of its own samples; ``+`` agrees, either way
    round, and refuses other edges, another seed, a gap and an overlap."""
    from inflatox_amd import background

    _art, p, _twin, pd = hyper
    run, kw = parity_samples["rkf", 600], _kw("rkf", 600)
    a = pd.run(p, sr.PARITY_POINTS, 64, BINS, WIDE, **kw)
    b = pd.run(p, sr.PARITY_POINTS, 66, BINS, WIDE, first_realisation=64, **kw)
    whole = pd.run(p, sr.PARITY_POINTS, 130, BINS, WIDE, **kw)
    assert np.array_equal(a.rows, _expected(run, 64, WIDE)[0]) and np.array_equal(b.rows, _expected(run, 66, WIDE, first=64)[0])
    assert np.array_equal(a.rows + b.rows, whole.rows) and np.array_equal(a.counts + b.counts, whole.counts) and not np.array_equal(a.rows, b.rows)
    ra, rb, rw = _as_result(background, a, WIDE, 64, 0), _as_result(background, b, WIDE, 66, 64), _as_result(background, whole, WIDE, 130, 0)
    for total in (ra + rb, rb + ra):
        assert all(np.array_equal(getattr(total, f), getattr(rw, f), equal_nan=True) for f in rw._fields)
    with pytest.raises(ValueError, match="edges"):
        ra + _as_result(background, b, NARROW, 66, 64)
    with pytest.raises(ValueError, match="seed"):
        ra + _as_result(background, b, WIDE, 66, 64, seed=1)
    for first in (65, 63, 0):
        with pytest.raises(ValueError, match="adjoin"):
            ra + _as_result(background, b, WIDE, 66, first)
    with pytest.raises(TypeError):
        ra + (1, 2)


def test_in_law_against_independent_random_numbers(hyper):
    """The comparison the GPU test makes, on the host twin first: the LAW case (adaptive rkf, R = 2^14) against the numpy restatement
    driven by numpy's own generator, 64 bins over N_classical - 4 .. N_classical + 8, neighbours merged to at least 40 pooled counts:
    chi2 <= dof + 5 sqrt(2 dof) at every point."""
    art, p, twin, pd = hyper
    _spec, _art, model, _p = sr.hyperbolic_case()
    R = sr.LAW_R
    kw = dict(noise_scale=sr.LAW_SCALE, dN_max=sr.LAW_DN_MAX, max_err=1e-8, solver="rkf")
    classical = twin.run(p, sr.LAW_POINTS, 1, **dict(kw, noise_scale=0.0)).N
    ranges = np.stack([classical - 4.0, classical + 8.0], axis=1)
    got = pd.run(p, sr.LAW_POINTS, R, 64, ranges, lanes_per_point=1024, seed=0, **kw)
    want = sr.restatement_of(model, art, p).run(sr.LAW_POINTS, R, rng=np.random.default_rng(20240229), **kw)
    assert np.all(want.status == ENDED) and np.all(got.counts[:, ENDED] == R)
    for b in range(3):
        row, _counts = dr.bin_samples(want.N.reshape(3, R)[b], want.status.reshape(3, R)[b], *ranges[b], 64)
        chi2, dof = dr.chi2_two_samples(got.rows[b], row, least=40)
        print(f"point {b}: chi2 {chi2:.1f} with {dof} degrees of freedom (bound {dof + 5.0 * math.sqrt(2.0 * dof):.1f})")
        assert dof >= 10 and chi2 <= dof + 5.0 * math.sqrt(2.0 * dof)


def _binned_result(background, samples, lo, hi, bins):
    row, counts = dr.bin_samples(samples, np.full(samples.size, ENDED), lo, hi, bins)
    edges = lo + np.arange(bins + 1) * ((hi - lo) / bins)
    return background.StochasticDistribution(row[None, 1:-1], row[None, 0], row[None, -1], edges[None], counts[None], counts[None, ENDED], np.array([np.nan]),
                                             samples.size, 0, 0)  # fmt: skip


@pytest.mark.parametrize("rate,width,bins", [(2.0, 0.05, 200), (0.5, 0.125, 200), (4.0, 0.01, 200), (4.0, 0.025, 20)])
def test_tail_rate_of_binned_exponentials(rate, width, bins):
    """n = 10^5 exponentials above N_from = 3, binned with Lambda width <= 0.1 up to hi, the rest censored in ``above``: the midpoint
    bias is below (Lambda width)^2 / 12 < 1e-3 relative and the standard error Lambda / sqrt(n_in) about 3e-3, so the estimate is within
    5 standard errors of Lambda; and so is the estimate from an edge further up the tail.  The last case censors 13.5 per cent."""
    from inflatox_amd import background

    assert rate * width <= 0.1
    n = 100_000
    samples = 3.0 + np.random.default_rng(int(rate * 100) + bins).exponential(1.0 / rate, n)
    d = _binned_result(background, samples, 3.0, 3.0 + bins * width, bins)
    assert d.below[0] == 0 and d.hist.sum() + d.above[0] == n
    for start in (3.0, 3.0 + 10.3 * width, 2.0):
        got, err = background.distribution_tail_rate(d, start)
        print(f"Lambda {rate}, width {width}, from {start}: {got[0]:.5f} +- {err[0]:.5f}, above {d.above[0]}")
        n_in = d.hist[0, int(np.searchsorted(d.edges[0], start)) :].sum()
        assert got.shape == err.shape == (1,) and abs(got[0] - rate) <= 5.0 * err[0] and err[0] == got[0] / math.sqrt(n_in)
        assert start > 3.0 or (n_in == n - d.above[0] and err[0] <= 3.5e-3 * rate)
    assert np.isnan(background.distribution_tail_rate(d, 1e9)[0][0])


def test_pdf_survival_and_mean(hyper, parity_samples):
    from inflatox_amd import background

    run = parity_samples["rkf", 600]
    for N_range in (NARROW, WIDE):
        rows, counts = _expected(run, 130, N_range)
        d = _as_result(background, dr.TwinDistribution(rows, counts, 0), N_range, 130, 0)
        inside, n_ended = d.hist.sum(axis=1), d.n_ended
        surv = background.distribution_survival(d)
        assert surv.shape == (3, BINS + 1) and np.array_equal(surv[:, 0], (inside + d.above) / n_ended) and np.array_equal(surv[:, -1], d.above / n_ended)
        assert np.all(np.diff(surv, axis=1) <= 0.0)
        pdf = background.distribution_pdf(d)
        width = (N_range[1] - N_range[0]) / BINS
        assert pdf.shape == d.hist.shape and np.allclose(pdf.sum(axis=1) * width, inside / n_ended, rtol=1e-14, atol=0.0)
        n = run.N.reshape(3, 130)
        want = np.array([n[b][(n[b] >= N_range[0]) & (n[b] < N_range[1])].mean() for b in range(3)])
        assert np.all(np.abs(background.distribution_mean(d) - want) <= width / 2)
    empty = _as_result(background, dr.TwinDistribution(np.zeros((3, BINS + 2), dtype=np.int64), np.zeros((3, 6), dtype=np.int64), 0), WIDE, 130, 0)
    assert np.isnan(background.distribution_pdf(empty)).all() and np.isnan(background.distribution_survival(empty)).all() and np.isnan(background.distribution_mean(empty)).all()
    # maps: the helpers keep the leading shape
    grid = background.StochasticDistribution(*(np.asarray(a).reshape(3, 1, *np.shape(a)[1:]) for a in d[:7]), *d[7:])
    assert background.distribution_survival(grid).shape == (3, 1, BINS + 1) and background.distribution_mean(grid).shape == (3, 1)
    assert background.distribution_tail_rate(grid, 9.0)[0].shape == (3, 1)


def test_bad_arguments_raise_before_the_device(monkeypatch):
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    for ensure in ("ensure_stochastic", "ensure_distribution", "ensure_background"):
        monkeypatch.setattr(CompilationArtifact, ensure, no_device)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = np.zeros((3, 2)) + 2.0, np.zeros((3, 2)) + 0.1
    shape, value = _native.InflatoxShapeError, ValueError
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    bad = (dict(seed=-1), dict(seed=2**64), dict(seed=1.5), dict(noise_scale=-1.0), dict(noise_scale=float("nan")), dict(noise_scale=float("inf")), dict(noise_scale="abc"),
           dict(dN_max=0.0), dict(dN_max=-1.0), dict(dN_max=float("nan")), dict(max_steps=0), dict(max_steps=2.5), dict(max_err=0.0), dict(max_err=float("nan")),
           dict(solver="euler"), dict(dt=0.0), dict(dt=float("inf")), dict(first_realisation=-1), dict(first_realisation=2**32 - 7), dict(first_realisation=1.5),
           dict(lanes_per_point=0), dict(lanes_per_point=96), dict(lanes_per_point=-64), dict(lanes_per_point=2**20 + 64), dict(lanes_per_point=64.0),
           dict(centre="mean"), dict(centre=0.0))  # fmt: skip
    ok_range = (0.0, 20.0)
    bad_ranges = ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0), (-float("inf"), 0.0), (-1e308, 1e308), ("a", "b"))
    for kw in bad:
        with pytest.raises(value):
            background.stochastic_distribution(art, p, x, v, 8, 16, ok_range, **kw)
    for kw in (dict(streams=[0, 1, -1]), dict(streams=[0, 1, 2**32]), dict(streams=[0.5, 1.0, 2.0])):
        with pytest.raises(value):
            background.stochastic_distribution(art, p, x, v, 8, 16, ok_range, **kw)
    for R in (0, -1, 2**32, 2.5, "abc"):
        with pytest.raises(value):
            background.stochastic_distribution(art, p, x, v, R, 16, ok_range)
    for bins in (0, -3, 2**20 + 1, 1.5, "abc"):
        with pytest.raises(value):
            background.stochastic_distribution(art, p, x, v, 8, bins, ok_range)
    for N_range in (*bad_ranges, [[0.0, 1.0], [0.0, 1.0], [1.0, 0.5]]):
        for centre in (None, "classical"):
            with pytest.raises(value):
                background.stochastic_distribution(art, p, x, v, 8, 16, N_range, centre=centre)
    for args, kw in (((p[:2], x, v, 8, 16, ok_range), {}), ((np.zeros((2, p.size)), x, v, 8, 16, ok_range), {}), ((p, x, v[:2], 8, 16, ok_range), {}),
                     ((p, np.zeros((3, 3)), np.zeros((3, 3)), 8, 16, ok_range), {}), ((p, x[0], v[0], 8, 16, ok_range), {}), ((p, x, v, 8, 16, ok_range), dict(streams=[1, 2])),
                     ((p, x, v, 8, 16, (0.0, 1.0, 2.0)), {}), ((p, x, v, 8, 16, np.zeros((2, 2)) + [0.0, 1.0]), {}), ((p, x, v, 8, 16, np.zeros((3, 3))), {})):  # fmt: skip
        with pytest.raises(shape):
            background.stochastic_distribution(art, *args, **kw)
    with pytest.raises(shape):
        background.stochastic_distribution(three, np.zeros(3), x, v, 8, 16, ok_range)
    grid = ([[1.5, 4.0], [-1.0, 1.0]], 3, 3)
    for kw in bad:
        with pytest.raises(value):
            background.stochastic_distribution_map(art, p, *grid, 8, 16, (-2.0, 2.0), **kw)
    for R in (0, 2**32):
        with pytest.raises(value):
            background.stochastic_distribution_map(art, p, *grid, R, 16, (-2.0, 2.0))
    for bins in (0, 2**20 + 1):
        with pytest.raises(value):
            background.stochastic_distribution_map(art, p, *grid, 8, bins, (-2.0, 2.0))
    for N_range in bad_ranges:
        with pytest.raises(value):
            background.stochastic_distribution_map(art, p, *grid, 8, 16, N_range)
    with pytest.raises(value):
        background.stochastic_distribution_map(art, p, grid[0], 0, 3, 8, 16, (-2.0, 2.0))
    for args, kw in (((p, [1.0, 2.0, 3.0], 3, 3, 8, 16, (-2.0, 2.0)), {}), ((np.zeros((9, p.size)), *grid, 8, 16, (-2.0, 2.0)), {}),
                     ((p, *grid, 8, 16, (-2.0, 2.0)), dict(derivatives_init=(0.0, 0.0, 0.0))), ((p, *grid, 8, 16, np.zeros((4, 2)) + [0.0, 1.0]), {})):  # fmt: skip
        with pytest.raises(shape):
            background.stochastic_distribution_map(art, *args, **kw)
    with pytest.raises(TypeError):
        background.stochastic_distribution_map(art, p, *grid, 8, 16, (-2.0, 2.0), streams=[1] * 9)  # (the stream of a point is its index)
    with pytest.raises(TypeError):
        background.stochastic_distribution(art, p, x, v, 8, 16, ok_range, N_stop=1.0)  # (every N would be the same)


def test_public_names_and_unchanged_surface():
    import ctypes
    import inspect
    import re

    from inflatox_amd import _native, background
    from inflatox_amd.compiler import _DISTRIBUTION_SOURCES, _STOCHASTIC_SOURCES, KERNEL_GROUPS, CompilationArtifact

    names = {"stochastic_distribution", "stochastic_distribution_map", "StochasticDistribution", "distribution_pdf", "distribution_survival", "distribution_mean",
             "distribution_tail_rate"}  # fmt: skip
    assert names <= set(background.__all__) and all(name in background.__doc__ for name in names - {"StochasticDistribution"})
    assert background.StochasticDistribution._fields == ("hist", "below", "above", "edges", "counts", "n_ended", "N_classical", "realisations", "first_realisation", "seed")
    sig = inspect.signature(background.stochastic_distribution)
    assert list(sig.parameters) == ["artifact", "pars", "fields_init", "derivatives_init", "realisations", "bins", "N_range", "centre", "seed", "streams",
                                    "first_realisation", "lanes_per_point", "noise_scale", "dN_max", "max_steps", "max_err", "solver", "dt"]  # fmt: skip
    assert [sig.parameters[k].default for k in list(sig.parameters)[7:]] == [None, 0, None, 0, None, 1.0, 1 / 32, 1_000_000, 1e-8, "rkf", None]
    assert inspect.signature(background.stochastic_distribution_map).parameters["centre"].default == "classical"
    assert callable(CompilationArtifact.ensure_distribution) and "distribution" not in KERNEL_GROUPS
    assert _DISTRIBUTION_SOURCES == ("inflx_distribution_kernels.hip", "inflx_distribution.h", "inflx_distribution_abi.h", "inflx_stochastic.h", "inflx_philox.h",
                                     "inflx_background.h", "inflx_background_abi.h") and _DISTRIBUTION_SOURCES[3:] == _STOCHASTIC_SOURCES[1:2] + _STOCHASTIC_SOURCES[3:]  # fmt: skip
    assert list(_native.DISTRIBUTION_SIGNATURES) == ["inflx_stochastic_distribution"]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inflx_hip_distribution.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(inflx_[a-z_0-9]+)\s*\(", text))) == ["inflx_stochastic_distribution"]
    assert '#include "inflx_hip_distribution.h"' in open(os.path.join(ROOT, "include", "inflx_hip.h")).read()
    assert len(_native.DISTRIBUTION_SIGNATURES["inflx_stochastic_distribution"][1]) == 22
    assert not set(_native.DISTRIBUTION_SIGNATURES) & (set(_native.SIGNATURES) | set(_native.DELTAN_SIGNATURES) | set(_native.EVOLUTION_SIGNATURES)
                                                       | set(_native.STOCHASTIC_SIGNATURES))  # fmt: skip
    _native.build_library()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "inflx_stochastic_distribution") and callable(_native.InflatoxDevLib.stochastic_distribution)
    csrc = os.path.join(ROOT, "inflatox_amd", "csrc")
    # the stochastic object's layout word is still 1, and the new object has one of its own
    assert re.search(r"#define INFLX_ST_ABI_VERSION 1\b", open(os.path.join(csrc, "inflx_stochastic_abi.h")).read())
    assert re.search(r"#define INFLX_PD_ABI_VERSION 1\b", open(os.path.join(csrc, "inflx_distribution_abi.h")).read())
    assert (_native.PD_MAX_REALISATIONS, _native.PD_MAX_BINS, _native.PD_MAX_LANES_PER_POINT, _native.ST_MAX_REALISATIONS) == (2**32 - 1, 1 << 20, 1 << 20, 1 << 20)


def test_twin_program_under_address_and_ub_sanitizers(tmp_path, hyper):
    """tests/distribution_twin.cpp as a stand-alone program (DISTRIBUTION_TWIN_MAIN) under ASan + UBSan on the CPU: two points x 150
    realisations on 64 lanes, both steppers, adaptive to the end of inflation and at a fixed dt with 40 steps that no realisation ends in."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not available")
    _art, p, _twin, pd = hyper
    exe = str(tmp_path / "distribution_twin")
    cmd = [gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DDISTRIBUTION_TWIN_MAIN",
           *sr.StochasticTwin.compile_options(*pd.headers), pd.source, "-o", exe]  # fmt: skip
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe, *map(repr, p.tolist())], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 8 and all("realisations 150," in ln for ln in lines), run.stdout[-3000:]
    assert sum("fixed 0" in ln and "ended 150, running 0," in ln for ln in lines) == 4 and sum("fixed 1" in ln and "ended 0, running 150," in ln for ln in lines) == 4
