"""The first-passage histograms on the GPU (inflatox_amd.background.stochastic_distribution, stochastic_distribution_map,
InflatoxDevLib.stochastic_distribution).  Binding to the existing device path is bit for bit: every expected value is the stated bin
rule applied in numpy (tests/distribution_reference.py ``bin_samples``) to ``stochastic_efolds(..., return_samples=True)`` for the
same seed, streams and options -- so a state that leaks from one realisation of a lane into the next shows as a wrong integer.  Then:
lanes fewer than, equal to and more than the realisations, offsets of the first realisation, two passes, reproducibility, the law
against independent random numbers, the map, and the handling of the object."""

import math
import os
import subprocess

import numpy as np
import pytest

import distribution_reference as dr
import stochastic_reference as sr

pytestmark = pytest.mark.gpu

BINS = 48
RECYCLE_R = 1000
INTEGERS = ("hist", "below", "above", "counts", "n_ended")


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper():
    _spec, art, _model, p = sr.hyperbolic_case()
    return art, p


# the two recycling cases: adaptive rkf as the comparison in law runs it, and rk4 at a fixed dt with a max_steps that leaves
# realisations unfinished (they count as COMPLETE and their lanes go on with the next ticket).  The ranges leave realisations below and
# above on the host twin, and most of them inside.
CASES = {
    "rkf": (dict(noise_scale=sr.LAW_SCALE, dN_max=sr.LAW_DN_MAX, solver="rkf", seed=3), (8.5, 13.0)),
    "rk4": (dict(noise_scale=sr.LAW_SCALE, solver="rk4", dt=sr.PARITY_DT, max_steps=320, seed=sr.PARITY_SEED), (7.0, 9.5)),
}


@pytest.fixture(scope="module")
def samples(bg, hyper):
    """the reference of every case, computed once: stochastic_efolds with samples, R = 1000"""
    art, p = hyper
    x, v = sr.LAW_POINTS[:, :2], sr.LAW_POINTS[:, 2:]
    return {name: bg.stochastic_efolds(art, p, x, v, RECYCLE_R, return_samples=True, **kw) for name, (kw, _range) in CASES.items()}


def _binned(se, N_range, bins=BINS, columns=slice(None)):
    rows, counts = zip(*(dr.bin_samples(n[columns], s[columns], *N_range, bins) for n, s in zip(se.N, se.status)))
    return np.stack(rows), np.stack(counts)


def _is(d, rows, counts):
    return (np.array_equal(d.hist, rows[:, 1:-1]) and np.array_equal(d.below, rows[:, 0]) and np.array_equal(d.above, rows[:, -1])
            and np.array_equal(d.counts, counts) and np.array_equal(d.n_ended, counts[:, sr.ENDED]))  # fmt: skip


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in INTEGERS)


@pytest.mark.parametrize("case", ["rkf", "rk4"])
def test_recycled_lanes_give_the_binned_samples(bg, hyper, samples, case):
    """Three points x 1000 realisations on 64 lanes per point (three points share a workgroup, a lane runs about sixteen
    realisations), on 256 and on the default (1024: the last 24 lanes never start): the same integers, those of the binned samples."""
    art, p = hyper
    kw, N_range = CASES[case]
    rows, counts = _binned(samples[case], N_range)
    ended = counts[:, sr.ENDED]
    print(f"{case}: ended {ended}, statuses {counts.tolist()}, below {rows[:, 0]}, above {rows[:, -1]}")
    assert ended.sum() > 0 and (case == "rkf") == bool(np.all(ended == RECYCLE_R)) and rows[:, 1:-1].sum() > 0.5 * ended.sum()
    if case == "rk4":
        assert counts[:, 0].sum() > 100  # (realisations that ran out of max_steps)
    for L in (64, 256, None):
        got = bg.stochastic_distribution(art, p, sr.LAW_POINTS[:, :2], sr.LAW_POINTS[:, 2:], RECYCLE_R, BINS, N_range, lanes_per_point=L, **kw)
        assert _is(got, rows, counts), (L, got.hist.sum(axis=1), got.counts)
        assert np.all(got.counts.sum(axis=1) == RECYCLE_R) and got.realisations == RECYCLE_R and got.first_realisation == 0
        assert np.array_equal(got.edges, np.tile(N_range[0] + np.arange(BINS + 1) * ((N_range[1] - N_range[0]) / BINS), (3, 1)))


@pytest.mark.parametrize("R", [40, 1])
def test_fewer_realisations_than_lanes(bg, hyper, samples, R):
    """R = 40 on 64 lanes (24 lanes are retired from the start) and R = 1: the first R samples of the R = 1000 call, binned."""
    art, p = hyper
    kw, N_range = CASES["rkf"]
    rows, counts = _binned(samples["rkf"], N_range, columns=slice(0, R))
    got = bg.stochastic_distribution(art, p, sr.LAW_POINTS[:, :2], sr.LAW_POINTS[:, 2:], R, BINS, N_range, lanes_per_point=64, **kw)
    assert _is(got, rows, counts) and np.all(got.n_ended == R)
    default = bg.stochastic_distribution(art, p, sr.LAW_POINTS[:, :2], sr.LAW_POINTS[:, 2:], R, BINS, N_range, **kw)
    assert _same(got, default)


def test_first_realisation_offsets_and_sums(bg, hyper, samples):
    """first_realisation = 500 with R = 500 is the binning of the samples 500 .. 999 of the R = 1000 call, and its sum with the first
    half is the whole."""
    art, p = hyper
    kw, N_range = CASES["rkf"]
    x, v = sr.LAW_POINTS[:, :2], sr.LAW_POINTS[:, 2:]
    second = bg.stochastic_distribution(art, p, x, v, 500, BINS, N_range, first_realisation=500, lanes_per_point=64, **kw)
    assert _is(second, *_binned(samples["rkf"], N_range, columns=slice(500, 1000)))
    first = bg.stochastic_distribution(art, p, x, v, 500, BINS, N_range, lanes_per_point=128, **kw)
    assert _is(first, *_binned(samples["rkf"], N_range, columns=slice(0, 500)))
    whole = first + second
    assert _is(whole, *_binned(samples["rkf"], N_range)) and whole.realisations == 1000 and whole.first_realisation == 0
    assert _same(second + first, whole)
    with pytest.raises(ValueError, match="adjoin"):
        first + first


# five points within about half an e-fold of the end of inflation (the classical runs take 27 to 54 steps of PARITY_DT on the host twin)
NEAR_END = np.array([[2.4, 0.3, -0.75, 1e-4], [2.5, -0.2, -0.75, 1e-4], [2.6, 0.3, -0.75, -1e-4], [2.7, 0.1, -0.75, 1e-4], [2.8, -0.4, -0.75, 2e-4]])


def test_two_passes_are_the_single_point_calls(bg, hyper):
    """B = 5 with 2^18 lanes per point and R = 2^18 + 67: four points fill a pass of 2^20 lanes, so the call takes two passes, and 67
    lanes of every point take a second ticket.  Every point's row is that of the call with the point alone and its stream."""
    art, p = hyper
    L = 1 << 18
    R = L + 67
    kw = dict(seed=77, noise_scale=sr.LAW_SCALE, solver="rk4", dt=sr.PARITY_DT, max_steps=400, lanes_per_point=L)
    whole = bg.stochastic_distribution(art, p, NEAR_END[:, :2], NEAR_END[:, 2:], R, 32, (0.0, 1.6), **kw)
    print(f"two passes: ended {whole.n_ended}, below {whole.below}, above {whole.above}, classical {whole.N_classical}")
    assert np.all(whole.counts.sum(axis=1) == R) and np.all(whole.n_ended > 0.99 * R) and np.all(whole.hist.sum(axis=1) > 0.9 * R)
    assert np.all((whole.N_classical > 0.2) & (whole.N_classical < 0.8))
    for b in range(5):
        one = bg.stochastic_distribution(art, p, NEAR_END[b : b + 1, :2], NEAR_END[b : b + 1, 2:], R, 32, (0.0, 1.6), streams=[b], **kw)
        assert all(np.array_equal(getattr(whole, f)[b : b + 1], getattr(one, f)) for f in INTEGERS), b
    assert not np.array_equal(whole.hist[0], whole.hist[4])


def test_reproducible_and_seeded(bg, hyper):
    art, p = hyper
    kw, N_range = CASES["rkf"]
    x, v = sr.LAW_POINTS[:, :2], sr.LAW_POINTS[:, 2:]
    a = bg.stochastic_distribution(art, p, x, v, 300, BINS, N_range, **kw)
    b = bg.stochastic_distribution(art, p, x, v, 300, BINS, N_range, **kw)
    c = bg.stochastic_distribution(art, p, x, v, 300, BINS, N_range, **dict(kw, seed=4))
    assert _same(a, b) and np.array_equal(a.edges, b.edges) and not np.array_equal(a.hist, c.hist)
    assert np.array_equal(a.N_classical, c.N_classical) and np.all(c.counts.sum(axis=1) == 300)


def test_in_law_against_independent_random_numbers(bg, hyper):
    """The LAW case (adaptive rkf, R = 2^14, seed 0) against the numpy restatement driven by numpy's own generator: neighbouring bins
    merged until each holds at least 40 pooled counts, the two-sample chi-squared of every point at most dof + 5 sqrt(2 dof).  The host
    twin against the same restatement gives chi2 / dof = 38.3 / 33, 20.4 / 28 and 61.9 / 38 with these 64 bins over N_classical - 4 ..
    N_classical + 8 (tests/test_background_distribution.py asserts it)."""
    art, p = hyper
    _spec, _art, model, _p = sr.hyperbolic_case()
    R = sr.LAW_R
    kw = dict(noise_scale=sr.LAW_SCALE, dN_max=sr.LAW_DN_MAX, max_err=1e-8, solver="rkf")
    got = bg.stochastic_distribution(art, p, sr.LAW_POINTS[:, :2], sr.LAW_POINTS[:, 2:], R, 64, (-4.0, 8.0), centre="classical", seed=0, **kw)
    want = sr.restatement_of(model, art, p).run(sr.LAW_POINTS, R, rng=np.random.default_rng(20240229), **kw)
    assert np.all(want.status == sr.ENDED) and np.all(got.n_ended == R)
    for b in range(3):
        row, _counts = dr.bin_samples(want.N.reshape(3, R)[b], want.status.reshape(3, R)[b], got.edges[b, 0], got.edges[b, -1], 64)
        mine = np.concatenate([[got.below[b]], got.hist[b], [got.above[b]]])
        chi2, dof = dr.chi2_two_samples(mine, row, least=40)
        print(f"point {b}: chi2 {chi2:.1f} with {dof} degrees of freedom (bound {dof + 5.0 * math.sqrt(2.0 * dof):.1f}); outside {mine[0]} + {mine[-1]}")
        assert dof >= 10 and chi2 <= dof + 5.0 * math.sqrt(2.0 * dof)


def test_map_is_the_batch_call_on_the_grid(bg, hyper):
    """8 x 8 grid, R = 16, centred on the classical e-fold count; the grid's first row lies at phi = 0, where the model is not finite:
    the classical run does not end there, and the row is all zero with NaN edges."""
    art, p = hyper
    ss = [[0.0, 8.0], [-1.0, 1.0]]
    kw = dict(seed=8, noise_scale=sr.LAW_SCALE, dN_max=0.125, max_steps=4000)
    got = bg.stochastic_distribution_map(art, p, ss, 8, 8, 16, 12, (-3.0, 3.0), derivatives_init=(-0.8, 0.0), **kw)
    x0, x1 = bg.grid_points(ss, 8, 8)
    x = np.stack([np.repeat(x0, 8), np.tile(x1, 8)], axis=1)
    want = bg.stochastic_distribution(art, p, x, np.tile([-0.8, 0.0], (64, 1)), 16, 12, (-3.0, 3.0), centre="classical", **kw)
    assert got.hist.shape == (8, 8, 12) and got.edges.shape == (8, 8, 13) and got.counts.shape == (8, 8, 6) and got.N_classical.shape == (8, 8)
    for f in (*INTEGERS, "edges", "N_classical"):
        assert np.array_equal(getattr(got, f).reshape(getattr(want, f).shape), getattr(want, f), equal_nan=True), f
    ran = np.isfinite(got.N_classical)
    print(f"map: {ran.sum()} of 64 points have a classical end; ended {got.n_ended[ran].min()} .. {got.n_ended[ran].max()} of 16")
    assert 8 <= ran.sum() < 64 and np.all(got.counts[ran].sum(axis=-1) == 16) and np.all(got.counts[~ran] == 0) and np.all(got.hist[~ran] == 0)
    assert np.all(np.isnan(got.edges[~ran])) and np.all(np.isfinite(got.edges[ran]))


def test_distribution_object_of_another_layout_is_refused(bg):
    """An object built with -DINFLX_PD_ABI_VERSION=2 is refused with INFLX_ERR_VERSION and the "does not belong" message, a missing one
    is INFLX_ERR_SYMBOL with the way to build it; the artefact's own build then replaces the refused file and works on the same handle,
    and stochastic_efolds on that handle gives the same bits before and after.  The C function's own argument checks come before the
    device."""
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    import background_reference as br

    # (an artefact of its own: no other handle of this process has had its distribution object loaded from the same path)
    art, p = br.wall_artifact()
    init, dt = np.array([[1.0, 0.0, 0.0, 0.0]]), 5e-2
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".distribution"
    headers = {stale + ".model.h": header_text, stale + ".eom.h": art.eom_header_text(), stale + ".noise.h": art.noise_header_text()}
    # (init, R, streams, seed, first, L, noise_scale, dN_max, max_steps, method, max_err, dt, bins, ranges)
    args = (init, 70, None, 1, 0, 64, 1.0, 1.0 / 32.0, 40, _native.EOM_RK4, 1e-8, dt, 8, [[0.0, 2.0]])
    efolds = (init, 70, None, 1, 1.0, 1.0 / 32.0, math.nan, 40, _native.EOM_RK4, 1e-8, dt)
    try:
        if os.path.exists(stale):
            os.remove(stale)
        art.ensure_stochastic()
        lib = _native.InflatoxDevLib(art.shared_object_path)
        before = lib.stochastic_efolds(p, *efolds, want_samples=True)
        with pytest.raises(SystemError, match=r"ensure_distribution\(\)") as err:
            lib.stochastic_distribution(p, *args)
        assert ".distribution exists" in str(err.value)
        for path, text in headers.items():
            with open(path, "w") as fh:
                fh.write(text)
        hdr, eom_hdr, noise_hdr = headers
        cmd = [hipcc_path(), *options, "-DINFLX_PD_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_NOISE_HEADER="{noise_hdr}"', os.path.join(_CSRC, "inflx_distribution_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.stochastic_distribution(p, *args)
        assert "INFLX_PD_ABI 2, expected 1" in str(err.value)
        os.remove(stale)
        art.ensure_distribution()
        hist, counts = lib.stochastic_distribution(p, *args)
        rows, want = dr.bin_samples(before[1][0], before[1][6], 0.0, 2.0, 8)
        assert hist.shape == (1, 10) and counts.shape == (1, 6) and np.array_equal(hist[0], rows) and np.array_equal(counts[0], want) and counts.sum() == 70
        after = lib.stochastic_efolds(p, *efolds, want_samples=True)
        assert np.array_equal(before[0], after[0], equal_nan=True) and np.array_equal(before[1], after[1], equal_nan=True)
        for bad, words in (((init, 0) + args[2:], "realisations"), ((init, 1 << 32) + args[2:], "realisations"), (args[:4] + (2**32 - 69,) + args[5:], "first_realisation"),
                           (args[:5] + (96,) + args[6:], "lanes_per_point"), (args[:5] + ((1 << 20) + 64,) + args[6:], "lanes_per_point"),
                           (args[:6] + (-1.0,) + args[7:], "noise_scale"), (args[:7] + (0.0,) + args[8:], "dN_max"), (args[:12] + (0,) + args[13:], "bins"),
                           (args[:12] + ((1 << 20) + 1,) + args[13:], "bins"), (args[:13] + ([[0.0, math.inf]],), "range"), (args[:13] + ([[1.0, 1.0]],), "range")):  # fmt: skip
            with pytest.raises(Exception, match=words):
                lib.stochastic_distribution(p, *bad)
        lib.close()
    finally:
        for path in (stale, *headers):
            if os.path.exists(path):
                os.remove(path)
        art._companion_paths.pop("distribution", None)
