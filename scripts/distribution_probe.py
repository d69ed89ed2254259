"""First-passage histograms against the stochastic e-folds at equal work -- measurement tool (inflatox_amd.background).

Times ``stochastic_distribution`` beside ``stochastic_efolds`` in one process: three hyperbolic points 8 to 12 e-folds before the end of
inflation, noise_scale 0.4, dN_max 0.125, adaptive rkf (the comparison-in-law case of the tests), R = 2^18 realisations per point.
Every call ends in a stream synchronise inside the library; the clock is ``time.perf_counter`` around the call.  After a warm-up of
each, the calls alternate, ``--repeats`` times (at least five): ``stochastic_efolds``, then ``stochastic_distribution`` at each of the
``lanes_per_point`` of ``--lanes`` (0: the default rule, which gives 2^18 here).  Then one ``stochastic_distribution`` call at R = 2^24,
which ``stochastic_efolds`` cannot run at all (R <= 2^20), at the default lanes (349504 per point) and at 1024 lanes per point.  The histograms of all lane
counts must be identical, and equal to the binned samples of a ``stochastic_efolds`` call at R = 2^16.  Writes medians, extremes and the
SHA-256 of the two code objects into ``profiles/background_distribution.json`` (or ``--out``), keeping what the file holds otherwise.

``--registers`` needs no GPU: it reads vgpr + agpr, spilled registers and scratch bytes of ``inflx_pd_advance_*`` and
``inflx_st_advance_*`` from the cross-compiled objects of every prebuilt model (``llvm-readelf --notes``) into the same file.
Run from the repository root.
"""

import argparse
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import workloads  # noqa: E402
from inflatox_amd import background  # noqa: E402
from inflatox_amd.compiler import hipcc_path  # noqa: E402

POINTS = np.array([[7.3, 0.4, -0.8, 1e-4], [6.9, -0.7, -0.8, -2e-4], [7.6, 0.1, -0.8, 5e-5]])
OPTIONS = dict(noise_scale=0.4, dN_max=0.125, max_err=1e-8, solver="rkf", seed=0)
BINS, RANGE = 256, (4.0, 24.0)
PROFILE = os.path.join(ROOT, "profiles", "background_distribution.json")
MODELS = ("hyperbolic", "doc", "angular", "egno", "d5")


def sha256(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def summary(times):
    return {"median_s": round(statistics.median(times), 4), "min_s": round(min(times), 4), "max_s": round(max(times), 4), "calls": len(times)}


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def measure(repeats, lanes):
    spec, art = workloads.artifact_for("hyperbolic")
    p, x, v = np.asarray(spec.args, dtype=np.float64), POINTS[:, :2], POINTS[:, 2:]
    R = 1 << 18
    efolds = lambda r=R, samples=False: background.stochastic_efolds(art, p, x, v, r, return_samples=samples, **OPTIONS)  # noqa: E731
    dist = lambda L, r=R: background.stochastic_distribution(art, p, x, v, r, BINS, RANGE, lanes_per_point=L or None, **OPTIONS)  # noqa: E731
    # what is timed computes the same thing: the binned samples at R = 2^16, every lane count
    se = efolds(1 << 16, True)
    k = np.floor((se.N - RANGE[0]) * (BINS / (RANGE[1] - RANGE[0])))
    inside = (se.status == background.ENDED) & (k >= 0) & (k < BINS)
    want = np.stack([np.bincount(row[m].astype(np.int64), minlength=BINS) for row, m in zip(k, inside)])
    for L in lanes:
        got = dist(L, 1 << 16)
        assert np.array_equal(got.hist, want) and np.array_equal(got.below + got.above, (se.status == background.ENDED).sum(axis=1) - inside.sum(axis=1)), L
    print("the histograms of every lane count are the binned samples at R = 2^16", flush=True)
    efolds(), [dist(L) for L in lanes]  # warm-up of every timed shape
    times = {"stochastic_efolds": [], **{f"stochastic_distribution_L{L or 'default'}": [] for L in lanes}}
    first = None
    for i in range(repeats):
        print(f"repeat {i} ...", flush=True)
        times["stochastic_efolds"].append(timed(efolds)[0])
        for L in lanes:
            dt, d = timed(lambda: dist(L))
            times[f"stochastic_distribution_L{L or 'default'}"].append(dt)
            first = d if first is None else first
            assert np.array_equal(d.hist, first.hist) and np.array_equal(d.counts, first.counts)
    rec = {"case": "three hyperbolic points 8 to 12 e-folds before the end, noise_scale 0.4, dN_max 0.125, adaptive rkf, max_err 1e-8; 256 bins over N in [4, 24)",
           "clock": "time.perf_counter around whole calls, each ending in a stream synchronise; calls alternate after a warm-up of each",
           "R_2^18": {name: summary(t) for name, t in times.items()}, "R_2^18_n_ended": first.n_ended.tolist()}  # fmt: skip
    big = {}
    for L in (0, 1024):
        print(f"R = 2^24 on {L or 'the default'} lanes per point ...", flush=True)
        dt, d = timed(lambda: dist(L, 1 << 24))
        big[f"stochastic_distribution_L{L or 'default'}"] = {"seconds": round(dt, 3), "n_ended": d.n_ended.tolist(), "above": d.above.tolist(),
                                                            "survival_at_N_classical_plus_6": [float(background.distribution_survival(d)[b][np.searchsorted(d.edges[b], d.N_classical[b] + 6.0)]) for b in range(3)]}  # fmt: skip
        big.setdefault("hist_sha256", hashlib.sha256(d.hist.tobytes()).hexdigest())
        assert big["hist_sha256"] == hashlib.sha256(d.hist.tobytes()).hexdigest()
    rec["R_2^24"] = big
    rec["code_objects_sha256"] = {"stochastic": sha256(art.ensure_stochastic()), "distribution": sha256(art.ensure_distribution())}
    return rec


def registers():
    tool = os.path.join(os.path.dirname(os.path.realpath(hipcc_path())), "..", "lib", "llvm", "bin", "llvm-readelf")
    out = {"what": "llvm-readelf --notes of the cross-compiled <artefact>.distribution and <artefact>.stochastic objects: [vgpr_count + agpr_count, "
                   "spilled vgprs, scratch bytes per lane] of the rk4 / rkf advance kernels"}  # fmt: skip
    for name in MODELS:
        _spec, art = workloads.artifact_for(name)
        rec = {}
        for obj, prefix in ((art.ensure_distribution(), "inflx_pd_advance_"), (art.ensure_stochastic(), "inflx_st_advance_")):
            notes = subprocess.run([tool, "--notes", obj], capture_output=True, text=True, check=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                kernel = re.search(r"\.name:\s+(\S+)", block).group(1)
                if kernel.startswith(prefix):
                    field = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))  # noqa: E731
                    rec[kernel] = [field("vgpr_count") + int(block.split()[0]), field("vgpr_spill_count"), field("private_segment_fixed_size")]
        out[name] = rec
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lanes", type=int, nargs="*", default=[0, 1024, 1 << 14, 1 << 16, 1 << 18])
    ap.add_argument("--registers", action="store_true")
    ap.add_argument("--out", default=PROFILE)
    args = ap.parse_args()
    result = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.registers:
        result["registers"] = registers()
    else:
        assert args.repeats >= 5
        result["timing"] = measure(args.repeats, args.lanes)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result.get("registers" if args.registers else "timing"), indent=1))
