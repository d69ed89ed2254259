"""Horizon crossings beside the sampled trajectories at equal work -- measurement tool (inflatox_amd.background).

Times ``horizon_crossings`` beside ``solve_eom_sampled`` in one process: B = 2^16 lanes that all start from one hyperbolic point at rest, 57
e-folds before the end of inflation, adaptive rkf, S = 8 wavenumbers relative to ln H_0.  All lanes being the same trajectory, the
e-fold counts that ``horizon_crossings`` locates are one list, and ``solve_eom_sampled`` at that list takes the same accepted steps and
emits from the same steps: the two calls differ by the event alone.  Every call ends in a stream synchronise inside the library; the
clock is ``time.perf_counter`` around the call.  After a warm-up of each the calls alternate, ``--repeats`` times (at least five).
Writes medians, extremes and the SHA-256 of the two code objects into ``profiles/background_crossing.json`` (or ``--out``), keeping what
the file holds otherwise.

``--registers`` needs no GPU: it reads vgpr + agpr, spilled registers and scratch bytes of ``inflx_hx_advance_*`` and ``inflx_hx_end_*``
beside ``inflx_bg_advance_*_sampled`` from the cross-compiled objects of every prebuilt model (``llvm-readelf --notes``) into the same
file.  Run from the repository root.
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

POINT = np.array([16.0, 0.4, 0.0, 0.0])
LN_K = np.array([0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 48.0])
PROFILE = os.path.join(ROOT, "profiles", "background_crossing.json")
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


def measure(repeats, B):
    spec, art = workloads.artifact_for("hyperbolic")
    p = np.asarray(spec.args, dtype=np.float64)
    x, v = np.tile(POINT[:2], (B, 1)), np.tile(POINT[2:], (B, 1))
    one = background.solve_eom_batch(art, p, 1, x[:1], v[:1])
    offset = float(np.log(one.states[0, 0, 4]))
    crossings = lambda: background.horizon_crossings(art, p, LN_K, x, v, offset=offset)  # noqa: E731
    cr = crossings()
    assert np.all(cr.status == background.TARGET) and np.all(cr.N == cr.N[0])
    n_located = np.array(cr.N[0])
    sampled = lambda: background.solve_eom_sampled(art, p, n_located, x, v)  # noqa: E731
    sm = sampled()
    assert np.all(sm.status == background.TARGET)
    worst = float(np.max(np.abs(sm.states - cr.states) / np.maximum(np.abs(cr.states), 1e-3)))
    times = {"horizon_crossings": [], "solve_eom_sampled": []}
    for i in range(repeats):
        print(f"repeat {i} ...", flush=True)
        times["solve_eom_sampled"].append(timed(sampled)[0])
        times["horizon_crossings"].append(timed(crossings)[0])
    rec = {"case": f"{B} lanes from one hyperbolic point, adaptive rkf, max_err 1e-8, 8 wavenumbers; solve_eom_sampled at the e-fold counts the crossings located",
           "clock": "time.perf_counter around whole calls, each ending in a stream synchronise; calls alternate after a warm-up of each",
           "located_N": n_located.tolist(), "states_max_relative_difference": worst, **{name: summary(t) for name, t in times.items()}}  # fmt: skip
    rec["ratio_of_medians"] = round(rec["horizon_crossings"]["median_s"] / rec["solve_eom_sampled"]["median_s"], 3)
    rec["code_objects_sha256"] = {"background": sha256(art.ensure_background()), "crossing": sha256(art.ensure_crossing())}
    return rec


def registers():
    tool = os.path.join(os.path.dirname(os.path.realpath(hipcc_path())), "..", "lib", "llvm", "bin", "llvm-readelf")
    out = {"what": "llvm-readelf --notes of the cross-compiled <artefact>.crossing and <artefact>.background objects: [vgpr_count + agpr_count, "
                   "spilled vgprs, scratch bytes per lane] of the crossing kernels and of the sampled kernels"}  # fmt: skip
    for name in MODELS:
        _spec, art = workloads.artifact_for(name)
        rec = {}
        for obj, pattern in ((art.ensure_crossing(), r"inflx_hx_(advance|end)_"), (art.ensure_background(), r"inflx_bg_advance_\w+_sampled")):
            notes = subprocess.run([tool, "--notes", obj], capture_output=True, text=True, check=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                kernel = re.search(r"\.name:\s+(\S+)", block).group(1)
                if re.match(pattern, kernel):
                    field = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))  # noqa: E731
                    rec[kernel] = [field("vgpr_count") + int(block.split()[0]), field("vgpr_spill_count"), field("private_segment_fixed_size")]
        out[name] = rec
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=1 << 16)
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
