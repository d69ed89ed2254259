"""Lane-steps per second of the reheating kernels beside inflation_end -- measurement tool (inflatox_amd.reheating).

B = 2^16 hyperbolic lanes (seeded draws of the fields in [1.5, 4] x [-1, 1] with velocities in [-0.2, 0.2]) at a fixed dt = 0.01 with
rkf, so that a lane's accepted steps are its stopping time over dt: ``inflation_end`` over the lanes, then ``reheating`` with
Gamma = 0.2 and omega_r = 0.99 from the located end states of the same lanes.  Lane-steps per second is the sum of the lanes' accepted
steps over the wall time of the call (``time.perf_counter`` around the whole call, which ends in a stream synchronise); a launch
lasts as long as its slowest lane, so idle lanes lower the figure.  After a warm-up of each the calls alternate, ``--repeats`` times
(at least five).  Nothing is asserted on the figures.  Writes medians, extremes and the SHA-256 of the two code objects under
``"probe"`` into ``profiles/reheating.json`` (or ``--out``), keeping what the file holds otherwise.

``--registers`` needs no GPU: it reads vgpr + agpr, spilled registers and the private-segment (scratch) bytes of ``inflx_rh_*`` from the
metadata notes of the cross-compiled objects of every prebuilt model (``llvm-readelf --notes``) into the same file.  Run from the
repository root.
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
from inflatox_amd import background, reheating  # noqa: E402
from inflatox_amd.compiler import hipcc_path  # noqa: E402

PROFILE = os.path.join(ROOT, "profiles", "reheating.json")
MODELS = ("hyperbolic", "doc", "angular", "egno", "d5")
DT, GAMMA, OMEGA_R = 0.01, 0.2, 0.99


def sha256(path):
    with open(path, "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def summary(times, lane_steps):
    med = statistics.median(times)
    return {"median_s": round(med, 4), "min_s": round(min(times), 4), "max_s": round(max(times), 4), "calls": len(times), "lane_steps": int(lane_steps),
            "lane_steps_per_s": round(lane_steps / med)}  # fmt: skip


def measure(repeats, B):
    spec, art = workloads.artifact_for("hyperbolic")
    p = np.asarray(spec.args, dtype=np.float64)
    rng = np.random.default_rng(0)
    x = np.stack([rng.uniform(1.5, 4.0, B), rng.uniform(-1, 1, B)], axis=1)
    v = rng.uniform(-0.2, 0.2, (B, 2))
    to_end = lambda: background.inflation_end(art, p, x, v, solver="rkf", dt=DT)  # noqa: E731
    end = to_end()
    assert np.all(end.status == background.ENDED)
    decay = lambda: reheating.reheating(art, p, GAMMA, end.state[:, :2], end.state[:, 2:4], omega_r=OMEGA_R, solver="rkf", dt=DT)  # noqa: E731
    reh = decay()
    assert np.all(reh.status == reheating.REHEATED)
    steps = {"inflation_end": np.ceil(end.t_end / DT - 1e-9).sum(), "reheating": np.ceil(reh.t_reh / DT - 1e-9).sum()}
    times = {"inflation_end": [], "reheating": []}
    for i in range(repeats):
        print(f"repeat {i} ...", flush=True)
        times["inflation_end"].append(timed(to_end)[0])
        times["reheating"].append(timed(decay)[0])
    rec = {"case": f"{B} hyperbolic lanes, rkf at a fixed dt = {DT}; inflation_end, then reheating with Gamma = {GAMMA}, omega_r = {OMEGA_R} from the located end states",
           "clock": "time.perf_counter around whole calls, each ending in a stream synchronise; calls alternate after a warm-up of each",
           "steps_per_lane": {"inflation_end": [float(np.ceil(end.t_end / DT - 1e-9).min()), float(np.ceil(end.t_end / DT - 1e-9).max())],
                              "reheating": [float(np.ceil(reh.t_reh / DT - 1e-9).min()), float(np.ceil(reh.t_reh / DT - 1e-9).max())]},
           **{name: summary(t, steps[name]) for name, t in times.items()}}  # fmt: skip
    rec["ratio_of_lane_steps_per_s"] = round(rec["reheating"]["lane_steps_per_s"] / rec["inflation_end"]["lane_steps_per_s"], 3)
    rec["code_objects_sha256"] = {"crossing": sha256(art.ensure_crossing()), "reheating": sha256(art.ensure_reheating())}
    return rec


def registers():
    tool = os.path.join(os.path.dirname(os.path.realpath(hipcc_path())), "..", "lib", "llvm", "bin", "llvm-readelf")
    out = {"what": "llvm-readelf --notes of the cross-compiled <artefact>.reheating objects: [vgpr_count + agpr_count, spilled vgprs, private-segment (scratch) "
                   "bytes per lane] of every reheating kernel"}  # fmt: skip
    for name in MODELS:
        _spec, art = workloads.artifact_for(name)
        rec = {}
        notes = subprocess.run([tool, "--notes", art.ensure_reheating()], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count:")[1:]:
            kernel = re.search(r"\.name:\s+(\S+)", block).group(1)
            if kernel.startswith("inflx_rh_"):
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
        result["probe"] = measure(args.repeats, args.lanes)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(result.get("registers" if args.registers else "probe"), indent=1))
