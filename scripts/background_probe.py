"""Throughput of the background-trajectory kernels (inflatox_amd.background) -- measurement tool.

Times ``solve_eom_batch`` (rkf, 256 rows, substeps 4) for B in {2^14, 2^17} and the same trajectories in the final-only mode (no
rows stored or copied: kernels plus one carry copy) for B in {2^14, 2^17, 2^20}, on hyperbolic and EGNO, and ``efolds_map`` at
1024^2 on hyperbolic; reports accepted lane-steps per second (wall time of the call) and writes
``profiles/background_<model>.json`` stamped with the core object's content tag.  The kernel time comes from a run of its own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/background_probe.py --quick

(kernels ``inflx_bg_advance_*``).  ``--horizon-exit`` times nothing but ``horizon_exit_map`` beside ``efolds_map`` on the same
1024^2 hyperbolic grid (best of three calls each, after a warm-up) and writes ``profiles/background_horizon_exit.json``.
``--sampled`` times nothing but ``solve_eom_sampled`` at B = 2^17 with S = 256 e-fold counts beside ``solve_eom_batch`` returning 256
rows of the same trajectories (three calls each, alternating, after a warm-up of both) and writes
``profiles/background_sampled.json``.  Run from the repository root on the GPU box.
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import workloads  # noqa: E402
from inflatox_amd import background  # noqa: E402

START = {"hyperbolic": ((2.0, 5.0), (-1.0, 1.0), 0.2), "egno": ((0.6, 0.9), (0.2, 0.5), 1.0)}


def batch(name, B, rows=256, substeps=4, seed=0):
    spec, art = workloads.artifact_for(name)
    (a0, b0), (a1, b1), vel = START[name]
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(a0, b0, B), rng.uniform(a1, b1, B)], axis=1)
    v = rng.uniform(-vel, vel, (B, 2))
    background.solve_eom_batch(art, spec.args, 4, x[:256], v[:256], solver="rkf", substeps=substeps)  # build / load / warm up
    rec = {}
    if B <= 1 << 17:  # (the (B, rows, 6) result of 2^20 lanes is 12.9 GB of host memory: that size is timed final-only)
        t0 = time.perf_counter()
        sol = background.solve_eom_batch(art, spec.args, rows, x, v, solver="rkf", substeps=substeps)
        dt = time.perf_counter() - t0
        steps = int(np.sum(np.minimum(sol.last_row, rows - 1))) * substeps
        rec = dict(seconds=dt, accepted_lane_steps=steps, lane_steps_per_s=steps / dt)
    # the same trajectories in the final-only mode: no rows stored or copied, so the call is the kernels plus one carry copy
    from inflatox_amd import _native

    init = np.concatenate([x, v], axis=1)
    dylib = background._dylib(art)
    t0 = time.perf_counter()
    _, _, _, fstatus, flast = dylib.solve_eom(spec.args, init, rows, substeps, _native.EOM_RKF, 1e-6, 0.0, _native.EOM_FINAL_ONLY)
    dt_final = time.perf_counter() - t0
    steps_final = int(np.sum(np.minimum(flast, rows - 1))) * substeps
    return art, dict(B=B, rows=rows, substeps=substeps, **rec, final_only_seconds=dt_final, final_only_accepted_lane_steps=steps_final,
                     final_only_lane_steps_per_s=steps_final / dt_final,
                     status_counts={int(k): int(c) for k, c in zip(*np.unique(fstatus, return_counts=True))})  # fmt: skip


def horizon_exit(n=1024, n_star=1.0, repeats=3):
    spec, art = workloads.artifact_for("hyperbolic")
    ss = [[1.0, 5.0], [-1.0, 1.0]]
    background.horizon_exit_map(art, spec.args, ss, 32, 32, N_star=n_star)  # build / load / warm up

    def best(fn):
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = fn()
            times.append(time.perf_counter() - t0)
        return min(times), out

    t_map, n_end = best(lambda: background.efolds_map(art, spec.args, ss, n, n))
    t_exit, (state, n_end2, status) = best(lambda: background.horizon_exit_map(art, spec.args, ss, n, n, N_star=n_star, return_status=True))
    assert np.array_equal(n_end, n_end2, equal_nan=True)
    rec = dict(model="hyperbolic", code_object=art._build[2], grid=[n, n], start_stop=ss, N_star=n_star, repeats=repeats,
               efolds_map_s=t_map, horizon_exit_map_s=t_exit, ratio=t_exit / t_map, ended=int(np.isfinite(n_end).sum()),
               exit_states=int(np.isfinite(state).all(axis=2).sum()),
               status_counts={int(k): int(c) for k, c in zip(*np.unique(status, return_counts=True))},
               command="python scripts/background_probe.py --horizon-exit")  # fmt: skip
    print(json.dumps(rec), flush=True)
    with open(os.path.join(ROOT, "profiles", "background_horizon_exit.json"), "w") as fh:
        json.dump(rec, fh, indent=1)


def sampled(log2_lanes=17, n_samples=256, rows=256, substeps=4, repeats=3, seed=0):
    spec, art = workloads.artifact_for("hyperbolic")
    (a0, b0), (a1, b1), vel = START["hyperbolic"]
    B = 1 << log2_lanes
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(a0, b0, B), rng.uniform(a1, b1, B)], axis=1)
    v = rng.uniform(-vel, vel, (B, 2))
    samples = np.linspace(0.0, 4.0, n_samples)
    kw = dict(max_err=1e-6, solver="rkf")
    background.solve_eom_sampled(art, spec.args, samples, x[:256], v[:256], **kw)  # build / load / warm up
    background.solve_eom_batch(art, spec.args, 4, x[:256], v[:256], substeps=substeps, **kw)
    t_sampled, t_rows = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        sol = background.solve_eom_sampled(art, spec.args, samples, x, v, **kw)
        t_sampled.append(time.perf_counter() - t0)
        stored = int(sol.n_stored.sum())
        status = {int(k): int(c) for k, c in zip(*np.unique(sol.status, return_counts=True))}
        del sol
        t0 = time.perf_counter()
        ref = background.solve_eom_batch(art, spec.args, rows, x, v, substeps=substeps, **kw)
        t_rows.append(time.perf_counter() - t0)
        row_steps = int(np.sum(np.minimum(ref.last_row, rows - 1))) * substeps
        del ref
    rec = dict(model="hyperbolic", code_object=art._build[2], B=B, samples=n_samples, sample_range=[0.0, 4.0], at="N", stop_at_end=True, solver="rkf",
               max_err=1e-6, repeats=repeats, solve_eom_sampled_s=t_sampled, samples_stored=stored, sampled_status_counts=status,
               solve_eom_batch_rows=rows, solve_eom_batch_substeps=substeps, solve_eom_batch_s=t_rows, solve_eom_batch_accepted_lane_steps=row_steps,
               note="wall time of whole calls; the two calls return different things (states at shared e-fold counts against every fourth accepted step), so this is a comparison of two ways to get 256 states per trajectory, not of the same work",
               command="python scripts/background_probe.py --sampled")  # fmt: skip
    print(json.dumps(rec), flush=True)
    with open(os.path.join(ROOT, "profiles", "background_sampled.json"), "w") as fh:
        json.dump(rec, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sampled", action="store_true", help="time solve_eom_sampled (B = 2^17, S = 256) beside solve_eom_batch returning 256 rows, nothing else")
    ap.add_argument("--horizon-exit", action="store_true", help="time horizon_exit_map beside efolds_map at 1024^2 on hyperbolic, nothing else")
    ap.add_argument("--quick", action="store_true", help="B = 2^14 only (for a profiler run)")
    ap.add_argument("--max-log2-lanes", type=int, default=20)
    args = ap.parse_args()
    if args.horizon_exit:
        horizon_exit()
        return
    if args.sampled:
        sampled()
        return
    sizes = [14] if args.quick else [k for k in (14, 17, 20) if k <= args.max_log2_lanes]
    for name in ("hyperbolic", "egno"):
        rec = {"model": name, "runs": []}
        art = None
        for k in sizes:
            art, r = batch(name, 1 << k)
            rec["runs"].append(r)
            print(json.dumps({"model": name, **r}), flush=True)
        rec["code_object"] = art._build[2]
        if name == "hyperbolic" and not args.quick:
            spec, _ = workloads.artifact_for(name)
            t0 = time.perf_counter()
            n_end, status = background.efolds_map(art, spec.args, [[1.0, 5.0], [-1.0, 1.0]], 1024, 1024, return_status=True)
            rec["efolds_map_1024x1024_s"] = time.perf_counter() - t0
            rec["efolds_map_finite"] = int(np.isfinite(n_end).sum())
            print(json.dumps({"efolds_map_1024x1024_s": rec["efolds_map_1024x1024_s"], "finite": rec["efolds_map_finite"]}), flush=True)
        if not args.quick:
            with open(os.path.join(ROOT, "profiles", f"background_{name}.json"), "w") as fh:
                json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
