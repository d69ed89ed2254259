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
``profiles/background_sampled.json``.  ``--rows`` times nothing but the three ways to 256 rows of 2^17 hyperbolic trajectories (rkf,
substeps 4; best of three calls each, alternating, after a warm-up): ``solve_eom`` with ``EOM_HOST_SCATTER`` (the rows rearranged by
the calling thread: the path of every earlier version), the default ``solve_eom`` (transposed on the device, two contiguous
copies) and ``solve_eom_batch_device`` followed by ``torch.cuda.synchronize()`` (nothing copied); a child process under ``rocprofv3
--kernel-trace --stats`` makes one device-resident call, for the summed time of the ``inflx_bg_rows_transpose`` launches beside the
``inflx_bg_advance_*`` launches.  Writes ``profiles/background_rows.json``.  Run from the repository root on the GPU box.
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


def _rows_batch(log2_lanes, seed=0):
    spec, art = workloads.artifact_for("hyperbolic")
    (a0, b0), (a1, b1), vel = START["hyperbolic"]
    B = 1 << log2_lanes
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(a0, b0, B), rng.uniform(a1, b1, B)], axis=1)
    v = rng.uniform(-vel, vel, (B, 2))
    return spec, art, x, v


def rows_workload(log2_lanes=17, rows=256, substeps=4):
    """what the --rows mode runs under the profiler: a warm-up on 256 lanes, then one device-resident call"""
    import torch

    spec, art, x, v = _rows_batch(log2_lanes)
    background.solve_eom_batch_device(art, spec.args, 4, x[:256], v[:256], substeps=substeps)
    sol = background.solve_eom_batch_device(art, spec.args, rows, x, v, substeps=substeps)
    torch.cuda.synchronize()
    print(json.dumps({"rows_workload_last_row_sum": int(np.minimum(sol.last_row, rows - 1).sum())}), flush=True)


def _kernel_trace(log2_lanes):
    """{kernel: [calls, total ns]} of the inflx_bg_* kernels of one device-resident call, from a child process under rocprofv3"""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile

    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="background_rows_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--rows-workload",
               "--max-log2-lanes", str(log2_lanes)]  # fmt: skip
        proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if proc.returncode != 0:
            return {"error": f"rocprofv3 exit status {proc.returncode}", "stderr": proc.stderr[-1000:]}
        kernels = {}
        for path in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    name = row["Name"].removesuffix(".kd")
                    if name.startswith("inflx_bg_"):
                        calls, total = kernels.get(name, (0, 0))
                        kernels[name] = (calls + int(row["Calls"]), total + int(row["TotalDurationNs"]))
        if not kernels:
            return {"error": "no inflx_bg_* kernel in the trace", "stdout": proc.stdout[-1000:]}
        return {k: list(v) for k, v in sorted(kernels.items())}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def rows_mode(log2_lanes=17, rows=256, substeps=4, repeats=3):
    trace = _kernel_trace(log2_lanes)  # first: this process has not opened the GPU yet
    import torch

    from inflatox_amd import _native

    spec, art, x, v = _rows_batch(log2_lanes)
    init = np.concatenate([x, v], axis=1)
    lib = background._dylib(art)
    call = (spec.args, init, rows, substeps, _native.EOM_RKF, 1e-6, 0.0)
    lib.solve_eom(spec.args, init[:256], 4, substeps, _native.EOM_RKF, 1e-6, 0.0, 0)  # build / load / warm up
    lib.solve_eom(spec.args, init[:256], 4, substeps, _native.EOM_RKF, 1e-6, 0.0, _native.EOM_HOST_SCATTER)
    background.solve_eom_batch_device(art, spec.args, 4, x[:256], v[:256], substeps=substeps)
    torch.cuda.synchronize()
    t_scatter, t_default, t_device = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        a = lib.solve_eom(*call, _native.EOM_HOST_SCATTER)
        t_scatter.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        b = lib.solve_eom(*call, 0)
        t_default.append(time.perf_counter() - t0)
        same = all(np.array_equal(u, w, equal_nan=True) for u, w in zip(a, b))
        steps = int(np.sum(np.minimum(b[4], rows - 1))) * substeps
        del a
        t0 = time.perf_counter()
        dev = background.solve_eom_batch_device(art, spec.args, rows, x, v, substeps=substeps)
        torch.cuda.synchronize()
        t_device.append(time.perf_counter() - t0)
        same = same and bool(torch.equal(torch.nan_to_num(dev.t[:4096].cpu()), torch.nan_to_num(torch.from_numpy(b[1][:4096]))))
        del b, dev
    rec = dict(model="hyperbolic", code_object=art._build[2], B=1 << log2_lanes, rows=rows, substeps=substeps, solver="rkf", max_err=1e-6, repeats=repeats,
               host_scatter_s=t_scatter, default_host_s=t_default, device_resident_s=t_device, best_s=dict(host_scatter=min(t_scatter),
               default_host=min(t_default), device_resident=min(t_device)), accepted_lane_steps=steps, results_equal=same,
               result_bytes=(1 << log2_lanes) * rows * 56, kernel_trace_ns=trace,
               note="wall time of whole calls, best of `repeats` after a warm-up, the three calls alternating in one process; kernel_trace_ns: "
                    "[launches, summed ns] per kernel of ONE device-resident call (and its 256-lane warm-up) in a child process under rocprofv3",
               command="python scripts/background_probe.py --rows")  # fmt: skip
    print(json.dumps(rec), flush=True)
    with open(os.path.join(ROOT, "profiles", "background_rows.json"), "w") as fh:
        json.dump(rec, fh, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", action="store_true", help="time the forced host scatter, the default host call and solve_eom_batch_device (B = 2^17, 256 rows), nothing else")
    ap.add_argument("--rows-workload", action="store_true", help="one device-resident call (what --rows runs under rocprofv3)")
    ap.add_argument("--sampled", action="store_true", help="time solve_eom_sampled (B = 2^17, S = 256) beside solve_eom_batch returning 256 rows, nothing else")
    ap.add_argument("--horizon-exit", action="store_true", help="time horizon_exit_map beside efolds_map at 1024^2 on hyperbolic, nothing else")
    ap.add_argument("--quick", action="store_true", help="B = 2^14 only (for a profiler run)")
    ap.add_argument("--max-log2-lanes", type=int, default=20)
    args = ap.parse_args()
    if args.rows_workload:
        rows_workload(min(args.max_log2_lanes, 17))
        return
    if args.rows:
        rows_mode(min(args.max_log2_lanes, 17))
        return
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
