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
``inflx_bg_advance_*`` launches.  Writes ``profiles/background_rows.json``.  ``--kinematics`` measures nothing but
``background.kinematics``: its device path on 2^22 hyperbolic states read in place from (2^14, 256, 6) rows (ld = 6) -- the wall
time of whole calls, each ending in a stream synchronise, and the ``inflx_kin_states`` kernel alone from a child process under
``rocprofv3`` -- beside a device-to-device copy that moves as many bytes as the kernel reads plus writes, timed with device
events in the same process; and the worst ratio of |result - 40-digit truth| to the allowance of tests/kinematics_reference.py
over the zoo of tests/background_truth.py, for the host build and for the GPU.  Writes ``profiles/background_kinematics.json``.
``--masses`` does the same for ``background.masses`` on hyperbolic and on EGNO: the ``inflx_mass_states`` kernel beside
``inflx_kin_states`` on the same states and beside the copy, one trace of a child process per model, and the accuracy against
tests/masses_reference.py.  Writes ``profiles/background_masses.json``.
Run from the repository root on the GPU box.
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


def _rows_batch(log2_lanes, seed=0, name="hyperbolic"):
    spec, art = workloads.artifact_for(name)
    (a0, b0), (a1, b1), vel = START[name]
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


def _kernel_trace(log2_lanes, workload="--rows-workload", prefix="inflx_bg_", extra=(), each=()):
    """{kernel: [calls, total ns]} of the kernels named ``prefix``* of the child process ``workload`` under rocprofv3 (by default
    one device-resident call of the solver); ``extra``: further rocprofv3 options -- with ``--memory-copy-trace`` the memory copies
    are listed the same way, by direction; ``each``: kernels whose single dispatches are listed too (``dispatch_ns``)"""
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
        cmd = [prof, "--kernel-trace", *extra, "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), workload,
               "--max-log2-lanes", str(log2_lanes)]  # fmt: skip
        proc = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        if proc.returncode != 0:
            return {"error": f"rocprofv3 exit status {proc.returncode}", "stderr": proc.stderr[-1000:]}
        kernels = {}
        stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if extra:
            stats += glob.glob(os.path.join(out, "**", "*memory_copy_stats.csv"), recursive=True)
        for path in stats:
            with open(path, newline="") as fh:
                for row in csv.DictReader(fh):
                    if not {"Name", "Calls", "TotalDurationNs"} <= set(row):
                        continue
                    name = row["Name"].removesuffix(".kd")[:120]
                    if name.startswith(prefix):
                        calls, total = kernels.get(name, (0, 0))
                        kernels[name] = (calls + int(row["Calls"]), total + int(row["TotalDurationNs"]))
        if not kernels:
            return {"error": f"no {prefix}* kernel in the trace", "stdout": proc.stdout[-1000:]}
        found = {k: list(v) for k, v in sorted(kernels.items())}
        if each:
            # the single dispatches of the kernels named in `each`: {name: durations in ns, longest first}
            found["dispatch_ns"] = {}
            for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
                with open(path, newline="") as fh:
                    for row in csv.DictReader(fh):
                        if {"Kernel_Name", "Start_Timestamp", "End_Timestamp"} <= set(row) and row["Kernel_Name"].removesuffix(".kd") in each:
                            found["dispatch_ns"].setdefault(row["Kernel_Name"].removesuffix(".kd"), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
            for durations in found["dispatch_ns"].values():
                durations.sort(reverse=True)
        return found
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


KIN_LOG2_TRAJ, KIN_ROWS = 14, 256  # 2^14 trajectories x 256 rows = 2^22 states
COPY_KERNEL = "__amd_rocclr_copyBuffer"  # what the HIP runtime carries a device-to-device copy out with
KIN_SETS = 3  # input sets used in turn: 3 x 201 MB read and 201 MB written per call -- a line is long out of the 256 MiB Infinity Cache when its set comes round again


def _kinematics_rows(name="hyperbolic"):
    """(artefact, parameter row, KIN_SETS views (2^14, 256, 5) of (2^14, 256, 6) device rows): the first rows of 2^14 trajectories of
    the model (hyperbolic unless named), repeated along the row axis with a small shift per row and per set so that no two states
    are the same"""
    import torch

    spec, art, x, v = _rows_batch(KIN_LOG2_TRAJ, name=name)
    sol = background.solve_eom_batch_device(art, spec.args, 2, x, v)
    first = torch.cat([sol.states[:, :1], sol.N[:, :1, None]], dim=2)  # (B, 1, 6)
    sets = []
    for k in range(KIN_SETS):
        shift = 1.0 + 1e-3 * (k / KIN_SETS + torch.arange(KIN_ROWS, dtype=torch.float64, device=first.device))[None, :, None]
        sets.append((first * shift).contiguous()[:, :, :5])
    return spec, art, sets


def _copy_buffers(sets, planes=6):
    """(KIN_SETS sources, one destination) for the device-to-device copy that moves what one call moves: a kinematics call reads
    the lines of (n, 6) rows and writes six planes, 96 bytes per state; a copy of 48 bytes per state reads and writes as much.  With
    ``planes`` = 8, a masses call: 112 bytes per state, a copy of 56"""
    import torch

    n = sets[0].shape[0] * sets[0].shape[1]
    srcs = [torch.empty(n * (6 + planes) // 2, dtype=torch.float64, device=sets[0].device).normal_() for _ in range(KIN_SETS)]
    return srcs, torch.empty_like(srcs[0])


def kinematics_workload(rounds=4):
    """what the --kinematics mode runs under the profiler: a warm-up of both, then ``rounds`` x KIN_SETS device-resident calls and as
    many device-to-device copies of the same bytes, each over input sets used in turn"""
    import torch

    spec, art, sets = _kinematics_rows()
    srcs, dst = _copy_buffers(sets)
    for r in range(rounds + 1):
        for k in range(KIN_SETS):
            kin = background.kinematics(art, spec.args, sets[k])
        for k in range(KIN_SETS):
            dst.copy_(srcs[k])
        torch.cuda.synchronize()
    print(json.dumps({"kinematics_workload_omega_nansum": float(torch.nansum(kin.omega))}), flush=True)


def kinematics_accuracy():
    """worst |result - truth| / allowance per model and quantity, host build and GPU (tests/kinematics_reference.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import background_truth as bt
    import kinematics_reference as kr

    rec = {}
    for name in bt.GPU_MODELS:
        states, pars = kr.zoo_states(name)
        truth = kr.zoo_truth(name, 257)
        host = kr.KinematicsTwin(bt.host_artifact(name)).kinematics(pars, states)
        gpu = np.stack(background.kinematics(bt.device_artifact(name), pars, states))
        allow = kr.allowance(truth, states[:, 4])
        rec[name] = dict(host=kr.worst_ratios(host, truth, states[:, 4]), gpu=kr.worst_ratios(gpu, truth, states[:, 4]),
                         gpu_to_host=dict(zip(kr.NAMES, (float(r) for r in (np.abs(gpu - host) / allow).max(axis=1)))))  # fmt: skip
        print(json.dumps({name: rec[name]}), flush=True)
    worst = {side: max(max(rec[m][side].values()) for m in rec) for side in ("host", "gpu", "gpu_to_host")}
    return dict(states_per_model=257, allowance="tests/kinematics_reference.py allowance(): 1e-10 of the size of the terms a quantity is built from", worst=worst, models=rec)


def kinematics_mode(repeats=8):
    # first: this process has not opened the GPU yet.  Every kernel and every memory copy of the child, so that the copy is found
    # whether the runtime makes it a kernel of its own or a copy-engine transfer
    trace = _kernel_trace(KIN_LOG2_TRAJ, "--kinematics-workload", "", extra=("--memory-copy-trace",), each=("inflx_kin_states", COPY_KERNEL))
    import torch

    spec, art, sets = _kinematics_rows()
    n = sets[0].shape[0] * sets[0].shape[1]
    assert all(background._state_stride(tuple(y.shape), tuple(y.stride())) == 6 for y in sets)
    srcs, dst = _copy_buffers(sets)
    for k in range(KIN_SETS):
        kin = background.kinematics(art, spec.args, sets[k])  # build / load / warm up
        dst.copy_(srcs[k])
    torch.cuda.synchronize()
    moved = n * 6 * 8 + n * 6 * 8  # the lines of the (n, 6) rows read, the six planes written
    t_call, t_copy = [], []
    for _ in range(repeats):  # alternating, the input sets in turn
        for k in range(KIN_SETS):
            t0 = time.perf_counter()
            kin = background.kinematics(art, spec.args, sets[k])  # (returns after its stream has been synchronised)
            torch.cuda.synchronize()
            t_call.append(time.perf_counter() - t0)
        for k in range(KIN_SETS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(srcs[k])
            e1.record()
            e1.synchronize()
            t_copy.append(e0.elapsed_time(e1) * 1e-3)
    # From the child's one trace: the kernel, and the copy as the runtime carries it out -- its copy kernel, which also serves the
    # small uploads of the parameter row; the 15 large copies are its 15 longest dispatches.  Medians of the 15 of each.
    want = KIN_SETS * 5
    each = trace.get("dispatch_ns", {}) if isinstance(trace, dict) else {}
    kernel_s = copy_trace_s = None
    if len(each.get("inflx_kin_states", [])) == want:
        kernel_s = float(np.median(each["inflx_kin_states"])) * 1e-9
    if len(each.get(COPY_KERNEL, [])) >= want:
        copy_trace_s = float(np.median(each[COPY_KERNEL][:want])) * 1e-9
        each[COPY_KERNEL] = each[COPY_KERNEL][: want + 3]  # (the record keeps the large ones and the next three)
    copy_s = float(np.median(t_copy))
    rec = dict(model="hyperbolic", code_object=art._build[2], states=n, ld=6, traj_len=KIN_ROWS, read="plain per-lane loads (the one variant built)",
               input_sets=KIN_SETS, bytes_moved=moved, repeats=repeats * KIN_SETS, call_s=dict(best=min(t_call), median=float(np.median(t_call))),
               trace_ns=trace, kernel_s=kernel_s, copy_in_trace=COPY_KERNEL, copy_in_trace_s=copy_trace_s,
               kernel_over_copy_in_trace=None if kernel_s is None or copy_trace_s is None else kernel_s / copy_trace_s,
               d2d_copy_bytes=moved // 2, d2d_copy_events_s=dict(best=min(t_copy), median=copy_s), call_over_copy_events=float(np.median(t_call)) / copy_s,
               finite=bool(torch.isfinite(kin.omega).all()),
               note="call_s: wall time of background.kinematics on device rows (allocation and upload of the parameter row, one launch, a stream "
                    "synchronise); trace_ns: [launches or transfers, summed ns] of every kernel and memory copy of a child process under rocprofv3 that "
                    "makes 15 calls and 15 device-to-device copies of bytes_moved / 2 bytes (a copy reads and writes each), five rounds over three input "
                    "sets used in turn, so that what a call or a copy reads was last touched 1.4 GB of traffic earlier; trace_ns.dispatch_ns: the single "
                    "dispatches, longest first; kernel_s and copy_in_trace_s are the medians of the 15 kernel dispatches and of the 15 longest dispatches "
                    "of the runtime's copy kernel (its others are small uploads), from the one trace; d2d_copy_events_s: the same copies between device events in this process (launch overhead "
                    "included), alternating with the calls",
               command="python scripts/background_probe.py --kinematics")  # fmt: skip
    print(json.dumps(rec), flush=True)
    rec["accuracy"] = kinematics_accuracy()
    with open(os.path.join(ROOT, "profiles", "background_kinematics.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


def masses_workload(name, rounds=4):
    """what the --masses mode runs under the profiler, once per model: a warm-up, then ``rounds`` x KIN_SETS device-resident
    ``masses`` calls, as many ``kinematics`` calls on the same states and as many device-to-device copies of the bytes a masses call
    moves, each over input sets used in turn"""
    import torch

    spec, art, sets = _kinematics_rows(name)
    srcs, dst = _copy_buffers(sets, planes=8)
    for r in range(rounds + 1):
        for k in range(KIN_SETS):
            mass = background.masses(art, spec.args, sets[k])
        for k in range(KIN_SETS):
            background.kinematics(art, spec.args, sets[k])
        for k in range(KIN_SETS):
            dst.copy_(srcs[k])
        torch.cuda.synchronize()
    print(json.dumps({"masses_workload_mu_s2_nansum": float(torch.nansum(mass.mu_s2))}), flush=True)


def masses_accuracy():
    """worst |result - truth| / allowance per model and quantity, host build and GPU (tests/masses_reference.py)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import background_truth as bt
    import kinematics_reference as kr
    import masses_reference as mr

    rec = {}
    for name in bt.GPU_MODELS:
        states, pars = kr.zoo_states(name)
        truth = mr.zoo_truth(name, 257)
        host = mr.MassesTwin(bt.host_artifact(name)).masses(pars, states)
        gpu = np.stack(background.masses(bt.device_artifact(name), pars, states))
        allow = mr.allowance(truth, states[:, 4])
        with np.errstate(divide="ignore", invalid="ignore"):
            to_host = np.where(gpu == host, 0.0, np.abs(gpu - host) / allow)
        rec[name] = dict(host=mr.worst_ratios(host, truth, states[:, 4]), gpu=mr.worst_ratios(gpu, truth, states[:, 4]),
                         gpu_to_host=dict(zip(mr.NAMES, (float(r) for r in to_host.max(axis=1)))))  # fmt: skip
        print(json.dumps({name: rec[name]}), flush=True)
    worst = {side: max(max(rec[m][side].values()) for m in rec) for side in ("host", "gpu", "gpu_to_host")}
    return dict(states_per_model=257, allowance="tests/masses_reference.py allowance(): 1e-10 of the sum of the absolute values of the terms a quantity is built from",
                worst=worst, models=rec)  # fmt: skip


def masses_mode():
    """kernel time of ``inflx_mass_states`` on 2^22 states read in place from (2^14, 256, 6) rows, hyperbolic and EGNO, beside
    ``inflx_kin_states`` on the same states and the runtime's copy kernel moving the same bytes: one trace of a child process per
    model, medians of the 15 dispatches of each; then the accuracy record.  Writes profiles/background_masses.json."""
    want = KIN_SETS * 5
    n = (1 << KIN_LOG2_TRAJ) * KIN_ROWS
    moved = n * 6 * 8 + n * 8 * 8  # the lines of the (n, 6) rows read, the eight planes written
    timing = {}
    for name in ("hyperbolic", "egno"):  # first: this process has not opened the GPU yet
        trace = _kernel_trace(KIN_LOG2_TRAJ, "--masses-workload-" + name, "", extra=("--memory-copy-trace",), each=("inflx_mass_states", "inflx_kin_states", COPY_KERNEL))
        each = trace.get("dispatch_ns", {}) if isinstance(trace, dict) else {}
        rec = dict(code_object=workloads.artifact_for(name)[1]._build[2])
        for key, kernel in (("masses_kernel_s", "inflx_mass_states"), ("kinematics_kernel_s", "inflx_kin_states")):
            rec[key] = float(np.median(each[kernel])) * 1e-9 if len(each.get(kernel, [])) == want else None
        # (the copy kernel also serves the small uploads of the parameter row; the 15 large copies are its 15 longest dispatches)
        rec["copy_in_trace_s"] = float(np.median(each[COPY_KERNEL][:want])) * 1e-9 if len(each.get(COPY_KERNEL, [])) >= want else None
        if COPY_KERNEL in each:
            each[COPY_KERNEL] = each[COPY_KERNEL][: want + 3]
        if rec["masses_kernel_s"] and rec["copy_in_trace_s"]:
            rec["masses_over_copy_in_trace"] = rec["masses_kernel_s"] / rec["copy_in_trace_s"]
            rec["bytes_per_s"] = moved / rec["masses_kernel_s"]
        if rec["masses_kernel_s"] and rec["kinematics_kernel_s"]:
            rec["masses_over_kinematics"] = rec["masses_kernel_s"] / rec["kinematics_kernel_s"]
        rec["trace_ns"] = trace
        timing[name] = rec
        print(json.dumps({name: {k: v for k, v in rec.items() if k != "trace_ns"}}), flush=True)
    rec = dict(states=n, ld=6, traj_len=KIN_ROWS, read="plain per-lane loads (the one variant built)", input_sets=KIN_SETS, bytes_moved=moved, d2d_copy_bytes=moved // 2,
               copy_in_trace=COPY_KERNEL, timing=timing,
               note="per model one child process under rocprofv3 --kernel-trace that makes 15 device-resident masses calls, 15 kinematics calls on the same "
                    "states and 15 device-to-device copies of bytes_moved / 2 bytes (a copy reads and writes each), five rounds over three input sets used in "
                    "turn, so that what a call or a copy reads was last touched more than 1 GB of traffic earlier; masses_kernel_s, kinematics_kernel_s and "
                    "copy_in_trace_s are the medians of the 15 dispatches of inflx_mass_states, of inflx_kin_states and of the 15 longest dispatches of the "
                    "runtime's copy kernel, from the one trace; trace_ns.dispatch_ns: the single dispatches, longest first.  A kinematics call moves "
                    "96 bytes per state, a masses call and the copy 112",
               command="python scripts/background_probe.py --masses")  # fmt: skip
    rec["accuracy"] = masses_accuracy()
    with open(os.path.join(ROOT, "profiles", "background_masses.json"), "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", action="store_true", help="time the forced host scatter, the default host call and solve_eom_batch_device (B = 2^17, 256 rows), nothing else")
    ap.add_argument("--rows-workload", action="store_true", help="one device-resident call (what --rows runs under rocprofv3)")
    ap.add_argument("--sampled", action="store_true", help="time solve_eom_sampled (B = 2^17, S = 256) beside solve_eom_batch returning 256 rows, nothing else")
    ap.add_argument("--horizon-exit", action="store_true", help="time horizon_exit_map beside efolds_map at 1024^2 on hyperbolic, nothing else")
    ap.add_argument("--quick", action="store_true", help="B = 2^14 only (for a profiler run)")
    ap.add_argument("--max-log2-lanes", type=int, default=20)
    ap.add_argument("--kinematics", action="store_true", help="time background.kinematics on 2^22 device-resident states beside a device-to-device copy, and record its accuracy; nothing else")
    ap.add_argument("--kinematics-workload", action="store_true", help="a few device-resident kinematics calls (what --kinematics runs under rocprofv3)")
    ap.add_argument("--masses", action="store_true", help="time the masses kernel on 2^22 device-resident states (hyperbolic, EGNO) beside the kinematics kernel and a device-to-device copy, and record its accuracy; nothing else")
    ap.add_argument("--masses-workload-hyperbolic", action="store_true", help="a few device-resident masses calls on hyperbolic (what --masses runs under rocprofv3)")
    ap.add_argument("--masses-workload-egno", action="store_true", help="the same on EGNO")
    args = ap.parse_args()
    if args.masses_workload_hyperbolic or args.masses_workload_egno:
        masses_workload("egno" if args.masses_workload_egno else "hyperbolic")
        return
    if args.masses:
        masses_mode()
        return
    if args.kinematics_workload:
        kinematics_workload()
        return
    if args.kinematics:
        kinematics_mode()
        return
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
