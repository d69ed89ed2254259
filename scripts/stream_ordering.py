#!/usr/bin/env python3
"""Cross-stream ordering of the device-result sweeps (GPU box), run by tests/test_stream_ordering_gpu.py in ONE child process with
GPU_MAX_HW_QUEUES=16, so that the handle's two streams, torch's default stream and the streams below each get a hardware queue
of their own (two streams on one queue would serialise exactly what is under test).

The adversary: a bounded device-side spin (torch.cuda._sleep, 100-500 ms) holds stream A back.  Every case enqueues its calls on A
and on other streams, and only then compares every result bit for bit (int64 views) with sweep_host of the same parameters, shape,
operation, row range and layout; the output buffers start as -7.0, so elements nobody wrote show up.  A case proves that the
adversary held: an event recorded behind the spin is still pending when the calls under test have been enqueued, and in the
cross-stream cases B.synchronize() returns while it is still pending (B's sweeps were not serialised behind A).  Calls that are
entitled to wait for A -- a parameter slot or a table / stage buffer that a sweep on A still reads -- come after those checks.

Prints one line per case, "CASE <id> PASS <details>" or "CASE <id> FAIL <reason>", then "stream ordering finished: ..."; exits 1
when a case failed and 2 on any other error (a HIP error ends the run: nothing more is started on the GPU after it).
usage: stream_ordering.py [case-id-prefix ...]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import workloads  # noqa: E402
from inflatox_amd import _native as N  # noqa: E402

SPIN_MS = 200.0  # target length of one hold; the calibration keeps every hold between 100 and 500 ms
WORKLOADS = ("hyperbolic", "doc", "angular", "egno", "d5")
SENTINEL = -7.0

# ---- models -------------------------------------------------------------------------------------------------------------------
_models = {}


def _column_only():
    """Nothing depends on x[0] (the column_only model of tests/test_models_extra.py): the column-broadcast path."""
    import sympy as sp

    from inflatox_amd import Compiler, InflationModelBuilder

    x, y = sp.symbols("x y", real=True)
    a, b = sp.symbols("a b", real=True)
    V = a * (y - b) ** 2 / 2
    G = [[1 + y**2, 0], [0, 1]]
    model = InflationModelBuilder.new([x, y], G, V, model_name="column_only", silent=True, init_sympy_printing=False, simplify=False, assertions=False).build()
    return Compiler(model, silent=True).compile(), np.array([1.3, 0.4]), (-1.0, 1.0, -2.0, 1.5)


def model(name):
    """(artefact, InflatoxDevLib, base parameters, start_stop) of one model, opened once per process."""
    if name not in _models:
        if name == "column_only":
            art, args, ext = _column_only()
        else:
            spec, art = workloads.artifact_for(name)
            args, ext = np.asarray(spec.args, dtype=np.float64), spec.extent
        _models[name] = (art, N.InflatoxDevLib(art.shared_object_path), args, np.array([[ext[0], ext[1]], [ext[2], ext[3]]]))
    return _models[name]


def rows_of(name, P, tag):
    """P parameter rows of `name`, distinct for every (row, tag): tags keep the calls of one sequence apart."""
    base = model(name)[2]
    return np.stack([base * (1.0 + 0.003 * q + 0.011 * tag) for q in range(P)])


# ---- the adversary ------------------------------------------------------------------------------------------------------------
class Spin:
    """Cycles per millisecond of torch.cuda._sleep, measured with a pair of timing events and refreshed after every hold (its
    clock is not a fixed rate)."""

    def __init__(self):
        s = torch.cuda.Stream()
        cycles, ms = 1 << 20, 0.0
        for _ in range(8):
            ms = self._time(s, cycles)
            if ms >= 20.0:
                break
            cycles = int(cycles * min(16.0, 40.0 / max(ms, 0.05)))
        self.rate = cycles / ms
        self.held_ms = []

    @staticmethod
    def _time(s, cycles):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            torch.cuda._sleep(int(cycles))
            e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1)


class Hold:
    """A held back by the spin; `held` is recorded behind it."""

    def __init__(self, spin, stream):
        self.spin, self.stream = spin, stream
        self.cycles = int(spin.rate * SPIN_MS)
        self.t0, self.held = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self.t0.record(stream)
            torch.cuda._sleep(self.cycles)
            self.held.record(stream)
        self.checks = []

    def pending(self, where):
        """The spin must still hold A at this point of the case: otherwise the case proved nothing."""
        if self.held.query():
            raise AssertionError(f"vacuous: the spin on A had already finished {where}")
        self.checks.append(where)

    def others_finished(self, stream, what):
        """`stream`'s work must finish while A is still held: if it waited for the spin, the streams were serialised."""
        self.pending(f"before {what} was waited for")
        stream.synchronize()
        if self.held.query():
            raise AssertionError(f"vacuous: {what} finished only after the spin on A -- it was serialised behind A, so the case did not race")
        self.checks.append(f"{what} done under the spin")

    def release(self):
        self.held.synchronize()
        ms = self.t0.elapsed_time(self.held)
        self.spin.held_ms.append(ms)
        self.spin.rate = self.cycles / ms  # the clock of the next hold is closer to this one's than to the calibration's
        return ms


# ---- calls ------------------------------------------------------------------------------------------------------------------
class Sweep:
    """One device-result sweep and its expectation (sweep_host of the same parameters, shape, operation, row range and layout)."""

    def __init__(self, name, op, P, n0, n1, tag, rb=0, rc=None, layout=N.LAYOUT_AOS, force_tile=False):
        self.name, self.op, self.n0, self.n1, self.rb = name, op, n0, n1, rb
        self.rc = n0 - rb if rc is None else rc
        self.layout, self.force_tile = layout, force_tile
        self.p = rows_of(name, P, tag)
        self.art, self.lib, _, self.ss = model(name)
        self.out = None

    def __repr__(self):
        lay = "soa" if self.layout == N.LAYOUT_SOA else "aos"
        return f"{self.name}/op{self.op}/P{len(self.p)}/{self.n0}x{self.n1}/rows{self.rb}+{self.rc}/{lay}{'/force_tile' if self.force_tile else ''}"

    def plan(self):
        return self.lib.sweep_plan(self.op, len(self.p), self.n1, self.rc, layout=self.layout, force_tile=self.force_tile)

    def prepare(self, warm_stream):
        """Expectation, sentinel-filled output, and one unblocked sweep of the same shape (other parameters) that sizes the
        tables, stage buffers and slots: otherwise a buffer that grows waits for the whole device, the spin included."""
        self.want = self.lib.sweep_host(self.op, self.p, self.ss, self.n0, self.n1, row_begin=self.rb, row_count=self.rc, layout=self.layout)
        self.out = torch.full((self.want.size,), SENTINEL, dtype=torch.float64, device="cuda:0")
        scratch = torch.empty_like(self.out)
        torch.cuda.synchronize()
        for _ in range(2):  # consecutive launches take the two buffers of a pair in turn: both are sized
            self.enqueue(warm_stream, p=self.p * 0.97, out=scratch)
        warm_stream.synchronize()
        return self

    def enqueue(self, stream, p=None, out=None):
        out = self.out if out is None else out
        sid = stream if isinstance(stream, int) else stream.cuda_stream
        self.lib.sweep_device(self.op, self.p if p is None else p, out.data_ptr(), out.numel() * 8, self.ss, self.n0, self.n1, row_begin=self.rb, row_count=self.rc,
                              layout=self.layout, stream=sid, force_tile=self.force_tile)  # fmt: skip

    def check(self, label):
        compare(self.out.cpu().numpy(), self.want, f"{label} {self!r}")


def compare(got, want, what):
    g = np.ascontiguousarray(got).reshape(-1).view(np.int64)
    w = np.ascontiguousarray(want).reshape(-1).view(np.int64)
    bad = (g != w) & ~(np.isnan(g.view(np.float64)) & np.isnan(w.view(np.float64)))
    if bad.any():
        first = int(np.flatnonzero(bad)[0])
        unwritten = int((g[bad] == np.float64(SENTINEL).view(np.int64)).sum())
        raise AssertionError(f"{what}: {int(bad.sum())} of {g.size} elements differ ({unwritten} never written), first at {first}: "
                             f"got {g.view(np.float64)[first]!r}, want {w.view(np.float64)[first]!r}")  # fmt: skip


def settle(*libs):
    for lib in libs:
        lib.synchronize()
    torch.cuda.synchronize()


def expect_path(sweep, path):
    got = sweep.plan()["path"]
    assert got == path, f"{sweep!r} takes the {got} path, the case needs {path}"


# ---- cases ------------------------------------------------------------------------------------------------------------------
CASES = []


def case(fn):
    CASES.append(fn)
    return fn


LONE = {"row": ("hyperbolic", N.OP_COMPLETE, 48, 256, "row_stream"), "col": ("column_only", N.OP_COMPLETE, 48, 256, "col_stream"),
        "tile": ("doc", N.OP_COMPLETE, 48, 256, "tile")}  # fmt: skip


def make_case1(lone, follow):
    def case1(spin, A, B):
        """A lone sweep on blocked A, then five sweeps with distinct parameters on B: the fifth parameter upload cycles the
        four-slot ring back onto the lone sweep's slot while that sweep has not run."""
        name, op, n0, n1, path = LONE[lone]
        first = Sweep(name, op, 1, n0, n1, tag=0)
        rest = [Sweep(name, op, 1 + k % 2, n0, n1, tag=1 + k, force_tile=follow == "tile") for k in range(5)]
        expect_path(first, path)
        for s in rest:
            expect_path(s, "tile" if follow == "tile" else path)
        for s in [first] + rest:
            s.prepare(B)
        settle(first.lib)
        # the follow-ups that share no table / stage buffer with the lone sweep run under the spin; one that does waits for it
        free = 3 if (path == "tile") != (follow == "tile" or path == "tile") else 1
        hold = Hold(spin, A)
        first.enqueue(A)  # the handle is idle: a lone call
        for s in rest[:free]:
            s.enqueue(B)
        hold.others_finished(B, f"B's first {free} sweep(s)")
        for s in rest[free:3]:
            s.enqueue(B)
        hold.pending("when the ring was about to reuse the lone sweep's slot")
        for s in rest[3:]:
            s.enqueue(B)
        hold.release()
        settle(first.lib)
        first.check("lone sweep on A")
        for k, s in enumerate(rest):
            s.check(f"follow-up {k} on B")
        return hold

    case1.__name__ = f"case1_lone_{lone}_then_{follow}"
    return case1


for _lone in ("row", "col", "tile"):
    for _follow in ("same", "tile"):
        case(make_case1(_lone, _follow))


def _alternate(spin, A, B, sweeps, big, path_of):
    """Sweeps alternately on blocked A and on B (A first, from an idle handle), then `big` on B."""
    for s in sweeps + [big]:
        s.prepare(B)
    settle(sweeps[0].lib)
    hold = Hold(spin, A)
    sweeps[0].enqueue(A)
    sweeps[1].enqueue(B)  # the other table / stage buffer: free
    hold.others_finished(B, "B's first sweep")
    for k in range(2, 4):
        sweeps[k].enqueue(A if k % 2 == 0 else B)
    hold.pending("when the buffers had been handed back and forth twice")
    for k in range(4, len(sweeps)):
        sweeps[k].enqueue(A if k % 2 == 0 else B)
    big.enqueue(B)
    hold.release()
    settle(sweeps[0].lib)
    for k, s in enumerate(sweeps):
        s.check(f"alternating sweep {k} on {'AB'[k % 2]}")
    big.check("multi-batch sweep on B")
    return hold


def _multi_batch(name, op, path, P, candidates, layout=N.LAYOUT_AOS):
    for n0, n1 in candidates:
        s = Sweep(name, op, P, n0, n1, tag=40, layout=layout)
        plan = s.plan()
        if plan["path"] == path and plan["batches"] >= 2:
            return s
    raise AssertionError(f"no shape of {candidates} gives {name} a {path} sweep of two or more batches")


@case
def case2_tables_row(spin, A, B):
    """The row table double buffer under sweeps in flight on two streams, and a sweep of two or more table batches."""
    sweeps = [Sweep("hyperbolic", N.OP_COMPLETE if k % 3 else N.OP_CONSISTENCY, 1 + k % 3, 40 + 8 * k, 256, tag=k, layout=N.LAYOUT_AOS) for k in range(6)]
    for s in sweeps:
        expect_path(s, "row_stream")
    big = _multi_batch("hyperbolic", N.OP_CONSISTENCY, "row_stream", 3, [(n0, 2) for n0 in (1 << 17, 1 << 18, 350_000, 1 << 19)])
    return _alternate(spin, A, B, sweeps, big, "row_stream")


@case
def case2_tables_col(spin, A, B):
    sweeps = [Sweep("column_only", N.OP_COMPLETE if k % 3 else N.OP_CONSISTENCY, 1 + k % 3, 40 + 8 * k, 256, tag=k,
                    layout=N.LAYOUT_SOA if k == 4 else N.LAYOUT_AOS) for k in range(6)]  # fmt: skip
    for s in sweeps:
        expect_path(s, "col_stream")
    big = _multi_batch("column_only", N.OP_CONSISTENCY, "col_stream", 3, [(1, n1) for n1 in (1 << 21, 3_000_000, 1 << 22)])
    return _alternate(spin, A, B, sweeps, big, "col_stream")


def make_case3(name):
    def case3(spin, A, B):
        """The two tile-stage buffers the same way, and a multi-launch tile sweep (a grid taller than one launch)."""
        sweeps = [Sweep(name, N.OP_COMPLETE if k % 3 else N.OP_CONSISTENCY, 1 + k % 3, 40 + 8 * k, 200 + 16 * k, tag=k, rb=k, layout=N.LAYOUT_SOA if k == 3 else N.LAYOUT_AOS) for k in range(6)]
        for s in sweeps:
            expect_path(s, "tile")
        tall = _multi_batch(name, N.OP_CONSISTENCY, "tile", 2, [(n0, 1) for n0 in (1 << 19, 1 << 20, 1 << 21, 1 << 22, 1 << 23)])
        return _alternate(spin, A, B, sweeps, tall, "tile")

    case3.__name__ = f"case3_stage_{name}"
    return case3


for _name in ("doc", "egno", "d5"):
    case(make_case3(_name))


def make_case4(name, path):
    def case4(spin, A, B):
        """A sweep on B with the parameters of a sweep still pending on A: the cache-hit branch of acquire_params and the
        cross-stream wait of release_params; then four sweeps with distinct parameters cycle the ring."""
        busy = Sweep(name, N.OP_COMPLETE, 1, 48, 256, tag=0)
        on_a = Sweep(name, N.OP_COMPLETE, 2, 48, 256, tag=1)
        on_b = Sweep(name, N.OP_COMPLETE, 2, 48, 256, tag=1)  # same parameters, its own output
        rest = [Sweep(name, N.OP_COMPLETE, 1 + k % 2, 48, 256, tag=2 + k) for k in range(4)]
        for s in [busy, on_a, on_b] + rest:
            expect_path(s, path)
            s.prepare(B)
        settle(busy.lib)
        hold = Hold(spin, A)
        busy.enqueue(A)  # the handle is busy from here on: the next two upload on the side stream, the second finds the slot filled
        on_a.enqueue(A)
        on_b.enqueue(B)
        hold.pending("when the cache hit had been enqueued")
        for s in rest:
            s.enqueue(B)
        hold.release()
        settle(busy.lib)
        for label, s in [("busy sweep on A", busy), ("sweep on A", on_a), ("cache hit on B", on_b)] + [(f"follow-up {k} on B", r) for k, r in enumerate(rest)]:
            s.check(label)
        return hold

    case4.__name__ = f"case4_cache_hit_{path}"
    return case4


case(make_case4("hyperbolic", "row_stream"))
case(make_case4("egno", "tile"))


@case
def case5_host_calls_in_between(spin, A, B):
    """Host-result calls on the same handle while its device sweeps are pending on A: their own results and the pending ones."""
    name = "hyperbolic"
    art, lib, base, ss = model(name)
    dev = [Sweep(name, N.OP_COMPLETE, 1, 48, 256, tag=k) for k in range(3)]
    for s in dev:
        s.prepare(B)
    p_host, p_traj, p_stats = rows_of(name, 2, 10), rows_of(name, 1, 11)[0], rows_of(name, 2, 12)
    want_host = lib.sweep_host(N.OP_CONSISTENCY, p_host, ss, 40, 96, row_begin=3, row_count=30, layout=N.LAYOUT_SOA)
    pts = np.column_stack([np.linspace(ss[0, 0], ss[0, 1], 257), np.linspace(ss[1, 0], ss[1, 1], 257)])
    want_traj = lib.sweep_on_trajectory(N.OP_RAW, p_traj, pts)
    want_stats = lib.sweep_stats(p_stats, ss, 32, 128)
    want_full = lib.sweep_host(N.OP_COMPLETE, p_stats, ss, 32, 128)
    d_out = torch.full((want_full.size,), SENTINEL, dtype=torch.float64, device="cuda:0")
    settle(lib)
    hold = Hold(spin, A)
    dev[0].enqueue(A)
    dev[1].enqueue(A)
    dev[2].enqueue(B)
    hold.pending("when the device sweeps had been enqueued")
    got_host = lib.sweep_host(N.OP_CONSISTENCY, p_host, ss, 40, 96, row_begin=3, row_count=30, layout=N.LAYOUT_SOA)
    got_traj = lib.sweep_on_trajectory(N.OP_RAW, p_traj, pts)
    got_stats = lib.sweep_stats(p_stats, ss, 32, 128)
    got_stats_out = lib.sweep_stats(p_stats, ss, 32, 128, d_out_ptr=d_out.data_ptr(), d_out_bytes=d_out.numel() * 8, stream=B.cuda_stream)
    hold.release()
    settle(lib)
    compare(got_host, want_host, "sweep_host in between")
    compare(got_traj, want_traj, "sweep_on_trajectory in between")
    for key in ("min", "max", "count"):
        compare(got_stats[key], want_stats[key], f"sweep_stats in between: {key}")
        compare(got_stats_out[key], want_stats[key], f"sweep_stats(d_out) in between: {key}")
    compare(d_out.cpu().numpy(), want_full, "sweep_stats(d_out) result")
    for k, s in enumerate(dev):
        s.check(f"device sweep {k}")
    return hold


@case
def case6_multi_device_handle(spin, A, B):
    """InflatoxMultiLib on devices [0, 0] with a stream per device, the first one blocked; five calls cycle both handles' rings."""
    name = "hyperbolic"
    art, lib, base, ss = model(name)
    multi = N.InflatoxMultiLib(art.shared_object_path, devices=[0, 0])
    try:
        n = multi.n_devices
        P, n0, n1, K = 2, 48, 256, 6
        calls = []
        for tag in range(6):
            p = rows_of(name, P, 20 + tag)
            full = lib.sweep_host(N.OP_COMPLETE, p, ss, n0, n1)
            blocks, outs = [], []
            for k in range(n):
                sp = N.shard_plan(P, n0, n, k)
                blk = full[sp["p_begin"]:sp["p_begin"] + sp["p_count"], sp["row_begin"]:sp["row_begin"] + sp["row_count"]]
                blocks.append(np.ascontiguousarray(blk))
                outs.append(torch.full((max(blk.size, 1),), SENTINEL, dtype=torch.float64, device="cuda:0"))
            calls.append((p, blocks, outs))
        # warm-up: one unblocked call of the same shape
        scratch = [torch.empty_like(o) for o in calls[0][2]]
        for _ in range(2):  # both table buffers of every handle
            multi.sweep_device(N.OP_COMPLETE, calls[0][0] * 0.97, [t.data_ptr() for t in scratch], [t.numel() * 8 for t in scratch], ss, n0, n1, streams=[B.cuda_stream] * n)
        torch.cuda.synchronize()
        for k in range(n):
            N._check(multi._lib.inflx_synchronize(multi._lib.inflx_multi_handle(multi._h, k)))
        C = torch.cuda.Stream()
        hold = Hold(spin, A)
        for j, (p, blocks, outs) in enumerate(calls):
            streams = [A, B] if j == 0 else [C, B]
            multi.sweep_device(N.OP_COMPLETE, p, [t.data_ptr() for t in outs], [t.numel() * 8 for t in outs], ss, n0, n1, streams=[s.cuda_stream for s in streams])
            if j == 0:
                hold.others_finished(B, "device 1's sweep on B")
            if j == 3:
                hold.pending("when the rings were about to cycle")
        hold.release()
        for k in range(n):
            N._check(multi._lib.inflx_synchronize(multi._lib.inflx_multi_handle(multi._h, k)))
        torch.cuda.synchronize()
        for j, (p, blocks, outs) in enumerate(calls):
            for k in range(n):
                if blocks[k].size:
                    compare(outs[k].cpu().numpy()[: blocks[k].size], blocks[k], f"multi-device call {j}, device {k}")
        return hold
    finally:
        multi.close()


@case
def case7_front_end(spin, A, B):
    """GeneralisedAL.complete_analysis_device under torch.cuda.stream(A) with A blocked, then under B, with other parameters."""
    from inflatox_amd.consistency_conditions import GeneralisedAL

    name = "hyperbolic"
    art, lib, base, ss = model(name)
    al = GeneralisedAL(art)
    n0, n1 = 48, 256
    ext = (ss[0, 0], ss[0, 1], ss[1, 0], ss[1, 1])
    params = [rows_of(name, 1, 30 + k)[0] for k in range(6)]
    wants = [al.dylib.sweep_host(N.OP_COMPLETE, p, ss, n0, n1) for p in params]
    for _ in range(2):  # warm-up: the front end's stream, both table buffers
        al.complete_analysis_device(params[0] * 0.97, *ext, n0, n1)
    al.dylib.synchronize()
    torch.cuda.synchronize()
    hold = Hold(spin, A)
    got = []
    for k, p in enumerate(params):
        with torch.cuda.stream(A if k == 0 else B):
            got.append(al.complete_analysis_device(p, *ext, n0, n1))
        if k == 3:
            hold.pending("when the ring was about to cycle")
    hold.release()
    al.dylib.synchronize()
    torch.cuda.synchronize()
    for k, (g, w) in enumerate(zip(got, wants)):
        compare(torch.stack(g, dim=-1).cpu().numpy(), w, f"complete_analysis_device call {k} ({'AB'[min(k, 1)]})")
    return hold


SEEDS = tuple(range(8))
OPS = [(N.OP_COMPLETE, 6), (N.OP_CONSISTENCY, 1), (N.OP_RAW, 5), (N.OP_EPSILON_V, 1), (N.OP_RAPIDTURN, 1), (N.OP_HESSE, 4)]


def make_case8(seed):
    def case8(spin, A, B):
        """A seeded random sequence of up to 10 calls on A (blocked), B, C and the handle's own stream."""
        rng = np.random.default_rng(1000 + seed)
        C = torch.cuda.Stream()
        streams = {"A": A, "B": B, "C": C, "own": 0}
        name = (WORKLOADS + ("column_only",))[seed % 6]
        art, lib, base, ss = model(name)
        n0, n1 = int(rng.choice([17, 48, 96])), int(rng.choice([64, 130, 256, 301]))
        ops = OPS[:2] if name == "column_only" else OPS
        seq = []
        for j in range(int(rng.integers(6, 11))):
            # (column_only: no stats group, which is built on first use)
            kinds = ["device"] * 6 + ["host"] + ([] if name == "column_only" else ["stats", "stats_out"])
            kind = "device" if j == 0 else str(rng.choice(kinds))
            on = "A" if j == 0 else str(rng.choice(["A", "B", "C", "own"]))
            P = int(rng.integers(1, 5))
            rb = int(rng.integers(0, n0 // 2))
            rc = int(rng.integers(1, n0 - rb + 1))
            if kind == "device":
                op, _ = ops[int(rng.integers(0, len(ops)))]
                lay = N.LAYOUT_SOA if rng.integers(0, 2) else N.LAYOUT_AOS
                s = Sweep(name, op, P, n0, n1, tag=j, rb=rb, rc=rc, layout=lay, force_tile=bool(rng.integers(0, 4) == 0))
                seq.append((kind, on, s))
            else:
                seq.append((kind, on, (rows_of(name, P, j), rb, rc)))
        trace = [f"{k}@{on}:{x!r}" if k == "device" else f"{k}@{on}:P{len(x[0])}/rows{x[1]}+{x[2]}" for k, on, x in seq]
        where = f"seed {1000 + seed}, {name} {n0}x{n1}: " + " ; ".join(trace)
        wants = []
        for kind, on, x in seq:
            if kind == "device":
                x.prepare(B)
                wants.append(None)
            elif kind == "host":
                wants.append(lib.sweep_host(N.OP_COMPLETE, x[0], ss, n0, n1, row_begin=x[1], row_count=x[2]))
            else:
                full = lib.sweep_host(N.OP_COMPLETE, x[0], ss, n0, n1, row_begin=x[1], row_count=x[2]) if kind == "stats_out" else None
                wants.append((lib.sweep_stats(x[0], ss, n0, n1, row_begin=x[1], row_count=x[2]), full))
        outs = [torch.full((w[1].size,), SENTINEL, dtype=torch.float64, device="cuda:0") if kind == "stats_out" else None for (kind, _, _), w in zip(seq, wants)]
        settle(lib)
        hold = Hold(spin, A)
        got = []
        try:
            for j, (kind, on, x) in enumerate(seq):
                sid = streams[on] if on == "own" else streams[on].cuda_stream
                if kind == "device":
                    x.enqueue(sid)
                    got.append(None)
                elif kind == "host":
                    got.append(lib.sweep_host(N.OP_COMPLETE, x[0], ss, n0, n1, row_begin=x[1], row_count=x[2]))
                else:
                    o = outs[j]
                    got.append(lib.sweep_stats(x[0], ss, n0, n1, row_begin=x[1], row_count=x[2], d_out_ptr=0 if o is None else o.data_ptr(),
                                               d_out_bytes=0 if o is None else o.numel() * 8, stream=sid))  # fmt: skip
                if j == 0:
                    hold.pending("when the first call of the sequence had been enqueued")
            hold.release()
            settle(lib)
            for j, (kind, on, x) in enumerate(seq):
                if kind == "device":
                    x.check(f"call {j} ({on})")
                elif kind == "host":
                    compare(got[j], wants[j], f"call {j} sweep_host")
                else:
                    for key in ("min", "max", "count"):
                        compare(got[j][key], wants[j][0][key], f"call {j} {kind} {key}")
                    if outs[j] is not None:
                        compare(outs[j].cpu().numpy(), wants[j][1], f"call {j} {kind} result")
        except AssertionError as e:
            raise AssertionError(f"{e} [{where}]") from None
        return hold

    case8.__name__ = f"case8_random_seed{seed}"
    return case8


for _seed in SEEDS:
    case(make_case8(_seed))


def main(prefixes):
    assert torch.cuda.is_available(), "no HIP device"
    t_start = time.time()
    spin = Spin()
    print(f"spin: {spin.rate / 1e3:.0f} kcycles/ms (GPU_MAX_HW_QUEUES={os.environ.get('GPU_MAX_HW_QUEUES')})", flush=True)
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    failed = ran = 0
    for fn in CASES:
        if prefixes and not any(fn.__name__.startswith(p) for p in prefixes):
            continue
        ran += 1
        t0 = time.time()
        try:
            hold = fn(spin, A, B)
        except AssertionError as e:
            failed += 1
            torch.cuda.synchronize()  # whatever the case left enqueued runs out before the next case starts
            print(f"CASE {fn.__name__} FAIL {e}", flush=True)
            continue
        except Exception as e:  # a HIP error: nothing more is started on the GPU
            print(f"CASE {fn.__name__} ERROR {type(e).__name__}: {e}", flush=True)
            return 2
        print(f"CASE {fn.__name__} PASS held {spin.held_ms[-1]:.0f} ms; {len(hold.checks)} pending checks: {' | '.join(hold.checks)} ({time.time() - t0:.1f} s)", flush=True)
    held = spin.held_ms
    print(f"holds: {len(held)}, {min(held, default=0):.0f}-{max(held, default=0):.0f} ms", flush=True)
    print(f"stream ordering finished: {ran} cases, {failed} failed, {time.time() - t_start:.1f} s")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
