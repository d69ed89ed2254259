"""Single-batch broadcast sweeps run evaluation and store stream on the caller's stream, with the parameter rows in the kernel
arguments and no event between sweeps (csrc/inflx_hip.cpp launch_broadcast).

Reference for every comparison: the same call under INFLX_SWEEP_FORCE_TILE -- every grid point through the tile kernels, parameters
through the slot ring, tables in the stage ring -- compared bit for bit.  Shapes are the smallest at which the row pass can go wrong:
grid rows around one 64-row block (1, 63, 64, 65, 129: a lone lane, a ragged block, a full one, two and three blocks) and N1 = 2, 86,
1366, which the AoS store stream cuts into 1, 2 (ragged tail) and 17 pieces of 256 units -- 1, 2 and 16 replicas of the table entry,
written by 1, 2 and 4 write slices."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GRID_ROWS = (1, 63, 64, 65, 129)
N1S = (2, 86, 1366)


@pytest.fixture(scope="module")
def hyp(gpu_lib):
    import workloads

    spec, art = workloads.artifact_for("hyperbolic")
    lib = gpu_lib.InflatoxDevLib(art.shared_object_path)
    assert lib.stage_info["out_mask"] & 2 == 0
    return spec, lib


def rows_for(spec, P, salt):
    """P parameter rows, no two alike, none shared between two values of `salt`."""
    base = np.asarray(spec.args, dtype=np.float64)
    return np.stack([base * (1.0 + 0.013 * q + 0.0031 * salt) + 0.002 * q for q in range(P)])


def sweep(lib, gpu_lib, op, rows, extent, n0, n1, layout, stream=0, force_tile=False, out=None, fill=-7.0):
    """One device-result sweep into a sentinel-filled buffer of its own (or into `out`), not synchronised."""
    import torch

    if out is None:
        count = rows.shape[0] * n0 * n1 * gpu_lib.OP_WIDTH[op]
        out = torch.full((count,), fill, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()  # the fill ran on torch's stream
    lib.sweep_device(op, rows, out.data_ptr(), out.numel() * 8, extent, n0, n1, layout=layout, stream=stream, force_tile=force_tile)
    return out


def same_bits(a, b):
    import torch

    return torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("what", ["aos6", "single_value", "soa_planes"])
def test_row_stream_equals_the_forced_tile_path(hyp, gpu_lib, what):
    import torch

    spec, lib = hyp
    op, layout = {"aos6": (gpu_lib.OP_COMPLETE, gpu_lib.LAYOUT_AOS), "single_value": (gpu_lib.OP_EPSILON_V, gpu_lib.LAYOUT_AOS),
                  "soa_planes": (gpu_lib.OP_COMPLETE, gpu_lib.LAYOUT_SOA)}[what]  # fmt: skip
    stream = torch.cuda.Stream(device="cuda:0")
    salt = 0
    for n0 in GRID_ROWS:
        for n1 in N1S:
            for P in (1, 2):
                salt += 1
                plan = lib.sweep_plan(op, P, n1, n0, layout=layout)
                assert plan["path"] == "row_stream" and plan["batches"] == 1, (n0, n1, P, plan)
                assert lib.sweep_plan(op, P, n1, n0, layout=layout, force_tile=True)["path"] == "tile"
                rows = rows_for(spec, P, salt)
                got = sweep(lib, gpu_lib, op, rows, spec.extent, n0, n1, layout, stream=stream.cuda_stream)
                want = sweep(lib, gpu_lib, op, rows, spec.extent, n0, n1, layout, stream=stream.cuda_stream, force_tile=True, fill=-9.0)
                stream.synchronize()
                lib.synchronize()
                assert same_bits(got, want), (what, n0, n1, P)
                assert not bool(torch.any(want == -9.0)), (what, n0, n1, P)
    if what == "aos6":
        # the replicas the shapes above were chosen for
        assert [lib.sweep_plan(op, 1, n1, 129)["replicas"] for n1 in N1S] == [1, 2, 16]


def test_several_table_batches_keep_the_side_stream(hyp, gpu_lib):
    """P > batch: 2^19 grid rows of one replica are 32 MiB of table per parameter row, two rows per 64 MiB batch, three rows two
    batches -- the double-buffered side stream, as inflx_sweep_plan reports -- between two single-batch sweeps on the same stream,
    which take the ring's buffers before and after it."""
    import torch

    spec, lib = hyp
    op, layout = gpu_lib.OP_COMPLETE, gpu_lib.LAYOUT_AOS
    n0, n1, P = 1 << 19, 2, 3
    plan = lib.sweep_plan(op, P, n1, n0)
    assert plan["path"] == "row_stream" and plan["batch_rows"] == 2 and plan["batches"] == 2, plan
    stream = torch.cuda.Stream(device="cuda:0")
    rows = rows_for(spec, P, 100)
    small = [rows_for(spec, 1, 101 + k) for k in range(2)]
    want = sweep(lib, gpu_lib, op, rows, spec.extent, n0, n1, layout, stream=stream.cuda_stream, force_tile=True, fill=-9.0)
    want_small = [sweep(lib, gpu_lib, op, r, spec.extent, 129, 86, layout, stream=stream.cuda_stream, force_tile=True, fill=-9.0) for r in small]
    outs = [torch.full_like(w, -7.0) for w in [want_small[0], want, want_small[1]]]
    stream.synchronize()
    lib.synchronize()
    torch.cuda.synchronize()
    sweep(lib, gpu_lib, op, small[0], spec.extent, 129, 86, layout, stream=stream.cuda_stream, out=outs[0])
    sweep(lib, gpu_lib, op, rows, spec.extent, n0, n1, layout, stream=stream.cuda_stream, out=outs[1])
    sweep(lib, gpu_lib, op, small[1], spec.extent, 129, 86, layout, stream=stream.cuda_stream, out=outs[2])
    stream.synchronize()
    lib.synchronize()
    assert same_bits(outs[0], want_small[0])
    assert same_bits(outs[1], want)
    assert same_bits(outs[2], want_small[1])


def test_column_only_mirror(gpu_lib):
    """colvals + colstream on the caller's stream: the column-only model of tests/test_models_extra.py, one small shape (two column
    blocks, the second ragged), AoS and planes, P = 1 and 2."""
    import torch
    from test_models_extra import setup

    from inflatox_amd import Compiler

    model, args, ext, *_ = setup("column_only")
    art = Compiler(model, silent=True).compile()  # (owns the code object file for as long as it lives)
    lib = gpu_lib.InflatoxDevLib(art.shared_object_path)
    stream = torch.cuda.Stream(device="cuda:0")
    n0, n1 = 65, 300
    for P in (1, 2):
        rows = np.stack([args * (1.0 + 0.03 * q) for q in range(P)])
        for layout in (gpu_lib.LAYOUT_AOS, gpu_lib.LAYOUT_SOA):
            plan = lib.sweep_plan(gpu_lib.OP_COMPLETE, P, n1, n0, layout=layout)
            assert plan["path"] == "col_stream" and plan["batches"] == 1, plan
            got = sweep(lib, gpu_lib, gpu_lib.OP_COMPLETE, rows, ext, n0, n1, layout, stream=stream.cuda_stream)
            want = sweep(lib, gpu_lib, gpu_lib.OP_COMPLETE, rows, ext, n0, n1, layout, stream=stream.cuda_stream, force_tile=True, fill=-9.0)
            stream.synchronize()
            lib.synchronize()
            assert same_bits(got, want), (P, layout)


@pytest.fixture(scope="module")
def scan(hyp, gpu_lib):
    """20 distinct parameter rows and the forced-tile result of each, computed once.  1024 x 8192: a store stream of 403 MB, about
    55 us -- several times what it takes the host to enqueue the next call, so that a table buffer taken early is taken from under
    a store stream that still reads it."""
    import torch

    spec, lib = hyp
    n0, n1 = 1024, 8192
    assert lib.has_row_pass  # the sweeps below run the row pass, not the core object's per-row kernels
    rows = [rows_for(spec, 1, 200 + k) for k in range(20)]
    want = torch.full((20, n0 * n1 * 6), -9.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    for k, r in enumerate(rows):
        sweep(lib, gpu_lib, gpu_lib.OP_COMPLETE, r, spec.extent, n0, n1, gpu_lib.LAYOUT_AOS, force_tile=True, out=want[k])
    lib.synchronize()
    torch.cuda.synchronize()
    assert not bool(torch.any(want == -9.0))
    assert len({want[k].view(torch.int64)[: 6 * n1].cpu().numpy().tobytes() for k in range(20)}) == 20  # no two calls alike
    return n0, n1, rows, want


# which caller stream call k goes to.  Every call is one table batch and takes the ring's buffers in turn (buffer k % 2):
#   one  -- a scan on one stream: stream order alone;
#   aab  -- A A B A A B ...: from call 2 on, two calls of three take a buffer whose last user ran on the OTHER stream (call 2 on B
#           takes buffer 0 from call 0 on A, call 4 on A takes it back, call 5 on B takes buffer 1 from call 3 on A, ...);
#   abc  -- three streams in turn: every call from the third on takes its buffer from another stream.
# The last user's store stream (about 55 us) is still queued or running when the next call is enqueued about 10 us later: without the
# ordering of TableRing::order_behind_solo the new row pass overwrites table entries that store stream has yet to read.
PATTERNS = {"one": lambda k: 0, "aab": lambda k: 1 if k % 3 == 2 else 0, "abc": lambda k: k % 3}


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
def test_twenty_back_to_back_sweeps(hyp, gpu_lib, scan, pattern):
    """20 sweeps with 20 parameter rows into 20 result slices, enqueued without a synchronisation on the caller streams PATTERNS
    names; every slice must be the forced-tile result of ITS parameters.  The parameter array handed to a call is overwritten as
    soon as the call returns."""
    import torch

    spec, lib = hyp
    n0, n1, rows, want = scan
    stream_of = PATTERNS[pattern]
    callers = [torch.cuda.Stream(device="cuda:0") for _ in range(3)]
    got = torch.full_like(want, -7.0)
    torch.cuda.synchronize()
    # hand-offs this pattern makes: calls whose buffer was last used on another stream
    handoffs = [k for k in range(2, 20) if stream_of(k) != stream_of(k - 2)]
    assert len(handoffs) == {"one": 0, "aab": 12, "abc": 18}[pattern]
    buf = np.empty_like(rows[0])
    for k, r in enumerate(rows):
        buf[:] = r
        sweep(lib, gpu_lib, gpu_lib.OP_COMPLETE, buf, spec.extent, n0, n1, gpu_lib.LAYOUT_AOS, stream=callers[stream_of(k)].cuda_stream, out=got[k])
        buf[:] = np.nan  # the caller's array is dead after the call
    for s in callers:
        s.synchronize()
    lib.synchronize()
    bad = [k for k in range(20) if not same_bits(got[k], want[k])]
    assert not bad, f"sweeps {bad} differ from their forced-tile results (hand-offs at {handoffs})"


def test_parameter_slot_hit_from_another_stream(gpu_lib):
    """acquire_params finds a call's bytes in the current slot although another stream uploaded them, and must not read them before
    that upload ran.  Tile path (doc model; the row pass of a row-only model uses no slot): stream A is kept busy by a sweep of a
    SECOND handle, then the handle under test -- idle, so everything goes to the caller's stream -- gets parameters X on A: upload
    and kernels are queued behind the busy sweep.  The same X on stream B arrives at a handle that is no longer idle: its stage
    tables go to the side stream and hit the slot.  Without the wait for the slot's event they would read what the slot held
    before (the warm-up's parameters).  Both results must be those of X."""
    import torch

    import workloads

    spec, art = workloads.artifact_for("doc")
    lib, other = gpu_lib.InflatoxDevLib(art.shared_object_path), gpu_lib.InflatoxDevLib(art.shared_object_path)
    op, lay = gpu_lib.OP_COMPLETE, gpu_lib.LAYOUT_AOS
    n0, n1 = 97, 300
    assert lib.sweep_plan(op, 1, n1, n0)["path"] == "tile"
    base = np.asarray(spec.args, dtype=np.float64)
    base = base.reshape(1, -1)
    x, warm = base * 1.07, base * 0.93
    a, b = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    want = sweep(lib, gpu_lib, op, x, spec.extent, n0, n1, lay, stream=a.cuda_stream, fill=-9.0)
    a.synchronize()
    lib.synchronize()
    for _ in range(4):  # the four slots and both stage buffers hold the warm-up's parameters
        sweep(lib, gpu_lib, op, warm, spec.extent, n0, n1, lay, stream=a.cuda_stream)
        warm = warm * 1.001
        a.synchronize()
        lib.synchronize()
    busy = torch.empty((4096 * 4096 * 6,), dtype=torch.float64, device="cuda:0")
    got_a = torch.full_like(want, -7.0)
    got_b = torch.full_like(want, -7.0)
    torch.cuda.synchronize()
    sweep(other, gpu_lib, op, base, spec.extent, 4096, 4096, lay, stream=a.cuda_stream, out=busy)  # keeps A busy; not the handle under test
    sweep(lib, gpu_lib, op, x, spec.extent, n0, n1, lay, stream=a.cuda_stream, out=got_a)
    sweep(lib, gpu_lib, op, x, spec.extent, n0, n1, lay, stream=b.cuda_stream, out=got_b)
    a.synchronize()
    b.synchronize()
    lib.synchronize()
    other.synchronize()
    assert same_bits(got_a, want)
    assert same_bits(got_b, want)
