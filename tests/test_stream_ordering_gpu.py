"""Cross-stream ordering of the device-result sweeps: scripts/stream_ordering.py holds a torch stream back with a bounded device-side
spin, enqueues sweeps on it and on other streams, and compares every result bit for bit with sweep_host.  The parameter ring
(four slots), the two row / column tables and the two tile-stage buffers are reused while sweeps on the held stream have not run:
a slot or buffer handed on before its last reader ran shows up as a wrong result, deterministically.

All cases run in ONE child process with GPU_MAX_HW_QUEUES=16 (set in the child's environment only): the handle's two streams,
torch's default stream and the test's streams would otherwise share the four default hardware queues, and two streams on one
queue serialise exactly what is under test.  Each case also proves that its adversary held (the spin still pending when the
calls under test were enqueued, and the other stream's sweeps finished under it where the case is a cross-stream race)."""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = (
    # 1. a lone sweep on the held stream (tables on the caller's stream), then five sweeps on B cycle the parameter ring
    "case1_lone_row_then_same",
    "case1_lone_row_then_tile",
    "case1_lone_col_then_same",
    "case1_lone_col_then_tile",
    "case1_lone_tile_then_same",  # the control: the tile path released its slot on the right stream before the fix
    "case1_lone_tile_then_tile",
    # 2. / 3. the table and stage double buffers handed between the held stream and B, with a multi-batch / multi-launch sweep
    "case2_tables_row",
    "case2_tables_col",
    "case3_stage_doc",
    "case3_stage_egno",
    "case3_stage_d5",
    # 4. a parameter-cache hit on B for a sweep still pending on the held stream
    "case4_cache_hit_row_stream",
    "case4_cache_hit_tile",
    # 5.-7. host-result calls in between, the multi-device handle, the front end
    "case5_host_calls_in_between",
    "case6_multi_device_handle",
    "case7_front_end",
    # 8. seeded random sequences
    *(f"case8_random_seed{s}" for s in range(8)),
)


@pytest.fixture(scope="module")
def child(gpu_lib):
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "stream_ordering.py")], capture_output=True, text=True, timeout=600, env=env)
    lines = proc.stdout.strip().splitlines()
    results = {}
    for line in lines:
        if line.startswith("CASE "):
            _, name, verdict, *rest = line.split(" ", 3)
            results[name] = (verdict, rest[0] if rest else "")
    return proc, lines, results


def _tail(proc):
    return proc.stdout[-3000:] + proc.stderr[-2000:]


@pytest.mark.gpu
def test_child_ran_every_case(child):
    proc, lines, results = child
    assert lines, _tail(proc)
    last = lines[-1]
    assert last.startswith("stream ordering finished:") and f"{len(CASES)} cases, 0 failed" in last, _tail(proc)
    assert proc.returncode == 0, _tail(proc)
    assert sorted(results) == sorted(CASES), _tail(proc)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_case(child, name):
    proc, lines, results = child
    assert name in results, f"{name} did not run: {_tail(proc)}"
    verdict, detail = results[name]
    assert verdict == "PASS", f"{name}: {detail}"
    # the adversary held: every case checked at least once that the spin was still pending (a vacuous case is a FAIL of its own)
    m = re.search(r"held (\d+) ms; (\d+) pending checks", detail)
    assert m and int(m.group(2)) >= 1, detail
