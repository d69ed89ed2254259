"""Device-resident rows on the GPU (inflatox_amd.background.solve_eom_batch_device) and the row transpose behind the host result:
bit-equality of the device result, the default host result and the forced host scatter (``EOM_HOST_SCATTER``, the path of every
earlier version) -- with ragged tiles, lanes that end inside the call, several windows of the row buffer and several passes of
lanes --, the degenerate shapes, the ordering against torch's current stream, and the refusal of a background object of the
previous layout."""

import os
import subprocess

import numpy as np
import pytest

import workloads
from background_reference import COMPLETE, ENDED, power_law_artifact, power_law_init
from test_background import VELOCITY, _points
from test_background_gpu import _hyper_batch

pytestmark = pytest.mark.gpu

ROW_FIELDS = ("states", "t", "N")
LANE_FIELDS = ("status", "last_row", "N_end")


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


def _host(sol, sl=slice(None)):
    """the slice `sl` of a device solution's trajectories on the host"""
    return type(sol)(*(getattr(sol, f)[sl].cpu().numpy() for f in ROW_FIELDS), *(getattr(sol, f)[sl] for f in LANE_FIELDS))


def _assert_same(a, b, what=""):
    for f in ROW_FIELDS:
        assert getattr(a, f).shape == getattr(b, f).shape, (what, f)
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True), (what, f)
    for f in LANE_FIELDS:
        # (N_end is NaN for a lane that did not end: the one lane array that needs equal_nan)
        assert np.array_equal(getattr(a, f), getattr(b, f), equal_nan=f == "N_end"), (what, f)


def _native_rows(lib, p, init, rows, substeps, method, max_err, dt, flags):
    """(states, t, efolds, status, last_row) of _native solve_eom as a tuple of arrays"""
    return lib.solve_eom(p, init, rows, substeps, method, max_err, dt, flags)


def _assert_same_tuples(a, b, sl=slice(None), what=""):
    for k, (u, w) in enumerate(zip(a, b)):
        assert np.array_equal(u[sl], w[sl], equal_nan=k < 3), (what, k)  # states, t, efolds may hold NaN; status and last_row may not


def _ending_batch(B):
    """initial states near the minimum of the hyperbolic potential: within 36 adaptive steps most lanes reach epsilon_H = 1, at
    different rows, and about a quarter start past it (the host build of the stepper: tests/background_reference.py)"""
    rng = np.random.default_rng(11)
    x = np.stack([rng.uniform(1.02, 3.0, B), rng.uniform(-1, 1, B)], axis=1)
    v = rng.uniform(-0.2, 0.2, (B, 2))
    return x, v


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_device_equals_host_with_ragged_tiles_and_ended_lanes(bg, solver):
    """B = 257 (four lane tiles and one lane), 19 rows (two row tiles and three rows), substeps 2, stop_at_end."""
    import torch

    spec, art = workloads.artifact_for("hyperbolic")
    x, v = _ending_batch(257)
    kw = dict(solver=solver, substeps=2, stop_at_end=True)
    want = bg.solve_eom_batch(art, spec.args, 19, x, v, **kw)
    dev = bg.solve_eom_batch_device(art, spec.args, 19, x, v, **kw)
    assert isinstance(dev, bg.EoMSolution)
    for f, shape in (("states", (257, 19, 5)), ("t", (257, 19)), ("N", (257, 19))):
        tensor = getattr(dev, f)
        assert isinstance(tensor, torch.Tensor) and tensor.dtype == torch.float64 and tuple(tensor.shape) == shape, f
        assert tensor.device == torch.device("cuda", bg._dylib(art).device)
        assert hasattr(tensor, "__dlpack__") and hasattr(tensor, "__cuda_array_interface__")
    # views of one (B, steps, 6) tensor and one (B, steps) tensor
    assert dev.states.untyped_storage().data_ptr() == dev.N.untyped_storage().data_ptr() != dev.t.untyped_storage().data_ptr()
    assert dev.states.stride() == (19 * 6, 6, 1) and dev.N.stride() == (19 * 6, 6) and dev.N.storage_offset() == 5 and dev.t.is_contiguous()
    for f in LANE_FIELDS:
        assert isinstance(getattr(dev, f), np.ndarray)
    # some lanes end inside the call: the row they end in holds a state, their later rows are NaN
    inside = (want.status == ENDED) & (want.last_row > 0) & (want.last_row < 18)
    assert inside.sum() >= 20 and (want.last_row == 0).any(), np.bincount(want.last_row)
    for k in np.flatnonzero(inside)[:20]:
        last = want.last_row[k]
        assert np.isfinite(want.states[k, : last + 1]).all() and np.isnan(want.states[k, last + 1 :]).all() and np.isnan(want.t[k, last + 1 :]).all()
    _assert_same(_host(dev), want, solver)


@pytest.mark.parametrize("name", ["hyperbolic", "egno"])
def test_both_host_paths_agree(bg, name):
    """_native solve_eom with and without EOM_HOST_SCATTER, B = 1000, 37 rows, adaptive, both steppers; EGNO is a second code object,
    whose advance kernels run one wavefront per SIMD."""
    from inflatox_amd import _native

    spec, art = workloads.artifact_for(name)
    lib = bg._dylib(art)
    if name == "hyperbolic":
        x, v = _hyper_batch(1000, seed=9)
        init = np.concatenate([x, v], axis=1)
    else:
        init = _points(name, 1000, seed=1) * np.array([1, 1, VELOCITY[name], VELOCITY[name]])
    for method in (_native.EOM_RK4, _native.EOM_RKF):
        for flags in (0, _native.EOM_STOP_AT_END):
            default = _native_rows(lib, spec.args, init, 37, 1, method, 1e-6, 0.0, flags)
            scatter = _native_rows(lib, spec.args, init, 37, 1, method, 1e-6, 0.0, flags | _native.EOM_HOST_SCATTER)
            assert default[0].shape == (1000, 37, 6) and default[1].shape == (1000, 37)
            assert np.isfinite(default[0][:, 0]).all() and (flags or np.isfinite(default[0]).mean() > 0.25)  # (not two arrays of NaN)
            _assert_same_tuples(default, scatter, what=(name, method, flags))


def test_windows_of_the_row_buffer(bg):
    """B = 100 003, 60 rows, substeps 2: the 256 MiB row buffer holds 47 rows, so the second window is rows 47..59 -- row_base > 0 and a
    ragged row tile (13 rows).  The default host result against the forced scatter on every element, and the device result against
    both on the first 64 and the last 77 lanes."""
    from inflatox_amd import _native

    spec, art = workloads.artifact_for("hyperbolic")
    B = 100_003
    assert (256 << 20) // (56 * B) == 47
    x, v = _hyper_batch(B, seed=6)
    init = np.concatenate([x, v], axis=1)
    lib = bg._dylib(art)
    default = _native_rows(lib, spec.args, init, 60, 2, _native.EOM_RKF, 1e-6, 0.0, 0)
    scatter = _native_rows(lib, spec.args, init, 60, 2, _native.EOM_RKF, 1e-6, 0.0, _native.EOM_HOST_SCATTER)
    _assert_same_tuples(default, scatter, what="default vs scatter")
    assert np.isfinite(default[0][:, 47:]).mean() > 0.5  # the second window holds states
    dev = bg.solve_eom_batch_device(art, spec.args, 60, x, v, substeps=2)
    for sl in (slice(0, 64), slice(B - 77, None)):
        got = _host(dev, sl)
        for other in (default, scatter):
            assert np.array_equal(got.states, other[0][sl][:, :, :5], equal_nan=True) and np.array_equal(got.N, other[0][sl][:, :, 5], equal_nan=True), sl
            assert np.array_equal(got.t, other[1][sl], equal_nan=True), sl
            assert np.array_equal(got.N_end, other[2][sl], equal_nan=True) and np.array_equal(got.status, other[3][sl]) and np.array_equal(got.last_row, other[4][sl])


def test_passes_of_lanes(bg):
    """B = 2^20 + 3, 3 rows, dt = 1e-3: a second pass of 3 lanes at lane_off = 2^20.  Default against forced scatter on the first five
    lanes and on the five around the boundary of the passes."""
    from inflatox_amd import _native

    spec, art = workloads.artifact_for("hyperbolic")
    B = (1 << 20) + 3
    x, v = _hyper_batch(B, seed=7)
    init = np.concatenate([x, v], axis=1)
    lib = bg._dylib(art)
    default = _native_rows(lib, spec.args, init, 3, 1, _native.EOM_RKF, 1e-6, 1e-3, 0)
    scatter = _native_rows(lib, spec.args, init, 3, 1, _native.EOM_RKF, 1e-6, 1e-3, _native.EOM_HOST_SCATTER)
    for sl in (slice(0, 5), slice((1 << 20) - 2, None)):
        _assert_same_tuples(default, scatter, sl, what=sl)
        assert np.isfinite(default[0][sl]).all()
    dev = bg.solve_eom_batch_device(art, spec.args, 3, x, v, dt=1e-3)
    for sl in (slice(0, 5), slice((1 << 20) - 2, None)):
        got = _host(dev, sl)
        assert np.array_equal(got.states, scatter[0][sl][:, :, :5]) and np.array_equal(got.t, scatter[1][sl]) and np.array_equal(got.status, scatter[3][sl])


def test_degenerate_shapes(bg):
    import torch

    spec, art = workloads.artifact_for("hyperbolic")
    x, v = _ending_batch(70)
    # steps = 1: row 0 only, no advance launch
    want = bg.solve_eom_batch(art, spec.args, 1, x, v, stop_at_end=True)
    dev = bg.solve_eom_batch_device(art, spec.args, 1, x, v, stop_at_end=True)
    assert tuple(dev.states.shape) == (70, 1, 5) and np.array_equal(want.states[:, 0, :4], np.concatenate([x, v], axis=1))
    _assert_same(_host(dev), want, "steps = 1")
    # B = 1
    want = bg.solve_eom_batch(art, spec.args, 12, x[3:4], v[3:4])
    dev = bg.solve_eom_batch_device(art, spec.args, 12, x[3:4], v[3:4])
    assert want.status[0] == COMPLETE and np.isfinite(want.states).all()
    _assert_same(_host(dev), want, "B = 1")
    # B = 0: empty tensors
    want = bg.solve_eom_batch(art, spec.args, 12, np.zeros((0, 2)), np.zeros((0, 2)))
    dev = bg.solve_eom_batch_device(art, spec.args, 12, np.zeros((0, 2)), np.zeros((0, 2)))
    assert tuple(dev.states.shape) == (0, 12, 5) and tuple(dev.t.shape) == tuple(dev.N.shape) == (0, 12) and dev.states.dtype == torch.float64 and dev.states.is_cuda
    assert dev.status.shape == dev.last_row.shape == dev.N_end.shape == (0,) and dev.status.dtype == np.int8 and dev.last_row.dtype == np.int64
    _assert_same(_host(dev), want, "B = 0")


def test_buffer_sizes_and_flags_are_checked(bg):
    import torch

    from inflatox_amd import _native

    spec, art = workloads.artifact_for("hyperbolic")
    lib = bg._dylib(art)
    x, v = _hyper_batch(9, seed=1)
    init = np.concatenate([x, v], axis=1)
    states = torch.empty((9, 5, 6), dtype=torch.float64, device=torch.device("cuda", lib.device))
    t = torch.empty((9, 5), dtype=torch.float64, device=states.device)
    args = (spec.args, init, 5, 1, _native.EOM_RKF, 1e-6, 0.0)
    with pytest.raises(_native.InflatoxShapeError, match="states buffer"):
        lib.solve_eom_device(*args, 0, states.data_ptr(), states.numel() * 8 - 1, t.data_ptr(), t.numel() * 8)
    with pytest.raises(_native.InflatoxShapeError, match="t buffer"):
        lib.solve_eom_device(*args, 0, states.data_ptr(), states.numel() * 8, t.data_ptr(), t.numel() * 8 - 8)
    for flags in (_native.EOM_FINAL_ONLY, _native.EOM_HOST_SCATTER, 16):
        with pytest.raises(ValueError):
            lib.solve_eom_device(*args, flags, states.data_ptr(), states.numel() * 8, t.data_ptr(), t.numel() * 8)
    # the handle's own stream (stream = 0), t not wanted
    states.fill_(-7.0)
    n_end, status, last_row = lib.solve_eom_device(*args, 0, states.data_ptr(), states.numel() * 8, 0, 0)
    want = lib.solve_eom(*args, 0)
    assert np.array_equal(states.cpu().numpy(), want[0], equal_nan=True) and np.array_equal(status, want[3]) and np.array_equal(last_row, want[4])


def test_stream_order(bg):
    """A reduction on torch's current stream right after the call, without a synchronise, sees the complete result; a second call
    right after the first returns equal tensors."""
    import torch

    spec, art = workloads.artifact_for("hyperbolic")
    x, v = _hyper_batch(5000, seed=12)
    first = bg.solve_eom_batch_device(art, spec.args, 33, x, v)
    early = (torch.nansum(first.states), torch.nansum(first.t), torch.nansum(first.N), torch.isnan(first.states).sum())
    second = bg.solve_eom_batch_device(art, spec.args, 33, x, v)
    torch.cuda.synchronize()
    late = (torch.nansum(first.states), torch.nansum(first.t), torch.nansum(first.N), torch.isnan(first.states).sum())
    for a, b in zip(early, late):
        assert a.item() == b.item(), (early, late)
    assert np.isfinite(early[0].item()) and early[0].item() != 0.0
    assert first.states.data_ptr() != second.states.data_ptr()
    _assert_same(_host(first), _host(second), "second call")
    _assert_same(_host(first), bg.solve_eom_batch(art, spec.args, 33, x, v), "host")


def test_background_object_of_layout_4_is_refused():
    """A background object of the previous layout version (INFLX_BG_ABI = 4: no transpose kernel) is refused."""
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".background"
    hdr, eom_hdr = stale + ".model.h", stale + ".eom.h"
    try:
        for path, text in ((hdr, header_text), (eom_hdr, art.eom_header_text())):
            with open(path, "w") as fh:
                fh.write(text)
        cmd = [hipcc_path(), *options, "-DINFLX_BG_ABI_VERSION=4", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', os.path.join(_CSRC, "inflx_background_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        init = np.array([power_law_init()])
        with pytest.raises(SystemError, match="does not belong"):
            lib.solve_eom(p, init, 5, 1, _native.EOM_RKF, 1e-6, 0.0, 0)
        lib.close()
    finally:
        for path in (stale, hdr, eom_hdr):
            if os.path.exists(path):
                os.remove(path)
