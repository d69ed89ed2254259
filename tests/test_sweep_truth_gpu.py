"""The sweep on the GPU against a truth that does not start from inflatox_amd/symbolic.py (tests/sweep_truth.py), on metrics with
G_01 != 0: ``skew``, ``shear`` (cse) and ``shear_g`` (``shear`` built with ``guesses=[[1, 0]]``).

The grid is 33 x 257 over the model's box -- one full and one ragged row tile, one full and one ragged column tile of the tile
kernels -- with three parameter rows in one call.  The truth is taken at a seeded sample of 400 grid points plus the four corners,
rows 31 and 32 and columns 255 and 256 (first parameter row), and at 100 points for the other two rows.  Two bounds hold for every
comparison: 1e-10 of the value's scale (the project's parity bar, literally), and FACTOR times what the host twin of the same stage
code (clang++, ``-ffp-contract=on``: the kernels' contraction rule, glibc instead of OCML) measures at the same points, floor 1e-13.
The measured figures are collected in profiles/sweep_truth.json (printed with -s; with INFLX_TEST_REPORT_DIR=DIR also kept in DIR/sweep_truth_gpu.json).
"""

import json
import os

import numpy as np
import pytest
from conftest import generalised_al
from host_twin import HostTwin

import sweep_truth as st

pytestmark = pytest.mark.gpu

N0, N1 = st.GRID_GPU
FACTOR = 4.0  # the pointwise factor of test_gpu_is_as_close_to_the_50_digit_truth_as_the_reference
TWIN_FLOOR = 1e-13
RECORD = {}


def record(name, **figures):
    RECORD.setdefault(name, {}).update({k: (float(f"{v:.3e}") if isinstance(v, float) else v) for k, v in figures.items()})
    out = os.environ.get("INFLX_TEST_REPORT_DIR")  # (manual runs: keeps the figures, for profiles/sweep_truth.json)
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "sweep_truth_gpu.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        for key, entries in RECORD.items():
            old.setdefault(key, {}).update(entries)
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except OSError:  # figures only
        pass


class Case:
    """A model's artefact, handle, host twin, sample and truths: built once per module and shared by its tests."""

    def __init__(self, name, gpu_lib):
        self.name, self.gpu = name, gpu_lib
        self.z = st.sweep_model(name)
        self.art = st.device_artifact(name)
        self.lib = gpu_lib.InflatoxDevLib(self.art.shared_object_path)
        self.twin = HostTwin(st.compiler_for(name).header, "on", "clang++")
        self.rows = st.parameter_rows(name)
        self.ss = np.array([[self.z.box[0], self.z.box[1]], [self.z.box[2], self.z.box[3]]])
        pts = st.grid_points(self.z.box, N0, N1)
        sample = st.gpu_sample()
        # (parameter row, flat grid indices, points, truth): the whole sample for the first row, its first 100 points for the others
        self.parts = []
        for q in range(3):
            idx = sample if q == 0 else sample[:100]
            self.parts.append((q, idx, pts[idx], st.truth(name, self.rows[q], pts[idx])))

    def against_truth(self, what, got, pick, twin_op, nan_rule=False):
        """``got``: (3, N0 * N1[, k]) of the GPU; ``pick(truth)`` the truth's array; ``twin_op`` the host twin's operation.  Returns
        (worst GPU error, worst twin error, excused share) over the three parameter rows, after asserting both bounds."""
        worst_gpu = worst_twin = 0.0
        excused = total = 0
        for q, idx, pts, t in self.parts:
            want = pick(t)
            mine, twin = got[q][idx], self.twin.trajectory(twin_op, self.rows[q], pts)
            if nan_rule:
                share, differ = st.nan_rule(mine, want, t.radicand, cap=1.0)
                st.nan_rule(twin, want, t.radicand, cap=1.0)
                excused, total = excused + int(differ.sum()), total + differ.size
                mine, twin = np.where(np.isnan(mine), want, mine), np.where(np.isnan(twin), want, twin)
            else:
                assert np.array_equal(np.isnan(mine), np.isnan(want)), (self.name, what, q)
            sc = st.scale(want)
            worst_gpu, worst_twin = max(worst_gpu, st.worst(mine, want, sc)), max(worst_twin, st.worst(twin, want, sc))
        share = excused / total if total else 0.0
        ratio = worst_gpu / max(worst_twin, TWIN_FLOOR)
        print(f"{self.name}/{what}: GPU {worst_gpu:.3e}, host twin {worst_twin:.3e}, ratio {ratio:.2f}, excused {share:.4f}")
        record(self.name, **{f"{what}_gpu": worst_gpu, f"{what}_twin": worst_twin, f"{what}_gpu_to_twin": ratio, f"{what}_excused_share": share})
        assert share <= 0.005, (self.name, what, share)
        assert worst_gpu <= st.BAR, (self.name, what, worst_gpu)
        assert worst_gpu <= FACTOR * max(worst_twin, TWIN_FLOOR), (self.name, what, worst_gpu, worst_twin)
        return worst_gpu, worst_twin, share


_CASES = {}


@pytest.fixture(scope="module", params=st.GPU_MODELS)
def case(request, gpu_lib):
    name = request.param
    if name not in _CASES:
        _CASES[name] = Case(name, gpu_lib)
    return _CASES[name]


def test_these_models_take_the_tile_path(case):
    gpu = case.gpu
    assert case.art.stage_info["out_mask"] & 3 == 3 and case.art.stage_info["v01_is_v10"]
    for op in (gpu.OP_COMPLETE, gpu.OP_RAW, gpu.OP_HESSE, gpu.OP_EPSILON_V):
        assert case.lib.sweep_plan(op, 3, N1, N0)["path"] == "tile", (case.name, op)


# ---- a. raw values ---------------------------------------------------------------------------------------------------------------
def test_raw_values_against_the_truth(case):
    """V, v00, v10, v11, |dV|^2 of three parameter rows in one call: all 3 x 5 x 33 x 257 values finite, and at the sampled points
    within both bounds of the truth."""
    got = case.lib.sweep_host(case.gpu.OP_RAW, case.rows, case.ss, N0, N1)
    assert got.shape == (3, N0, N1, 5) and np.isfinite(got).all()
    case.against_truth("raw", got.reshape(3, -1, 5), lambda t: t.raw, 4)


# ---- b. everything derived -------------------------------------------------------------------------------------------------------
def test_six_outputs_against_the_mpmath_epilogue_of_the_truth(case):
    """consistency, eps_V, eps_H, eta, delta, omega against tests/tolerance.py's epilogue restated in mpmath and applied to the 50-digit
    raw values: NaN patterns equal (omega and eta are NaN where omega's radicand is negative: 5 to 8 % of the values), except where
    the radicand is within 1e-9 of zero, at most 0.5 % of the values."""
    got = case.lib.sweep_host(case.gpu.OP_COMPLETE, case.rows, case.ss, N0, N1)
    assert got.shape == (3, N0, N1, 6)
    case.against_truth("six", got.reshape(3, -1, 6), lambda t: t.six, 0, nan_rule=True)


@pytest.mark.parametrize("key,op_name,twin_op", [("consistency", "OP_CONSISTENCY", 1), ("rapidturn", "OP_RAPIDTURN", 2), ("epsilon_v", "OP_EPSILON_V", 3)])
def test_single_quantity_sweeps_against_the_truth(case, key, op_name, twin_op):
    got = case.lib.sweep_host(getattr(case.gpu, op_name), case.rows, case.ss, N0, N1)
    assert got.shape == (3, N0, N1)
    case.against_truth(key, got.reshape(3, -1), lambda t: t.single[key], twin_op)


def test_hesse_operation_against_the_truth(case):
    """The four planes of ``INFLX_OP_HESSE``: v01 == v10, both the truth's H(w, v)."""
    gpu = case.gpu
    got = case.lib.sweep_host(gpu.OP_HESSE, case.rows, case.ss, N0, N1)
    assert got.shape == (3, N0, N1, 4) and np.isfinite(got).all()
    assert np.array_equal(got[..., 1], got[..., 2])
    raw = case.lib.sweep_host(gpu.OP_RAW, case.rows, case.ss, N0, N1)
    assert np.array_equal(got[..., [0, 2, 3]], raw[..., 1:4])
    case.against_truth("hesse", got.reshape(3, -1, 4), lambda t: t.hesse, 6)


# ---- c. basis and front end ------------------------------------------------------------------------------------------------------
def test_basis_on_points_against_the_truth(case):
    """v and w at 200 sample points: orthonormal in the FULL metric to 1e-12, components within 1e-10 of their scale of the truth's --
    for ``shear_g`` those of the w built from the guess, which points the other way at 45 % of the points."""
    q, idx, pts, t = case.parts[0]
    pts, frame = pts[:200], t.frame[:200]
    got = case.lib.basis_on_points(case.rows[0], pts)
    assert np.abs(got[:, :3] - [1.0, 0.0, 1.0]).max() <= 1e-12
    err = st.worst(got[:, 3:], frame[:, 3:])
    record(case.name, basis_gpu=err, basis_twin=st.worst(case.twin.basis(case.rows[0], pts)[:, 3:], frame[:, 3:]))
    assert err <= st.BAR, (case.name, err)
    if case.name == "shear_g":
        plain = st.truth("shear", case.rows[0], case.parts[0][2]).frame[:200]
        turned = np.sign(plain[:, 5]) != np.sign(frame[:, 5])
        assert turned.mean() >= 0.10 and np.array_equal(np.sign(got[:, 5]), np.sign(frame[:, 5]))


def test_front_end_on_a_nondiagonal_metric(case):
    """``validate_basis_on_domain`` passes over the box; ``flag_quantum_dif`` is (v^0 <= a) & (v^1 <= a) of the truth's v (a component
    within 1e-9 of a excused, at most 0.2 % of the points); ``complete_analysis`` and the array helpers return the C-ABI sweeps' bits
    and the two point calls the truth."""
    gpu = case.gpu
    al = generalised_al(case.art)
    p = case.rows[0]
    x0a, x0b, x1a, x1b = case.z.box
    al.validate_basis_on_domain(p, [x0a, x1a], [x0b, x1b], N=[16, 12])
    q, idx, pts, t = case.parts[0]
    excused = 0
    for accuracy in (1e-3, 0.5, 0.9):
        got = al.flag_quantum_dif(p, x0a, x0b, x1a, x1b, N0, N1, progress=False, accuracy=accuracy)
        assert got.dtype == np.bool_ and got.shape == (N0, N1)
        v = t.frame[:, 3:5]
        want = (v[:, 0] <= accuracy) & (v[:, 1] <= accuracy)
        differ = got.reshape(-1)[idx] != want
        assert (np.abs(v[differ] - accuracy) <= 1e-9).any(axis=1).all(), (case.name, accuracy, int(differ.sum()))
        assert differ.sum() <= 0.002 * idx.size, (case.name, accuracy, int(differ.sum()))
        excused += int(differ.sum())
    record(case.name, flag_excused_points=excused)
    six = np.stack(al.complete_analysis(p, x0a, x0b, x1a, x1b, N0, N1, progress=False), axis=-1)
    assert np.array_equal(six, case.lib.sweep_host(gpu.OP_COMPLETE, p, case.ss, N0, N1), equal_nan=True)
    raw = case.lib.sweep_host(gpu.OP_RAW, p, case.ss, N0, N1)
    assert np.array_equal(al.calc_V_array(p, [x0a, x1a], [x0b, x1b], [N0, N1]), raw[..., 0])
    H = al.calc_H_array(p, x0a, x0b, x1a, x1b, [N0, N1])
    assert H.shape == (2, 2, N0, N1)
    for (a, b), k in (((0, 0), 1), ((0, 1), 2), ((1, 0), 2), ((1, 1), 3)):
        assert np.array_equal(H[a, b], raw[..., k]), (case.name, a, b)
    sc = st.scale(t.raw)
    for k in (0, 7, idx.size - 1):  # a sampled point, another, and one on the last column
        assert abs(al.calc_V(pts[k], p) - t.raw[k, 0]) <= st.BAR * sc[k, 0]
        Hx = al.calc_H(pts[k], p)
        assert Hx.shape == (2, 2) and (np.abs(Hx.reshape(-1) - t.hesse[k]) <= st.BAR * sc[k, [1, 2, 2, 3]]).all(), (case.name, k)


# ---- d. quick point stage and geometry -------------------------------------------------------------------------------------------
def test_quick_point_stage_equals_the_default_build(case):
    """``Compiler(hoist_reciprocals=True)`` on a metric whose inverse carries a determinant: the same bits as the default build."""
    gpu = case.gpu
    quick = st.device_artifact(case.name, hoist_reciprocals=True)
    if case.name.startswith("shear"):
        assert quick.stage_info["hoisted_quotients"] > 0 and case.art.stage_info["hoisted_quotients"] == 0
    lib_q = gpu.InflatoxDevLib(quick.shared_object_path)
    for n0, n1 in ((N0, N1), (45, 333)):
        for op in (gpu.OP_COMPLETE, gpu.OP_RAW):
            a = case.lib.sweep_host(op, case.rows, case.ss, n0, n1)
            assert np.array_equal(a, lib_q.sweep_host(op, case.rows, case.ss, n0, n1), equal_nan=True), (case.name, op, n0, n1)
    lib_q.close()


def test_sweep_geometry_equals_point_evaluation(case):
    """Six seeded cases of the property of test_geometry_fuzz_sweeps_equal_point_evaluation: element [p, i, j] of a sweep with a row
    range, either layout and one to three parameter rows is bit for bit what the on-trajectory kernel computes at that point; the
    last case goes through ``sweep_device`` on a torch stream."""
    import torch

    gpu, lib = case.gpu, case.lib
    rng = np.random.default_rng(2025 + sum(map(ord, case.name)))
    shapes = [(1, 1), (1, 257), (300, 1), (33, 255), (31, 513), (int(rng.integers(2, 200)), int(rng.integers(2, 900)))]
    ops = [(gpu.OP_COMPLETE, 6), (gpu.OP_RAW, 5), (gpu.OP_HESSE, 4), (gpu.OP_CONSISTENCY, 1)]
    x0a, x0b, x1a, x1b = case.z.box
    for k, (n0, n1) in enumerate(shapes):
        P = 1 + k % 3
        op, width = ops[k % len(ops)]
        layout = gpu.LAYOUT_SOA if k % 2 else gpu.LAYOUT_AOS
        rb = int(rng.integers(0, n0))
        rc = int(rng.integers(1, n0 - rb + 1))
        xs0 = np.arange(rb, rb + rc, dtype=np.float64) * ((x0b - x0a) / n0) + x0a
        xs1 = np.arange(n1, dtype=np.float64) * ((x1b - x1a) / n1) + x1a
        pts = np.stack(np.meshgrid(xs0, xs1, indexing="ij"), axis=-1).reshape(-1, 2)
        want = np.stack([lib.sweep_on_trajectory(op, case.rows[q], pts).reshape(rc, n1, width) for q in range(P)])
        if layout == gpu.LAYOUT_SOA:
            want = np.moveaxis(want, -1, 1)
        what = (case.name, k, n0, n1, P, op, layout, rb, rc)
        if k < len(shapes) - 1:
            got = lib.sweep_host(op, case.rows[:P], case.ss, n0, n1, row_begin=rb, row_count=rc, layout=layout)
            assert got.size == want.size and np.array_equal(got.reshape(want.shape), want, equal_nan=True), what
        else:
            stream = torch.cuda.Stream()
            out = torch.full((want.size,), -7.0, dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            lib.sweep_device(op, case.rows[:P], out.data_ptr(), out.numel() * 8, case.ss, n0, n1, row_begin=rb, row_count=rc, layout=layout, stream=stream.cuda_stream)
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().reshape(want.shape), want, equal_nan=True), what
