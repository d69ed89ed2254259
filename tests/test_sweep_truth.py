"""The sweep's model values against a truth that does not start from inflatox_amd/symbolic.py (tests/sweep_truth.py), on the CPU.

  a. the truth itself against d d V - Gamma dV with textbook connections, at 50 digits;
  b. the truth against the reference's own derivation: the 50-digit planes stored with the goldens (``g16_raw_mp``, ``g64_raw_mp``);
  c. the host twin of the sweep kernels (g++ without contraction, clang++ with ``-ffp-contract=on``) against the truth: the 24
     fuzzed models of tests/test_model_fuzz.py and four models with G_01 != 0, two of them built with ``guesses``;
  d. staged == unstaged == quick point stage, bit for bit, on the metrics with G_01 != 0;
  e. the comparison sees the defects it is for: a truth without G_01 in the inner products, a w turned round.
The figures measured in (b) and (c) are collected in profiles/sweep_truth.json (printed with -s; with INFLX_TEST_REPORT_DIR=DIR also kept in DIR/sweep_truth_cpu.json).
"""

import json
import os

import mpmath as mp
import numpy as np
import pytest
import sympy as sp
from conftest import GOLDEN_DIR, golden
from host_twin import HostTwin

import sweep_truth as st

BUILDS = (("off", "g++"), ("on", "clang++"))
RECORD = {}


def record(section, key, **figures):
    """Keep the measured figures of this run where INFLX_TEST_REPORT_DIR says (manual runs, for profiles/sweep_truth.json)."""
    RECORD.setdefault(section, {})[key] = {k: (float(f"{v:.3e}") if isinstance(v, float) else v) for k, v in figures.items()}
    out = os.environ.get("INFLX_TEST_REPORT_DIR")
    if not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, "sweep_truth_cpu.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        for sec, entries in RECORD.items():
            old.setdefault(sec, {}).update(entries)
        with open(path, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except OSError:  # figures only
        pass


# ---- a. the truth against closed forms -------------------------------------------------------------------------------------------
def _polar():
    """the polar plane of tests/test_symbolic.py with its textbook connection: Gamma[m][(i, j)]"""
    import test_symbolic as ts

    bld = ts.polar_builder()
    r = ts.r
    gamma = {(0, 1, 1): -r, (1, 0, 1): 1 / r, (1, 1, 0): 1 / r}  # Gamma^r_{theta theta} = -r, Gamma^theta_{r theta} = 1 / r
    return bld.fields, bld.metric, bld.V, gamma, ts.points((0.3, 0.1), (2.0, 3.0)), ts.PARAMS


def _half_plane():
    import test_symbolic as ts

    bld = ts.half_plane_builder()
    y = ts.y
    gamma = {(0, 0, 1): -1 / y, (0, 1, 0): -1 / y, (1, 0, 0): 1 / y, (1, 1, 1): -1 / y}  # Gamma^x_{xy}, Gamma^y_{xx}, Gamma^y_{yy}
    return bld.fields, bld.metric, bld.V, gamma, ts.points((-1.0, 0.4), (1.0, 2.5)), ts.PARAMS


@pytest.mark.parametrize("make", [_polar, _half_plane])
def test_lie_derivative_hesse_matrix_is_the_covariant_one(make):
    """H_ab = (L_X G)_ab / 2 with G X = dV against d_a d_b V - Gamma^m_ab d_m V, the connection written out from the textbook symbols
    of tests/test_symbolic.py: 40 seeded points, 50 digits, 1e-40 of the largest component at the point."""
    fields, metric, V, gamma, pts, params = make()
    ex = st.truth_expressions(fields, metric, V)
    V = sp.sympify(V)
    want = [[sp.diff(V, fields[a], fields[b]) - sum(gamma.get((m, a, b), 0) * sp.diff(V, fields[m]) for m in range(2)) for b in range(2)] for a in range(2)]
    names = sorted(params, key=str)
    f = sp.lambdify([*fields, *names], [*ex["H"][0], *ex["H"][1], *want[0], *want[1]], modules="mpmath")
    assert pts.shape == (40, 2)
    with mp.workdps(50):
        for a, b in pts:
            vals = f(mp.mpf(float(a)), mp.mpf(float(b)), *[mp.mpf(params[s]) for s in names])
            top = max(abs(v) for v in vals[4:])
            assert top > 0
            for got, ref in zip(vals[:4], vals[4:]):
                assert abs(got - ref) <= mp.mpf("1e-40") * top, (a, b, got, ref)


# ---- b. the truth against the reference's own derivation -------------------------------------------------------------------------
# the constants the stored planes were evaluated with: the float64 nearest to the 12-digit literals of the reference's C
REFERENCE_CONSTANTS = {sp.pi: float("3.14159265359"), sp.E: float("2.71828182846")}
# D5 -- the one example model whose potential contains pi -- against its stored planes: with the exact pi, and with the 12-digit one
# (ten times the worst values measured, profiles/sweep_truth.json "d5_finding")
D5_EXACT_PI_BOUND = 8.94e-10  # measured 8.94e-11 (g16), 5.35e-11 (g64)
D5_REFERENCE_PI_BOUND = 1.23e-19  # measured 5.6e-21 (g16), 1.23e-20 (g64)


def _golden_comparison(name, tag, dps=50, constants=None):
    from workloads import example_models

    spec = example_models.get(name)
    g = golden(name)
    symdict = json.load(open(os.path.join(GOLDEN_DIR, "symbols.json")))[name]["symbol_dictionary"]
    n0, n1 = (int(v) for v in g[f"{tag}_shape"])
    pts = st.grid_points(np.asarray(g[f"{tag}_extent"]).reshape(-1), n0, n1)
    guess = tuple(spec.guesses[0]) if spec.guesses else None
    if constants is not None:
        constants = {k: sp.Float(v, dps) for k, v in constants.items()}
    rows, _ = st.raw_truth(spec, symdict, g["args"], pts, guess=guess, dps=dps, constants=constants)
    return rows, st.to_float(rows).reshape(n0, n1, 5), g[f"{tag}_raw_mp"]


def _golden_figures(want, stored):
    """(share of the values compared, worst |want - stored| in units of the stored value's spacing, worst difference relative to
    max(|stored|, 1e-6 x column maximum)) over the values that are finite and non-zero in both"""
    with np.errstate(all="ignore"):
        ok = np.isfinite(stored) & np.isfinite(want) & (stored != 0)
        top = np.max(np.where(np.isfinite(stored), np.abs(stored), 0.0), axis=(0, 1), keepdims=True)
        rel = np.where(ok, np.abs(want - stored) / np.maximum(np.abs(stored), 1e-6 * top), 0.0)
        ulps = np.where(ok, np.abs(want - stored) / np.spacing(np.abs(stored)), 0.0)
    return float(ok.mean()), float(ulps.max()), float(rel.max())


@pytest.mark.parametrize("tag", ["g16", "g64"])
@pytest.mark.parametrize("name", ["hyperbolic", "angular", "egno", "doc"])
def test_truth_reproduces_the_stored_50_digit_planes(name, tag):
    """The Lie-derivative truth, at the points of the golden grids and with ``spec.guesses`` where the model has them, against the
    50-digit values of the expressions the REFERENCE's symbolic stage derived (tests/golden/make_golden.py mp_truth): equal after
    rounding to float64 (hyperbolic, angular, EGNO: within 1 ulp) resp. within 1e-13 (doc), on at least 70 % of the values."""
    _, want, stored = _golden_comparison(name, tag)
    share, ulps, rel = _golden_figures(want, stored)
    record("truth_against_stored_planes", f"{name}/{tag}", compared_share=share, worst_ulps=ulps, worst_rel=rel)
    print(f"{name}/{tag}: compared {share:.3f}, worst {ulps:.3g} ulp, {rel:.3e} relative")
    assert share >= 0.70, (name, tag, share)
    if name == "doc":
        assert rel <= 1e-13, (name, tag, rel)
    else:
        assert ulps <= 1.0, (name, tag, ulps)


def test_d5_differs_from_its_stored_planes_by_the_references_pi():
    """D5 is 9e-11 away from its stored planes where the other models are equal to the bit.  The truth does not move between 50 and
    100 digits, so the difference is not the truth's; the stored planes were evaluated with the reference's 12-digit constants
    (M_PI = 3.14159265359, off by 6.6e-14 relative: tests/golden/make_golden.py mp_truth), and D5 is the one example model with pi in
    its potential -- (2 pi)^5 in the brane tension, next to terms that cancel.  With that constant in place of pi the truth reproduces
    the stored planes like those of the other models (1.2e-20 of the column scale; with the exact pi 8.9e-11)."""
    rows50, want50, stored = _golden_comparison("d5", "g16", dps=50)
    rows100, _, _ = _golden_comparison("d5", "g16", dps=100)
    moved = mp.mpf(0)
    with np.errstate(all="ignore"):
        top = np.max(np.where(np.isfinite(stored), np.abs(stored), 0.0), axis=(0, 1)).reshape(-1)
        ok = (np.isfinite(stored) & np.isfinite(want50) & (stored != 0)).reshape(-1, 5)  # the values that are compared below
    with mp.workdps(100):
        for r50, r100, use in zip(rows50, rows100, ok):
            for k, (a, b) in enumerate(zip(r50, r100)):
                if use[k]:
                    moved = max(moved, abs(a - b) / max(abs(b), mp.mpf(1e-6 * top[k])))
    moved = float(moved)
    figures = {"truth_50_against_100_digits": moved}
    # (measured 1.7e-20: next to its singular lines D5 loses thirty of the fifty digits; that is still nine decades below the difference
    # to be explained and four below float64's rounding)
    assert moved <= 1e-18, moved
    for tag in ("g16", "g64"):
        _, want, stored = (None, want50, stored) if tag == "g16" else _golden_comparison("d5", tag)
        share, _, rel = _golden_figures(want, stored)
        _, want_ref, _ = _golden_comparison("d5", tag, constants=REFERENCE_CONSTANTS)
        share_ref, ulps_ref, rel_ref = _golden_figures(want_ref, stored)
        print(f"d5/{tag}: compared {share:.3f}; exact pi {rel:.3e}; the reference's 12-digit pi {rel_ref:.3e} ({ulps_ref:.3g} ulp)")
        figures.update({f"{tag}_compared_share": share, f"{tag}_exact_pi": rel, f"{tag}_reference_pi": rel_ref, f"{tag}_reference_pi_ulps": ulps_ref})
        assert share >= 0.70 and share_ref >= 0.70, (tag, share, share_ref)
        assert rel <= D5_EXACT_PI_BOUND, (tag, rel)
        assert rel_ref <= D5_REFERENCE_PI_BOUND, (tag, rel_ref)  # (v10 on the lines theta = k pi is a cancellation artefact of 1e-23: no ulp count there)
    record("d5_finding", "d5", **figures)


# ---- c. the host twin against the truth ------------------------------------------------------------------------------------------
MODELS_C = tuple(f"fuzz{s}" for s in range(24)) + st.NONDIAGONAL
SINGLE_OPS = {"consistency": 1, "rapidturn": 2, "epsilon_v": 3}


def _cpu_case(name):
    z = st.sweep_model(name)
    p = st.parameter_rows(name)[0]
    pts = st.grid_points(z.box, *st.GRID_CPU)
    return z, p, pts, st.truth(name, p, pts)


@pytest.mark.parametrize("name", MODELS_C)
def test_host_twin_against_the_truth(name):
    """The generated stage code, compiled for the host both ways, on a 23 x 19 grid over the model's box: every raw value within 1e-10
    of its scale of the truth (measured: 8.4e-13 at most, 3.0e-12 for a derived value -- the bound is a statement about correctness,
    not about rounding); for the models with G_01 != 0 also the six outputs, the three single quantities, the Hesse operation (v01 and
    v10 are both the truth's H(w, v)) and the basis, with equal NaN patterns."""
    z, p, pts, t = _cpu_case(name)
    n0, n1 = st.GRID_CPU
    assert np.isfinite(t.raw).all()
    for contract, cxx in BUILDS:
        twin = HostTwin(st.compiler_for(name).header, contract, cxx)
        raw = twin.grid(4, p, z.box, n0, n1).reshape(-1, 5)
        assert np.isfinite(raw).all()
        figures = {"raw": st.worst(raw, t.raw)}
        if name in st.NONDIAGONAL:
            six = twin.grid(0, p, z.box, n0, n1).reshape(-1, 6)
            figures["excused_share"], _ = st.nan_rule(six, t.six, t.radicand)
            derived = [st.worst(np.where(np.isnan(six), t.six, six), t.six)]
            for key, op in SINGLE_OPS.items():
                derived.append(st.worst(twin.grid(op, p, z.box, n0, n1).reshape(-1), t.single[key]))
            figures["derived"] = max(derived)
            assert twin.v01_is_v10
            figures["hesse"] = st.worst(twin.grid(6, p, z.box, n0, n1).reshape(-1, 4), t.hesse)
            frame = twin.basis(p, pts)
            assert np.abs(frame[:, :3] - [1.0, 0.0, 1.0]).max() <= 1e-12
            figures["basis"] = st.worst(frame[:, 3:], t.frame[:, 3:])
            figures["nan_share"] = float(np.isnan(t.six).mean())
        print(name, cxx, contract, figures)
        record("host_twin_against_truth", f"{name}/{cxx} contract={contract}", **figures)
        for key in ("raw", "derived", "hesse", "basis"):
            assert figures.get(key, 0.0) <= st.BAR, (name, cxx, key, figures[key])


# ---- d. staging changes no bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", st.NONDIAGONAL)
def test_staged_unstaged_and_quick_point_stage_are_bit_equal(name):
    z = st.sweep_model(name)
    p = st.parameter_rows(name)[0]
    staged, plain, quick = st.compiler_for(name), st.compiler_for(name, staged=False), st.compiler_for(name, hoist_reciprocals=True)
    if name == "shear":
        assert quick.stage_info["hoisted_quotients"] > 0 and staged.stage_info["hoisted_quotients"] == 0
    a, b, q = (HostTwin(c.header) for c in (staged, plain, quick))
    for op in (4, 0, 6):
        want = a.grid(op, p, z.box, 23, 37)
        assert np.array_equal(want, b.grid(op, p, z.box, 23, 37), equal_nan=True), (name, op, "staged against unstaged")
        assert np.array_equal(want, q.grid(op, p, z.box, 23, 37), equal_nan=True), (name, op, "quick point stage against the default")


# ---- e. the tests can see the defects they are for -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["skew", "shear"])
def test_a_truth_without_g01_is_far_from_the_right_one(name):
    """G_01 set to zero in the inner products and in the raising (the gradient and the Hesse matrix left alone): more than 1e-3 of the
    scale away in one of the five values at at least half of the points -- ten million times the bound of the comparisons above."""
    z, p, pts, t = _cpu_case(name)
    wrong = st.truth(name, p, pts, drop_g01=True)
    far = (np.abs(wrong.raw - t.raw) / st.scale(t.raw) > 1e-3).any(axis=1)
    print(name, "share of points where the truth without G_01 is far:", far.mean())
    assert far.mean() >= 0.5, (name, far.mean())


@pytest.mark.parametrize("name", ["skew", "shear_g"])
def test_turning_w_round_changes_the_sign_of_v10_and_nothing_else(name):
    z, p, pts, t = _cpu_case(name)
    flipped = st.truth(name, p, pts, flip_w=True)
    with mp.workdps(st.DPS):
        for r, f in zip(t.rows, flipped.rows):
            assert f[2] == -r[2] and r[2] != 0 and [f[k] for k in (0, 1, 3, 4)] == [r[k] for k in (0, 1, 3, 4)]
        for e, f in zip(t.basis, flipped.basis):
            assert [f[k] for k in (0, 2, 3, 4)] == [e[k] for k in (0, 2, 3, 4)] and (f[5], f[6]) == (-e[5], -e[6])


def test_the_guess_built_w_of_shear_really_points_the_other_way():
    """``shear`` built with ``guesses=[[1, 0]]``: v10 has the other sign at at least 10 % of the points (and is otherwise the same
    number), so a front end that ignored the guess would be caught; the ``[0, 1]`` guess on ``skew`` gives the automatic w."""
    _, p, pts, t = _cpu_case("shear")
    _, pg, _, tg = _cpu_case("shear_g")
    assert np.array_equal(p, pg)
    turned = np.sign(t.raw[:, 2]) != np.sign(tg.raw[:, 2])
    print("shear: v10 > 0 at", (t.raw[:, 2] > 0).mean(), "with the guess at", (tg.raw[:, 2] > 0).mean(), "turned at", turned.mean())
    assert turned.mean() >= 0.10
    assert np.allclose(np.abs(t.raw), np.abs(tg.raw), rtol=1e-13, atol=0.0)
