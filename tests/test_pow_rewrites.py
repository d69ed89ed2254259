"""The transpiler's power rewrites through the real paths, at the arguments where a rewrite of pow goes wrong.

staging.py:_print_Pow spells the reference's pow(x, n) as a multiplication chain (inflx_ipow<n>), pow(x, n/2.0) as a chain times a
square root (inflx_hpow<n>), negative exponents as 1.0/chain and a stand-alone x**(-1/2) as 1.0/inflx_hpow<1>(x).  pow has its
own table of results at zeros of both signs, infinities and NaN (C99 F.9.4.4): pow(-0.0, 2.5) = +0, pow(-inf, 2.5) = +inf,
pow(-inf, -2.5) = +0, where the naive x*x*sqrt(x) gives -0 and NaN.  The models below have ONE power each, as a factor of the
whole potential, so that a wrong sign or class of the power is a wrong sign or class of V (a sum would hide it: -0 + y^2/7).

CPU: the host twin of the generated header (tests/host_twin.cpp) against the oracle built from the same model by every reference
compiler, on trajectory points with special coordinates and on a small grid that starts at x < 0 (NaN region; the row-broadcast
staging: the power depends on the row axis alone).  GPU: the same points and grid through sweep_on_trajectory / sweep_host for the
default build, the quick point stage with shared reciprocals, and the inline quotients -- each against the oracle, and bit for
bit against each other.  NaN pattern exact, infinities with their sign, finite values within 1e-10 (conftest.compare).
"""

import functools

import numpy as np
import pytest
import sympy as sp
from conftest import COMPILERS, compare
from host_twin import HostTwin

import oracle
from inflatox_amd import Compiler, InflationModelBuilder

R = sp.Rational
#: name -> (the power of x that multiplies the whole potential, cse)
MODELS = {
    "x^(5/2)": (lambda x: x ** R(5, 2), False),
    "x^(-5/2)": (lambda x: x ** R(-5, 2), False),
    "x^(3/2)": (lambda x: x ** R(3, 2), False),
    "x^(-9/2)": (lambda x: x ** R(-9, 2), False),
    "x^3": (lambda x: x**3, False),
    "x^(-3)": (lambda x: x**-3, False),
    "x^16": (lambda x: x**16, False),
    "exp(x^(-1/2)), cse": (lambda x: sp.exp(x ** R(-1, 2)), True),  # the stand-alone x**(-1/2) becomes a cse definition
}
HALF_POWERS = ("x^(5/2)", "x^(-5/2)", "x^(3/2)", "x^(-9/2)", "exp(x^(-1/2)), cse")
ARGS = np.array([0.7])

_X0 = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-310, -1e-310, 1e300, -1e300, 2.0, -2.0, 1e-200, 1e200]
POINTS = np.array([(a, b) for a in _X0 for b in (0.5, -0.0)])
#: starts in x < 0 (finite negative bases: NaN for the half powers); rows and columns are multiples of 0.25, so the row x = 0 and
#: the column y = 0 are met exactly.  ops::complete_analysis amplifies rounding errors of the model values where its differences
#: cancel (3 - epsilon_H, lhs - rhs), and a multiplication chain may be (N-1)/2 ulps off where pow is below one: the grid has to be
#: one on which that amplification is small, which is decided on the reference alone -- its gcc and clang builds, which differ by
#: a few roundings (contraction), agree to REFERENCE_SPREAD on it, a hundredth of the bound the values are judged by
#: (asserted in references()).
GRID = ((-1.0, 1.5, -1.0, 1.25), 10, 9)
REFERENCE_SPREAD = 1e-12


@functools.lru_cache(maxsize=None)
def model(name):
    power, cse = MODELS[name]
    x, y, a = sp.symbols("x y a", real=True)
    V = a * power(x) * (1 + y**2)
    G = [[1, 0], [0, 1 + y**2]]
    return InflationModelBuilder.new([x, y], G, V, model_name="pow_rewrite", silent=True, init_sympy_printing=False, simplify=False, assertions=False).build(), cse


@functools.lru_cache(maxsize=None)
def references(name):
    """{compiler: {(what, op): values}} of the reference's C for this model -- computed once, shared by the CPU and GPU tests."""
    m, cse = model(name)
    src, symdict = oracle.emit_c_source(m, cse=cse)
    out = {}
    for cc in COMPILERS:
        om = oracle.OracleModel(oracle.compile_c_model(src, cc=cc))
        ext, n0, n1 = GRID
        out[cc] = {("points", op): om.trajectory_sweep(op, ARGS, POINTS) for op in (oracle.OP.RAW, oracle.OP.COMPLETE)}
        out[cc].update({("grid", op): om.grid_sweep(op, ARGS, ext, n0, n1) for op in (oracle.OP.RAW, oracle.OP.COMPLETE)})
    for per_cc in out.values():
        for v in per_cc.values():
            v.setflags(write=False)
    # the condition under which 1e-10 is a statement about the rewrites and not about the conditioning of the epilogue (see GRID)
    for cc in COMPILERS[1:]:
        for key, want in out[COMPILERS[0]].items():
            if key[0] == "grid":
                compare(out[cc][key], want, REFERENCE_SPREAD, f"{name} {key}: the reference built by {cc} against {COMPILERS[0]}")
    return out, symdict


def judge(name, got, what, op, tag):
    """`got` against every reference build; where it fails, say at which point."""
    refs, _ = references(name)
    for cc in COMPILERS:
        want = refs[cc][(what, op)]
        try:
            compare(got, want, 1e-10, f"{name} {tag} {what} op {op} [{cc}]")
        except AssertionError as e:
            g, w = np.asarray(got), np.asarray(want)
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w)) | (np.isfinite(g) & np.isfinite(w))))
            where = ""
            if len(bad) and what == "points":
                i = bad[0][0]
                where = f": first at x = ({POINTS[i][0]!r}, {POINTS[i][1]!r}), value {bad[0][1:]}: got {g[tuple(bad[0])]!r}, reference {w[tuple(bad[0])]!r}"
            raise AssertionError(str(e) + where) from None


def test_the_models_contain_the_rewrites_they_are_about():
    for name, want in (("x^(5/2)", "inflx_hpow<5>("), ("x^(-5/2)", "inflx_hpow<5>("), ("x^(3/2)", "inflx_hpow<3>("), ("x^(-9/2)", "inflx_hpow<9>("), ("x^3", "inflx_ipow<3>("),
                       ("x^(-3)", "inflx_ipow<3>("), ("x^16", "inflx_ipow<16>("), ("exp(x^(-1/2)), cse", "(1.0/inflx_hpow<1>(")):  # fmt: skip
        m, cse = model(name)
        hdr = Compiler(m, silent=True, cse=cse)._generate_hip_header()
        assert want in hdr, name
    # the reference's C of the same models calls pow with the exponent spelled as in the device probe
    for name, want in (("x^(5/2)", "pow(x[0], 5.0/2.0)"), ("x^3", "pow(x[0], 3)"), ("exp(x^(-1/2)), cse", "pow(x[0], -1.0/2.0)")):
        m, cse = model(name)
        assert want in oracle.emit_c_source(m, cse=cse)[0], name


@pytest.mark.parametrize("name", list(MODELS))
def test_host_twin_equals_the_reference_at_special_points(name):
    """±0, ±inf, NaN, denormals, the far field and negative bases as the row coordinate, 0.5 and -0.0 as the column coordinate."""
    m, cse = model(name)
    comp = Compiler(m, silent=True, cse=cse)
    tw = HostTwin(comp._generate_hip_header())
    assert comp.symbol_dict == references(name)[1]
    for op_t, op_o in ((4, oracle.OP.RAW), (0, oracle.OP.COMPLETE)):
        judge(name, tw.trajectory(op_t, ARGS, POINTS), "points", op_o, "host twin")
    # the host twin's V (just found equal to the reference's) at the two arguments the half powers are about: pow's class and sign,
    # not the naive product's
    if name in HALF_POWERS:
        V = tw.trajectory(4, ARGS, POINTS)[:, 0]
        at_minus_zero, at_minus_inf = V[2], V[6]  # x0 = _X0[1], _X0[3], both with x1 = 0.5
        assert POINTS[2, 0] == 0.0 and np.signbit(POINTS[2, 0]) and POINTS[6, 0] == -np.inf and POINTS[2, 1] == POINTS[6, 1] == 0.5
        negative = "-" in name
        if name.startswith("exp"):
            assert at_minus_zero == np.inf and at_minus_inf == ARGS[0] * 1.25
        else:
            assert (at_minus_zero == np.inf if negative else (at_minus_zero == 0.0 and not np.signbit(at_minus_zero))), at_minus_zero
            assert (at_minus_inf == 0.0 and not np.signbit(at_minus_inf)) if negative else at_minus_inf == np.inf, at_minus_inf


@pytest.mark.parametrize("name", list(MODELS))
def test_host_twin_equals_the_reference_on_a_grid_from_negative_x(name):
    m, cse = model(name)
    hdr = Compiler(m, silent=True, cse=cse)._generate_hip_header()
    tw = HostTwin(hdr)
    ext, n0, n1 = GRID
    for op_t, op_o in ((4, oracle.OP.RAW), (0, oracle.OP.COMPLETE)):
        got = tw.grid(op_t, ARGS, ext, n0, n1)
        judge(name, got, "grid", op_o, "host twin")
        if name in HALF_POWERS and op_t == 4:
            assert np.isnan(got[:4, :, 0]).all() and np.isfinite(got[5:, :, 0]).all(), "the grid is meant to cover the NaN region x < 0 and the regular one"
    # staging (the power is a row value) changes no bit
    plain = HostTwin(Compiler(m, silent=True, cse=cse, staged=False)._generate_hip_header())
    assert np.array_equal(tw.grid(0, ARGS, ext, n0, n1), plain.grid(0, ARGS, ext, n0, n1), equal_nan=True)
    assert np.array_equal(tw.trajectory(0, ARGS, POINTS), plain.trajectory(0, ARGS, POINTS), equal_nan=True)


BUILDS = {"default": {}, "quick+shared": dict(hoist_reciprocals=True, share_reciprocals=True), "inline": dict(hoist_reciprocals="inline")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MODELS))
def test_gpu_builds_equal_the_reference_and_each_other(name, gpu_lib):
    """The same points through sweep_on_trajectory and the same grid through sweep_host, for the three builds of the point stage."""
    m, cse = model(name)
    results = {}
    # one build after the other: builds whose headers come out equal share a content tag, hence a cache entry, and the second is a cache hit
    artefacts = {}  # (kept: an artefact removes its file when it goes)
    for tag, kwargs in BUILDS.items():
        artefacts[tag] = Compiler(m, silent=True, cse=cse, **kwargs).compile()
        lib = gpu_lib.InflatoxDevLib(artefacts[tag].shared_object_path)
        ext, n0, n1 = GRID
        for gop, oop in ((gpu_lib.OP_RAW, oracle.OP.RAW), (gpu_lib.OP_COMPLETE, oracle.OP.COMPLETE)):
            on_points = lib.sweep_on_trajectory(gop, ARGS, POINTS)
            on_grid = lib.sweep_host(gop, ARGS, ext, n0, n1)
            results[(tag, "points", oop)], results[(tag, "grid", oop)] = on_points, on_grid
            judge(name, on_points, "points", oop, tag)
            judge(name, on_grid, "grid", oop, tag)
    for (tag, what, op), got in results.items():
        assert np.array_equal(got, results[("default", what, op)], equal_nan=True), f"{name}: build {tag} differs from the default build ({what}, op {op})"
