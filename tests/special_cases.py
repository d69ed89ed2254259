"""One table of edge cases for csrc/inflx_sf.h, its mpmath truth and its verdict -- TEST INFRASTRUCTURE, shared by
tests/test_special_edges.py (the header built for the host, tests/sf_host.cpp) and tests/test_special_edges_gpu.py (the header
inside a gfx950 program, tests/sf_probe.hip).

Families (``Case.family``):

  seams   every argument at which a function changes its branch -- Chebyshev ranges, recurrence directions, quadrature steps,
          series against asymptotic or transformed forms, the leading-term formula for small arguments -- at the seam itself,
          1, 2, 8, 64 ulp and an eighth of it either side (one side only where the seam is the edge of the domain);
  range   the arguments and orders of tests/test_special_functions.py (1e-100 ... 1e5, orders up to 150.1), so that they run
          on the device as well;
  tiny    1e-20 down to the smallest subnormal;
  limits  exact values at 0, overflow to +inf and underflow to 0, sign symmetries and negative orders bit for bit;
  status  what the status word holds after a group of calls: 0 inside the domain and for NaN arguments, INFLX_SF_EDOM outside,
          INFLX_SF_EDECLINED for a refusal.

Every case is judged by ``judge``; how (``Verdict.rule``):

  budget     |result - truth| within the budget of tests/test_special_functions.py / tests/test_special_gpu.py
  exact      the result equals a given value (0, 1, +inf) / is NaN (``nan``) / has the bits of +-another case's result (``mirror``)
  range      |truth| outside [1e-300, 1e300]: no NaN; an infinite result has the truth's sign; a result of normal size has the
             truth's sign and lies beyond 1e+-290 on the truth's side
  subnormal  the ARGUMENT is subnormal: no NaN, an infinite result has the truth's sign
  declined   NaN with the group's status word INFLX_SF_EDECLINED -- open to cases marked ``decline_ok`` only (none is: the
             real-order Y and K below 1e-300, for which the issue kept that door open, are computed)

The 1e+-290 of the ``range`` rule: the truth lies beyond 1e+-300 and every function here is right to far better than a factor of
1e10 wherever it returns a number of normal size.
"""

from __future__ import annotations

import ctypes as C
import math
import struct
from collections import Counter

import numpy as np

from oracle import special

DP = C.POINTER(C.c_double)
DBL_MIN = 2.2250738585072014e-308
FUNCTIONS = ["Jn", "Yn", "In", "Kn", "jl", "yl", "Jnu", "Ynu", "Inu", "Knu", "0F1", "1F1", "2F1", "2F0"]
FID = {name: k for k, name in enumerate(FUNCTIONS)}
INTEGER, REAL = FUNCTIONS[:6], FUNCTIONS[6:10]
EDOM, EDECLINED = 1, 2
FAMILIES = ["seams", "range", "tiny", "limits", "status"]
TINY_X = [1e-20, 1e-40, 1e-52, 1e-60, 1e-70, 1e-100, 1e-150, 1e-200, 1e-300, DBL_MIN, 1e-310, 1e-323, 5e-324]
ULPS = (0, 1, 2, 8, 64)


class Case:
    __slots__ = ("fn", "n", "p", "x", "group", "family", "check", "expect", "mirror", "decline_ok")

    def __init__(self, fn, n, p, x, group, family, check="budget", expect=None, mirror=None):
        self.fn, self.n, self.p, self.x, self.group, self.family = fn, int(n), tuple(float(v) for v in p) + (0.0,) * (3 - len(p)), float(x), group, family
        self.check, self.expect, self.mirror, self.decline_ok = check, expect, mirror, False

    def __repr__(self):
        args = {"I": f"{self.n}", "R": f"{self.p[0]!r}", "0": f"{self.p[0]!r}", "1": f"{self.p[0]!r}, {self.p[1]!r}", "2": ", ".join(repr(v) for v in (self.p if self.fn == "2F1" else self.p[:2]))}
        key = "I" if self.fn in INTEGER else "R" if self.fn in REAL else self.fn[0]
        return f"{self.fn}({args[key]}; {self.x!r} = {self.x.hex()})"


class Group:
    __slots__ = ("family", "label", "status")

    def __init__(self, family, label, status):
        self.family, self.label, self.status = family, label, status


class Table:
    def __init__(self):
        self.cases: list[Case] = []
        self.groups: list[Group] = []

    def group(self, family, label, status=0):
        self.groups.append(Group(family, label, status))
        return len(self.groups) - 1

    def add(self, fn, order, x, group, **kw):
        """``order``: the integer order, the real order, or the tuple of hypergeometric parameters"""
        n, p = (order, ()) if fn in INTEGER else (0, (order,)) if fn in REAL else (0, tuple(order))
        self.cases.append(Case(fn, n, p, x, group, self.groups[group].family, **kw))
        return len(self.cases) - 1

    def counts(self):
        return dict(Counter(c.family for c in self.cases))


def step(x, k):
    """x moved by k ulp (towards +inf for k > 0)"""
    for _ in range(abs(k)):
        x = math.nextafter(x, math.inf if k > 0 else -math.inf)
    return x


def around(x, below=True, above=True):
    """the seam and 1, 2, 8, 64 ulp either side; and an eighth of it either side -- a seam that has MOVED (a branch used beyond
    the range it was fitted or is stable for) shows there, not within a few ulp of where it should be"""
    ks = [k for k in ULPS] + [-k for k in ULPS if k]
    near = {step(x, k) for k in ks if (k >= 0 or below) and (k <= 0 or above)}
    far = {x + d for d in (-abs(x) / 8, abs(x) / 8) if (d >= 0 or below) and (d <= 0 or above)}
    return sorted(near | far)


# ---- the host twin ----------------------------------------------------------------------------------------------------------
def host_call(lib, case):
    x, out = np.array([case.x]), np.zeros(1)
    xp, op = x.ctypes.data_as(DP), out.ctypes.data_as(DP)
    if case.fn in INTEGER:
        getattr(lib, f"sf_{case.fn}")(C.c_int(case.n), xp, 1, op)
    else:
        k = 1 if case.fn in REAL else {"0F1": 1, "1F1": 2, "2F1": 3, "2F0": 2}[case.fn]
        getattr(lib, f"sf_{case.fn}")(*[C.c_double(v) for v in case.p[:k]], xp, 1, op)
    return out[0]


def run_on_host(lib, table):
    """(results, [(status word after the group, status word on the next read)]) -- the shape of the device probe's output"""
    lib.sf_status_take.restype = C.c_uint
    got = np.zeros(len(table.cases))
    by_group = [[] for _ in table.groups]
    for i, c in enumerate(table.cases):
        by_group[c.group].append(i)
    status = []
    for members in by_group:
        lib.sf_status_take()
        for i in members:
            got[i] = host_call(lib, table.cases[i])
        status.append((lib.sf_status_take(), lib.sf_status_take()))
    return got, status


def two_f_zero_seam(lib, a, b):
    """(x_in, x_out): adjacent doubles, x_in the argument of largest magnitude at which 2F0(a, b; x) still is answered from the
    asymptotic series, x_out the next one beyond it; found by bisection on the host twin.  None where there is no such seam."""
    lib.sf_2F0_asymptotic_accepts.restype = C.c_int
    accepts = lambda x: bool(lib.sf_2F0_asymptotic_accepts(C.c_double(a), C.c_double(b), C.c_double(x)))
    lo, hi = -1e-9, -1e6
    if not accepts(lo) or accepts(hi):
        return None
    to_bits = lambda v: struct.unpack("<q", struct.pack("<d", -v))[0]
    from_bits = lambda k: -struct.unpack("<d", struct.pack("<q", k))[0]
    klo, khi = to_bits(lo), to_bits(hi)
    while khi - klo > 1:
        mid = (klo + khi) // 2
        if accepts(from_bits(mid)):
            klo = mid
        else:
            khi = mid
    return from_bits(klo), from_bits(khi)


# ---- the table --------------------------------------------------------------------------------------------------------------
SEAM_REAL_ORDERS = [0.0, 0.25, 1.0, 2.3, 7.5, 20.0, 33.3]
SEAM_0F1 = [(0.5,), (1.5,), (3.7,), (25.5,), (-0.5,), (-2.3,)]
SEAM_1F1 = [(0.5, 1.5), (-0.5, 1.0), (4.2, -1.5), (12.5, 3.0), (-11.3, 4.0), (2.7, 2.2)]
SEAM_2F1 = [(0.5, 0.5, 1.0), (1.0, 1.0, 2.0), (-0.5, 1.5, 2.5), (-3.0, 2.0, 1.5), (0.3, 0.7, -1.5), (2.0, 2.0, 4.5), (3.3, -1.2, 2.1), (2.3, 1.7, 1.0), (0.25, 0.6, 1.35)]
SEAM_2F0 = [(0.5, 0.5), (1.0, 2.0), (2.5, -1.5), (7.5, 2.0), (35.0, -7.5), (-2.0, 3.3), (0.3, 3.7)]  # (-2, 3.3) terminates: no seam


def _seams(t, lib):
    g = t.group("seams", "branch seams")
    for fn, n, seams in [("Jn", 0, [1e-4, 4.0]), ("Jn", 1, [4.0]), ("Yn", 0, [4.0]), ("Yn", 1, [4.0]), ("In", 0, [1e-4, 3.0, 8.0]), ("In", 1, [3.0, 8.0]),
                         ("Kn", 0, [2.0, 8.0]), ("Kn", 1, [2.0, 8.0]), ("Jn", 2, [2.0]), ("Jn", 5, [5.0]), ("Jn", 20, [20.0]), ("Yn", 3, [4.0]), ("Yn", 20, [4.0])]:
        for s in seams:
            for x in around(s):
                t.add(fn, n, x, g)
    for fn in ("In", "Kn"):  # through exp(x) K_0, exp(x) K_1 resp. K_0, K_1: ranges meeting at 2 and 8
        for n in (2, 4, 20):
            for s in (2.0, 8.0):
                for x in around(s):
                    t.add(fn, n, x, g)
    for l, s in ((0, 3.0), (1, 5.0), (2, 7.0)):
        for x in around(math.sqrt(s)):
            t.add("jl", l, x, g)
    for l in (3, 6, 20):
        for s in (math.sqrt(2.0 * l + 3.0), float(l)):
            for x in around(s):
                t.add("jl", l, x, g)
    for l in (4, 20):
        for x in around(1.0):
            t.add("yl", l, x, g)
    for fn in REAL:
        for nu in SEAM_REAL_ORDERS:
            seams = [9.0, 1e-8 * math.sqrt(nu + 1.0)] + ([(0.35 / 0.15) ** 2] if fn in ("Jnu", "Ynu") else []) + ([nu] if nu > 0 else [])
            for s in seams:
                for x in around(s):
                    t.add(fn, nu, x, g)
    for c in SEAM_0F1:
        for x in around(-400.0):
            t.add("0F1", c, x, g)
    for ab in SEAM_1F1:
        for s in (-30.0, 30.0):
            for x in around(s):
                t.add("1F1", ab, x, g)
    for abc in SEAM_2F1:
        xs = around(-1.0, below=False) + around(-0.5) + around(0.5) + around(0.9) + [step(1.0, -k) for k in (1, 2, 64)]
        for x in xs:
            if -1.0 <= x < 1.0:  # (an eighth above 0.9 is outside the domain)
                t.add("2F1", abc, x, g)
    for ab in SEAM_2F0:
        if any(v < 0 and v == math.floor(v) for v in ab):
            continue  # a terminating series is summed exactly: the asymptotic series is never asked
        pair = two_f_zero_seam(lib, *ab)
        if pair is not None:
            for x in pair:
                t.add("2F0", ab, x, g)


REAL_TINY = [("Ynu", 0.0, 1e-160), ("Ynu", 0.0, 1e-250), ("Ynu", 0.5, 1e-200), ("Ynu", 0.25, 1e-300), ("Jnu", 0.0, 1e-200), ("Jnu", 0.5, 1e-160), ("Ynu", 1.5, 1e-160)]


def _range(t):
    """The argument lists of tests/test_special_functions.py (its generators and seeds restated: they live inside its tests)."""
    from test_special_functions import REAL_ORDERS, points

    g = t.group("range", "the host suite's range")
    x = points()
    for kind in "JYIKjy":
        for order in (0, 1, 2, 3, 7, 20):
            for xi in x[x < 300] if kind in "IK" else x:
                t.add(kind + ("l" if kind in "jy" else "n"), order, xi, g)
    rng = np.random.default_rng(3)
    xs = np.concatenate([10.0 ** rng.uniform(-12, 0, 12), rng.uniform(0, 4, 15), rng.uniform(4, 60, 25), rng.uniform(60, 400, 8), [1e-100, 1e3, 1e5]])
    for kind in "JYIK":
        for nu in REAL_ORDERS:
            for xi in xs[xs < 300] if kind in "IK" else xs:
                t.add(kind + "nu", nu, xi, g)
    for fn, nu, xi in REAL_TINY:
        t.add(fn, nu, xi, g)
    rng = np.random.default_rng(31)
    x = np.concatenate([rng.uniform(-30, 30, 25), rng.uniform(-300, 300, 15), rng.uniform(-1, 1, 6), [0.0, 1e-8, -1e-8, 600.0, -600.0]])
    params = [(0.5, 1.5), (1.0, 2.0), (2.5, 0.7), (-0.5, 1.0), (-3.0, 2.0), (-2.7, 1.3), (4.2, -1.5), (0.1, 10.0), (-4.5, -2.5), (12.5, 3.0), (-11.3, 4.0), (20.0, 21.5)]
    params += [(float(rng.uniform(-8, 8)), float(rng.uniform(-8, 8))) for _ in range(6)]
    for ab in params:
        for xi in x:
            t.add("1F1", ab, xi, g)
    rng = np.random.default_rng(37)
    x = np.concatenate([rng.uniform(-1, 1, 30), rng.uniform(0.9, 0.997, 8), [-1.0, -0.999, -0.5, 0.5, 0.75, 0.9, 0.95, 0.99, 0.997, 1e-9]])
    params = [(0.5, 1.0, 1.5), (1.0, 1.0, 2.0), (0.5, 0.5, 1.0), (2.0, 3.0, 4.0), (-0.5, 1.5, 2.5), (-3.0, 2.0, 1.5), (1.5, -2.0, 0.5), (0.3, 0.7, -1.5)]
    params += [(2.0, 2.0, 4.5), (0.25, 0.75, 1.0), (3.3, -1.2, 2.1), (6.5, -4.2, 1.1), (0.1, 0.2, 7.3)] + [tuple(float(v) for v in rng.uniform(-5, 5, 3)) for _ in range(8)]
    for abc in params:
        for xi in x:
            t.add("2F1", abc, xi, g)
    for abc in [(0.5, 0.5, 1.0), (1.0, 1.0, 2.0), (2.0, 3.0, 4.0), (1.5, 2.5, 6.0), (-0.5, 0.5, 1.0), (3.5, 2.5, 2.0), (1.2, -0.7, -1.5)]:  # c - a - b an integer
        for xi in (0.95, 0.999, 0.999999, 1 - 1e-12):
            t.add("2F1", abc, xi, g)
    rng = np.random.default_rng(41)
    x = -np.concatenate([10.0 ** rng.uniform(-4, 4, 20), [1e-3, 0.02, 0.03, 0.05, 0.1, 0.3, 1.0, 3.0, 10.0, 100.0]])
    params = [(0.5, 0.5), (1.0, 2.0), (2.5, -1.5), (0.3, 3.7), (4.0, 0.2), (7.5, 2.0), (20.0, 3.0), (35.0, -7.5), (-2.0, 3.3), (-3.0, -4.0), (1.0, -0.5)]
    params += [(float(rng.uniform(0.25, 12)), float(rng.uniform(-6, 12))) for _ in range(8)]
    for ab in params:
        for xi in x:
            t.add("2F0", ab, xi, g)


def _tiny(t):
    g = t.group("tiny", "tiny arguments")
    for x in TINY_X:
        for fn in ("Jn", "In"):
            for n in (1, 2, 4, 5, 20):
                t.add(fn, n, x, g)
        for l in (1, 3, 6, 20):
            t.add("jl", l, x, g)
        for fn in ("Yn", "Kn", "yl"):
            for n in (0, 1, 2, 3):
                t.add(fn, n, x, g)
        for fn in REAL:
            for nu in (0.0, 0.5, 2.5, 5.0, 20.0):
                t.add(fn, nu, x, g)


def _limits(t):
    g = t.group("limits", "limits and exact values")
    inf = math.inf
    for fn in ("Jn", "In", "jl"):
        t.add(fn, 0, 0.0, g, check="exact", expect=1.0)
        for n in (1, 2, 3, 4, 5):
            t.add(fn, n, 0.0, g, check="exact", expect=0.0)
    for fn, nu, want in (("Jnu", 0.0, 1.0), ("Inu", 0.0, 1.0), ("Jnu", 0.5, 0.0), ("Inu", 2.5, 0.0)):
        t.add(fn, nu, 0.0, g, check="exact", expect=want)
    for x in (705.0, 712.0, 745.0, 800.0, 1e5):
        over = x >= 745.0
        for fn, order, limit in (("In", 0, inf), ("In", 1, inf), ("In", 4, inf), ("Kn", 0, 0.0), ("Kn", 2, 0.0), ("Inu", 0.5, inf), ("Inu", 2.5, inf), ("Knu", 0.5, 0.0), ("Knu", 2.5, 0.0)):
            if over:
                t.add(fn, order, x, g, check="exact", expect=limit)
            else:
                t.add(fn, order, x, g)  # I within its budget (I_0(712) = 2.468e307: no early overflow); K is below 1e-300: no NaN
    t.add("Jnu", 160.0, 1e-7, g, check="exact", expect=0.0)  # the lgamma branch of inflx_sf_small_x
    t.add("Inu", 200.5, 1e-9, g, check="exact", expect=0.0)
    for x in (0.7, 3.3, 12.5):
        for fn in ("Jn", "In"):
            for n in (0, 1, 2, 5):
                base = t.add(fn, n, x, g)
                t.add(fn, n, -x, g, check="mirror", mirror=(base, (-1.0) ** n))
        for fn, sign in (("Jn", -1.0), ("Yn", -1.0), ("In", 1.0), ("Kn", 1.0)):
            base = t.add(fn, 3, x, g)
            t.add(fn, -3, x, g, check="mirror", mirror=(base, sign))


def _status(t):
    nan = math.nan
    inside = [0.25, 1.0, 7.5, 40.0]
    g = t.group("status", "inside every domain", 0)
    for kind in "JYIKjy":
        for order in (0, 1, 2, 5):
            for x in inside:
                t.add(kind + ("l" if kind in "jy" else "n"), order, x, g)
    for kind in "JYIK":
        for nu in (0.5, 3.25):
            for x in inside:
                t.add(kind + "nu", nu, x, g)
    for x in inside:
        t.add("0F1", (1.5,), x, g)
        t.add("1F1", (0.5, 1.5), x, g)
    for x in (-0.9, 0.0, 0.5, 0.95):
        t.add("2F1", (0.5, 1.0, 1.5), x, g)
    for x in (-3.0, -0.01, 0.0):
        t.add("2F0", (0.5, 1.0), x, g)
    g = t.group("status", "NaN arguments", 0)
    for kind in "YKyj":
        for order in (1, 4):
            t.add(kind + ("l" if kind in "jy" else "n"), order, nan, g, check="nan")
    for kind in "JYIK":
        t.add(kind + "nu", 0.5, nan, g, check="nan")
        for x in inside:
            t.add(kind + "nu", nan, x, g, check="nan")
    t.add("2F1", (0.5, 1.0, 1.5), nan, g, check="nan")
    t.add("2F0", (0.5, 1.0), nan, g, check="nan")
    outside = [(kind + ("l" if kind in "jy" else "n"), order, -1.0) for kind in "YKyj" for order in (0, 1, 2, 4)]
    outside += [(kind + ("l" if kind == "y" else "n"), 3, 0.0) for kind in "YKy"]
    outside += [(kind + "nu", -0.5, 1.0) for kind in "JYIK"] + [(kind + "nu", 0.5, -1.0) for kind in "JYIK"] + [(kind + "nu", 0.5, 0.0) for kind in "YK"]
    outside += [("0F1", (-2.0,), 1.0), ("1F1", (0.5, -1.0), 1.0), ("2F1", (0.5, 1.0, -3.0), 0.5), ("2F1", (0.5, 1.0, 1.5), 1.0), ("2F1", (0.5, 1.0, 1.5), -1.5), ("2F0", (0.5, 1.0), 0.5)]
    for fn, order, x in outside:
        t.add(fn, order, x, t.group("status", f"outside the domain: {fn}({order}; {x})", EDOM), check="nan")
    for fn, order, x in [("Jnu", 2e7, 1.0), ("2F0", (0.1, 0.2), -5.0), ("2F1", (1.0, 1.0, 2.0 + 1e-7), 0.9999)]:
        t.add(fn, order, x, t.group("status", f"declined: {fn}({order}; {x})", EDECLINED), check="nan")


_TABLE = None


def table(lib):
    """The table, built once per process (the 2F0 seams are looked for on the host twin ``lib``)."""
    global _TABLE
    if _TABLE is None:
        t = Table()
        _seams(t, lib)
        _range(t)
        _tiny(t)
        _limits(t)
        _status(t)
        _TABLE = t
    return _TABLE


# ---- truth ------------------------------------------------------------------------------------------------------------------
_TRUTH: dict = {}


def truth(case):
    """(value, scale) as mpmath numbers: the function at 40 (Bessel) or 50 (hypergeometric) digits and the amplitude an absolute
    error is judged against (None while the value is out of [1e-300, 1e300]: no budget applies there).  Computed once per process."""
    key = (case.fn, case.n, case.p, case.x)
    if key not in _TRUTH:
        _TRUTH[key] = _truth(case)
    return _TRUTH[key]


def in_range(value):
    import mpmath as mp

    return bool(mp.isfinite(value)) and 1e-300 <= abs(value) <= 1e300


def _truth(case):
    import mpmath as mp

    fn, x = case.fn, case.x
    if fn in INTEGER:
        kind = fn[0]
        want = special.mp_bessel(kind, case.n, x)
        if not in_range(want):
            return want, None
        # special.mp_amplitude: the modulus of the oscillating pair above the turning point (one value for both of the pair's
        # functions, evaluated once), the magnitude of the function itself elsewhere
        if (kind in "JY" and x >= case.n) or (kind in "jy" and x >= case.n + 1):
            key = ("amplitude", kind.upper() == kind, case.n, x)
            if key not in _TRUTH:
                _TRUTH[key] = mp.mpf(special.mp_amplitude(kind, case.n, x))
            return want, _TRUTH[key]
        return want, abs(want)
    if fn in REAL:
        nu, kind = case.p[0], fn[0]
        f = {"J": mp.besselj, "Y": mp.bessely, "I": mp.besseli, "K": mp.besselk}[kind]
        with mp.workdps(40):
            xm = mp.mpf(x)
            want = f(nu, xm)
            if not in_range(want):
                return want, None
            amp = abs(want)
            if kind in "JY" and not (kind == "J" and nu >= x):
                key = ("amplitude", nu, x)
                if key not in _TRUTH:
                    _TRUTH[key] = mp.sqrt((want if kind == "J" else mp.besselj(nu, xm)) ** 2 + (want if kind == "Y" else mp.bessely(nu, xm)) ** 2)
                amp = _TRUTH[key]
            return want, amp
    with mp.workdps(50):
        xm, p = mp.mpf(x), case.p
        want = {"0F1": lambda: mp.hyp0f1(p[0], xm), "1F1": lambda: mp.hyp1f1(p[0], p[1], xm), "2F1": lambda: mp.hyp2f1(p[0], p[1], p[2], xm), "2F0": lambda: mp.hyp2f0(p[0], p[1], xm)}[fn]()
        want = mp.re(want)
        if not in_range(want):
            return want, None
        scale = abs(want)
        if fn == "0F1" and x < 0:  # oscillating: the envelope of the underlying Bessel pair, as in the existing tests
            z, a = 2 * mp.sqrt(-xm), abs(p[0] - 1)
            if z > a:
                scale = max(scale, abs(mp.gamma(p[0])) * (-xm) ** ((1 - p[0]) / 2) * mp.sqrt(mp.besselj(a, z) ** 2 + mp.bessely(a, z) ** 2))
        return want, scale


def budget(case, scale, device):
    """the existing tests' budgets, absolute"""
    x = abs(case.x)
    if case.fn in INTEGER:
        return (2e-15 + 2e-16 * abs(case.n)) * max(1.0, x / 10.0) * float(scale)
    if case.fn in REAL:
        return 1e-14 * max(1.0, x / 10.0) * float(scale)
    return (2e-12 if device else 1e-12) * float(scale)


# ---- verdict ----------------------------------------------------------------------------------------------------------------
class Verdict:
    __slots__ = ("ok", "rule", "ratio", "why")

    def __init__(self, ok, rule, ratio=0.0, why=""):
        self.ok, self.rule, self.ratio, self.why = ok, rule, ratio, why


RULES = ("budget", "exact", "range", "subnormal", "declined")
LENIENT = ("range", "subnormal", "declined")  # the only ways a case may escape its budget


def _bits(v):
    return struct.pack("<d", v)


def _one(case, got, results, status, device):
    import mpmath as mp

    nan = got != got
    if case.check == "nan":
        return Verdict(nan, "exact", why="" if nan else f"{got!r} where NaN is due")
    if case.check == "exact":
        return Verdict(got == case.expect, "exact", why=f"{got!r} where {case.expect!r} is due")
    if case.check == "mirror":
        base, sign = case.mirror
        return Verdict(_bits(got) == _bits(sign * results[base]), "exact", why=f"{got!r} is not {sign:+g} times {results[base]!r} bit for bit")
    want, scale = truth(case)
    sign_ok = lambda: (got > 0) == (want > 0)
    if 0.0 < abs(case.x) < DBL_MIN:
        ok = not nan and (not math.isinf(got) or sign_ok())
        return Verdict(ok, "subnormal", why=f"{got!r} at a subnormal argument, truth {mp.nstr(want, 17)}")
    if scale is None:
        ok = not nan and (not math.isinf(got) or sign_ok())
        if ok and not math.isinf(got) and abs(got) >= DBL_MIN and want != 0:  # of normal size: on the truth's side, with its sign
            ok = sign_ok() and (abs(got) <= 1e-290 if abs(want) < 1 else abs(got) >= 1e290)
        return Verdict(ok, "range", why=f"{got!r} where the truth is {mp.nstr(want, 17)}")
    if nan:
        if case.decline_ok and status == EDECLINED:
            return Verdict(True, "declined")
        return Verdict(False, "budget", math.inf, f"NaN where the truth is {mp.nstr(want, 17)}")
    allowed = budget(case, scale, device)
    err = float(abs(want - mp.mpf(got)))
    return Verdict(err <= allowed, "budget", err / allowed, f"{got!r} where the truth is {mp.nstr(want, 17)}: error {err:.3e}, budget {allowed:.3e}")


def judge(table, results, status, device):
    """One Verdict per case.  ``results``: the value of every case; ``status``: per group, (status word, status word on the next read)."""
    return [_one(c, float(results[i]), results, status[c.group][0], device) for i, c in enumerate(table.cases)]


def failures(table, verdicts, family):
    return [f"{c!r}: {v.why}" for c, v in zip(table.cases, verdicts) if c.family == family and not v.ok]


def status_failures(table, status, family):
    """groups of ``family`` whose status word is not the expected one, or is not 0 on the next read"""
    return [f"{g.label}: status {status[k][0]} then {status[k][1]}, expected {g.status} then 0" for k, g in enumerate(table.groups) if g.family == family and tuple(status[k]) != (g.status, 0)]


def report(table, verdicts, title):
    lines = [title, f"{len(table.cases)} cases in {len(table.groups)} groups; per family: " + ", ".join(f"{f} {n}" for f, n in sorted(table.counts().items()))]
    lines.append(f"{'function':8s} {'cases':>6s} {'budget':>7s} {'exact':>6s} {'range':>6s} {'subnormal':>9s} {'declined':>8s} {'failed':>6s}  worst error / budget (at)")
    for fn in FUNCTIONS:
        mine = [(c, v) for c, v in zip(table.cases, verdicts) if c.fn == fn]
        by_rule = Counter(v.rule for _, v in mine)
        judged = [(v.ratio, c) for c, v in mine if v.rule == "budget"]
        worst = max(judged, key=lambda t: t[0]) if judged else (0.0, None)
        lines.append(f"{fn:8s} {len(mine):6d} {by_rule['budget']:7d} {by_rule['exact']:6d} {by_rule['range']:6d} {by_rule['subnormal']:9d} {by_rule['declined']:8d} {sum(not v.ok for _, v in mine):6d}  {worst[0]:.3f} ({worst[1]!r})")
    return "\n".join(lines)
