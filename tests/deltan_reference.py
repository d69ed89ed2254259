"""Truth, restatement and host twin of the delta-N stencils (csrc/inflx_deltan.h) -- TEST INFRASTRUCTURE.

* ``DeltaNTwin`` compiles tests/deltan_twin.cpp -- the generated headers, csrc/inflx_background.h and csrc/inflx_deltan.h for the CPU,
  contraction off -- and drives every stencil as ``inflx_delta_n`` does.
* ``DeltaNRestatement`` is the same algorithm in Python floats over ``background_reference.Restatement``'s stepper: the two event searches
  and the stop rules spelled a second time.  It checks the C++ against another spelling, not the algorithm.
* ``truth_members`` is independent of both: the Euler-Lagrange right-hand side of tests/background_truth.py integrated by scipy's
  DOP853 at rtol 1e-13, with a terminal event on epsilon_H = 1 for the centre and on H = H_c for each of the nine members, the velocity
  rule restated from the sympy model.  ``formulas`` applies the delta-N formulas in numpy with G and Gamma from sympy (``geometry``).

The three cases of the truth tests are ``CASES``: the hyperbolic example model (Gamma != 0, rule "fixed"), a flat double-quadratic
model built here (m2 / m1 = 3, rule "slow_roll") and the fuzzed model fuzz0 of tests/test_model_fuzz.py (G_00 = 1 + x^2, rule
"fixed"), each with stencils 8 to 12 e-folds before the end of inflation.

``python tests/deltan_reference.py`` measures the twin's error against the truth and writes profiles/background_deltan.json;
``bound`` is what the tests assert: 1e-10 plus twice that.
"""

from __future__ import annotations

import ctypes as C
import functools
import hashlib
import json
import math
import os
import subprocess
import sys
import tempfile
from typing import NamedTuple

import numpy as np
import sympy as sp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "inflatox_amd", "csrc")
PROFILE = os.path.join(ROOT, "profiles", "background_deltan.json")
_DP = C.POINTER(C.c_double)

COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW, TARGET = 0, 1, 2, 3, 4, 5
LOCATED, PAST_SURFACE = 7, 8
FIXED, SLOW_ROLL, EXPLICIT = 0, 1, 2
RULES = {"fixed": FIXED, "slow_roll": SLOW_ROLL, "explicit": EXPLICIT}
MAX_LOCATE = 64
H_DEFAULT = 1e-2
MAX_ERRS = (1e-8, 1e-10)


class TwinDeltaN(NamedTuple):
    """What ``DeltaNTwin.delta_n`` returns: ``dn`` -- ``inflatox_amd.background.DeltaN`` --, ``N_c`` (B,) of phase A, ``member_status``
    and ``accepted`` (B, 9), ``centre_status`` and ``centre_accepted`` (B,) of phase A, ``out`` (21, B) as the C function's"""

    dn: object
    N_c: np.ndarray
    member_status: np.ndarray
    accepted: np.ndarray
    centre_status: np.ndarray
    centre_accepted: np.ndarray
    out: np.ndarray


# ---- the host build --------------------------------------------------------------------------------------------------------------
def host_artifact_of(model, cse=False, name="model"):
    """An artefact as far as the host twins need it (``background_truth.host_artifact`` for any model): no hipcc step"""
    from inflatox_amd import Compiler
    from inflatox_amd.compiler import CompilationArtifact

    comp = Compiler(model, silent=True, cse=cse)
    header = comp._generate_hip_header()
    art = CompilationArtifact(comp.symbol_dict, f"/nonexistent/{name}.hsaco", 2, len(comp.symbol_dict) - 2, auto_cleanup=False)
    art._build = (header, [], "")
    art._eom_recipe = (model, dict(comp._param_slots), comp.cse, comp.max_cses)
    return art


class DeltaNTwin:
    """tests/deltan_twin.cpp built for the CPU from an artefact's generated headers, contraction off like the other twins"""

    def __init__(self, artifact, cxx: str = "g++", contract: str = "off"):
        self.artifact = artifact
        texts = (artifact._build[0], artifact.eom_header_text())
        sources = [os.path.join(CSRC, "inflx_background.h"), os.path.join(CSRC, "inflx_deltan.h"), os.path.join(HERE, "deltan_twin.cpp")]
        tag = hashlib.sha1(("".join(texts) + "".join(open(f).read() for f in sources) + contract).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_deltan_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".so"))
        if not os.path.exists(so):
            for path, text in zip((hdr, eom_hdr), texts):
                with open(path, "w") as fh:
                    fh.write(text)
            tmp = so + f".{os.getpid()}.tmp"
            subprocess.run([cxx, "-O2", "-fPIC", "-shared", "-o", tmp, *self.compile_options(hdr, eom_hdr, contract), sources[-1]], check=True)
            os.replace(tmp, so)
        self.headers = (hdr, eom_hdr)
        self.lib = C.CDLL(so)
        self.lib.twin_delta_n.argtypes = [_DP, C.c_size_t, _DP, _DP, C.c_int, C.c_double, C.c_double, _DP, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_double,
                                          _DP, _DP, _DP, _DP]  # fmt: skip
        self.lib.twin_delta_n.restype = None
        self.lib.twin_reduce.argtypes = [_DP, _DP, C.POINTER(C.c_int), C.c_int, _DP, C.c_double, C.c_double, _DP, C.c_size_t, _DP]
        self.lib.twin_reduce.restype = None

    @staticmethod
    def compile_options(hdr, eom_hdr, contract="off"):
        """what any build of tests/deltan_twin.cpp takes besides its output (the stand-alone program adds -DDELTAN_TWIN_MAIN)"""
        return ["-std=c++17", f"-ffp-contract={contract}", *(["-mfma"] if contract != "off" else []), "-fno-fast-math", "-Wno-unknown-pragmas", f"-I{CSRC}",
                f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"']  # fmt: skip

    def delta_n(self, pars, fields_init, derivatives_init=None, *, h=H_DEFAULT, velocity="fixed", H_end=None, max_steps=1_000_000, max_err=1e-10, solver="rkf",
                dt=None) -> TwinDeltaN:  # fmt: skip
        """``inflatox_amd.background.delta_N``'s arguments, through its own checks"""
        from inflatox_amd import background

        p, centre, vel, rule, h0, h1, h_end, max_steps, max_err, dt = background._check_delta_n(self.artifact, pars, fields_init, derivatives_init, h, velocity, H_end,
                                                                                                 max_steps, max_err, solver, dt)  # fmt: skip
        B = centre.shape[0]
        out, surface, members, centres = np.empty((21, B)), np.empty((2, B)), np.empty((B, 9, 3)), np.empty((B, 3))
        ptr = lambda a: None if a is None else a.ctypes.data_as(_DP)  # noqa: E731
        self.lib.twin_delta_n(ptr(p), 0 if p.ndim == 1 else p.shape[1], ptr(centre), ptr(vel), rule, h0, h1, ptr(h_end), B, max_steps, 1 if solver == "rkf" else 0, max_err,
                              dt or 0.0, ptr(out), ptr(surface), ptr(members), ptr(centres))  # fmt: skip
        dn = background._delta_n_result(out, surface, out[20].astype(np.int32))
        return TwinDeltaN(dn, surface[1], members[..., 0].astype(np.int64), members[..., 2].astype(np.int64), centres[:, 0].astype(np.int64),
                          centres[:, 2].astype(np.int64), out)  # fmt: skip

    def reduce(self, p, n_members, x, h, h_star, status=None, status_a=LOCATED):
        """``inflx_dn_reduce`` on given planes: n_members (B, 3, 3), x (B, 2), h a pair, h_star (B,): (out (21, B), DeltaN)"""
        from inflatox_amd import background

        n9 = np.ascontiguousarray(np.asarray(n_members, dtype=np.float64).reshape(-1, 9))
        B = n9.shape[0]
        st = np.ascontiguousarray(np.full((B, 9), LOCATED) if status is None else status, dtype=np.int32)
        x = np.ascontiguousarray(x, dtype=np.float64)
        h_star = np.ascontiguousarray(np.broadcast_to(np.asarray(h_star, dtype=np.float64), (B,)))
        p = np.ascontiguousarray(p, dtype=np.float64)
        out = np.empty((21, B))
        self.lib.twin_reduce(p.ctypes.data_as(_DP), n9.ctypes.data_as(_DP), st.ctypes.data_as(C.POINTER(C.c_int)), int(status_a), x.ctypes.data_as(_DP), float(h[0]),
                             float(h[1]), h_star.ctypes.data_as(_DP), B, out.ctypes.data_as(_DP))  # fmt: skip
        return out, background._delta_n_result(out, np.full((2, B), np.nan), out[20].astype(np.int32))


# ---- the sympy side: velocity rule, metric, connection ------------------------------------------------------------------------------
def _slots(model, param_slots, exprs):
    plain = sp.printing.c.C99CodePrinter()._print_Symbol
    free = set().union(*[sp.sympify(e).free_symbols for e in exprs]) - set(model.coordinates) - set(model.coordinate_tangents)
    params = sorted(free, key=lambda s: int(param_slots[plain(s)][5:-1]))
    return params, [int(param_slots[plain(s)][5:-1]) for s in params]


@functools.lru_cache(maxsize=None)
def _geometry_exprs(model):
    n = 2
    X = list(model.coordinates)
    G = sp.Matrix(n, n, lambda a, b: sp.sympify(model.metric[a][b]))
    Gi = G.inv()
    V = sp.sympify(model.potential)
    gam = [[[sum(Gi[a, d] * (sp.diff(G[d, b], X[c]) + sp.diff(G[d, c], X[b]) - sp.diff(G[b, c], X[d])) for d in range(n)) / 2 for c in range(n)] for b in range(n)]
           for a in range(n)]  # fmt: skip
    up = [sum(Gi[a, b] * sp.diff(V, X[b]) for b in range(n)) for a in range(n)]
    return G, gam, up, V


def geometry(model, param_slots):
    """f(x0, x1, p) -> (G (2, 2), Gamma (2, 2, 2) [a][b][c] = Gamma^a_bc, G^ab d_b V (2,), V) from the sympy model"""
    G, gam, up, V = _geometry_exprs(model)
    exprs = [G[0, 0], G[0, 1], G[1, 1], *[gam[a][b][c] for a in range(2) for b in range(2) for c in range(2)], *up, V]
    params, slots = _slots(model, param_slots, exprs)
    fn = sp.lambdify([*model.coordinates, *params], exprs, modules="math", cse=True)

    def f(x0, x1, p):
        v = [float(w) for w in fn(x0, x1, *[p[k] for k in slots])]
        return np.array([[v[0], v[1]], [v[1], v[2]]]), np.array(v[3:11]).reshape(2, 2, 2), np.array(v[11:13]), v[13]

    return f


def member_states(geom, p, x, v, h, rule, vel9=None):
    """(9, 4): the initial fields and velocities of the nine members around the centre x (2,) with velocity v (2,), rule restated"""
    out = np.empty((9, 4))
    for m in range(9):
        i, j = divmod(m, 3)
        y0, y1 = x[0] + (i - 1) * h[0], x[1] + (j - 1) * h[1]
        if rule == SLOW_ROLL:
            _G, _gam, up, V = geom(y0, y1, p)
            w = -up / (3.0 * math.sqrt(V / 3.0))
        elif rule == EXPLICIT:
            w = vel9[m]
        else:
            w = v
        out[m] = [y0, y1, w[0], w[1]]
    return out


def formulas(n33, G, gam, h, h_star):
    """the delta-N formulas in numpy: (N_I (2,), N_IJ (2, 2), N_cov (2, 2), grad2, f_NL, P_zeta) of one stencil n33 (3, 3)"""
    n = np.asarray(n33, dtype=np.float64)
    n_i = np.array([(n[2, 1] - n[0, 1]) / (2 * h[0]), (n[1, 2] - n[1, 0]) / (2 * h[1])])
    cross = (n[2, 2] - n[2, 0] - n[0, 2] + n[0, 0]) / (4 * h[0] * h[1])
    n_ij = np.array([[(n[2, 1] - 2 * n[1, 1] + n[0, 1]) / h[0] ** 2, cross], [cross, (n[1, 2] - 2 * n[1, 1] + n[1, 0]) / h[1] ** 2]])
    cov = n_ij - np.einsum("kij,k->ij", gam, n_i)
    up = np.linalg.solve(G, n_i)
    grad2 = float(up @ n_i)
    return n_i, n_ij, cov, grad2, 5.0 / 6.0 * float(up @ cov @ up) / grad2**2, (h_star / (2 * math.pi)) ** 2 * grad2


# ---- the truth -------------------------------------------------------------------------------------------------------------------
T_MAX = 1e5


def _truth_run(g, init, p, event):
    from scipy.integrate import solve_ivp

    import background_truth as bt

    rhs = bt.bound(g, p)

    def f(_t, s):
        a, b, V, _k = rhs(s[0], s[1], s[2], s[3])
        return [s[2], s[3], -a - 3.0 * s[4] * s[2], -b - 3.0 * s[4] * s[3], V - 3.0 * s[4] * s[4], s[4]]

    event.terminal = True
    sol = solve_ivp(f, (0.0, T_MAX), bt.initial_y(rhs, init), method="DOP853", rtol=1e-13, atol=1e-15, events=[event])
    assert sol.status == 1 and len(sol.y_events[0]) == 1, "the truth did not meet its event"
    return sol.y_events[0][0]


def truth_end(g, init, p):
    """(H_c, N_c): H and N where epsilon_H = 1 on the trajectory from ``init`` (4,)"""

    def event(_t, s):
        return 0.5 * g(s[0], s[1], s[2], s[3], p)[3] / (s[4] * s[4]) - 1.0

    event.direction = 1
    y = _truth_run(g, init, p, event)
    return float(y[4]), float(y[5])


def truth_surface(g, init, p, h_c):
    """N where H = h_c on the trajectory from ``init`` (4,)"""

    def event(_t, s):
        return s[4] - h_c

    event.direction = -1
    return float(_truth_run(g, init, p, event)[5])


def truth_members(g, geom, p, x, v, h, rule, vel9=None, H_end=None):
    """(N (3, 3), H_c, N_c, H_star) of one stencil: the velocity rule restated, the surface from the centre's own epsilon_H = 1"""
    import background_truth as bt

    states = member_states(geom, p, x, v, h, rule, vel9)
    h_c, n_c = (H_end, math.nan) if H_end is not None else truth_end(g, states[4], p)
    n = np.array([truth_surface(g, states[m], p, h_c) for m in range(9)]).reshape(3, 3)
    return n, h_c, n_c, bt.initial_y(bt.bound(g, p), states[4])[4]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def _hermite(y0, f0, y1, f1, h, th):
    u = 1.0 - th
    h00, h10, h01, h11 = (1.0 + 2.0 * th) * u * u, th * u * u, th * th * (3.0 - 2.0 * th), -(th * th) * u
    return h00 * y0 + h10 * (h * f0) + h01 * y1 + h11 * (h * f1)


def _hermite_slope(y0, f0, y1, f1, h, th):
    u = 1.0 - th
    d00, d10, d11 = -6.0 * th * u, u * (1.0 - 3.0 * th), th * (3.0 * th - 2.0)
    return d00 * y0 + d10 * (h * f0) - d00 * y1 + d11 * (h * f1)


def _locate(n0, h0, n1, h1, h, target):
    """csrc/inflx_background.h inflx_bg_locate"""
    lo, hi = 0.0, 1.0
    th = (target - n0) / (n1 - n0)
    if not th > 0.0:
        th = 0.0
    if th > 1.0:
        th = 1.0
    for _ in range(MAX_LOCATE):
        g = _hermite(n0, h0, n1, h1, h, th) - target
        if g == 0.0:
            break
        if g < 0.0:
            lo = th
        else:
            hi = th
        nxt = th - g / _hermite_slope(n0, h0, n1, h1, h, th)
        if not (lo < nxt < hi):
            nxt = 0.5 * (lo + hi)
        moved = abs(nxt - th)
        th = nxt
        if moved <= 1e-15 or hi - lo <= 1e-15:
            break
    return th


class DeltaNRestatement:
    """One lane of csrc/inflx_deltan.h in Python floats, on ``background_reference.Restatement``'s stepper"""

    def __init__(self, eom, p):
        from background_reference import Restatement

        self.r = Restatement(eom, p)

    def _start(self, init):
        r = self.r
        _e0, _e1, V, kin = r.eom(init[0], init[1], init[2], init[3], r.p)
        y = [float(init[0]), float(init[1]), float(init[2]), float(init[3]), math.sqrt((V + 0.5 * kin) / 3.0), 0.0]
        f, kin = r.rhs(y)
        return y, f, kin

    def _step(self, method, y, f, t, h, max_err):
        """one accepted adaptive step: (y1, f1, kin1, t1, h_next, h_taken) or a status"""
        r = self.r
        rejections = 0
        while True:
            if t + h == t:
                return UNDERFLOW
            y1, err = r.trial(method, y, f, h, True)
            ok = all(math.isfinite(c) for c in y1) and math.isfinite(err)
            if ok and err <= 1.1 * max_err:
                taken = h
                t += h
                h *= r.factor(max_err, err)
                break
            h *= r.factor(max_err, err) if ok else 0.2
            rejections += 1
            if rejections >= r.MAX_REJECTIONS:
                return REJECTED
        f1, kin1 = r.rhs(y1)
        if not (all(math.isfinite(c) for c in f1) and math.isfinite(kin1)):
            return NONFINITE
        return y1, f1, kin1, t, h, taken

    def _eps_at(self, y0, f0, y1, f1, h, th):
        r = self.r
        y = [_hermite(y0[c], f0[c], y1[c], f1[c], h, th) for c in range(6)]
        kin = r.eom(y[0], y[1], y[2], y[3], r.p)[3]
        return y, 0.5 * kin / (y[4] * y[4])

    def end(self, init, method="rkf", max_err=1e-10, max_steps=1_000_000):
        """phase A: (status, H_c, N_c, accepted)"""
        y, f, kin = self._start(init)
        t, h, accepted = 0.0, self.r.FIRST_DT, 0
        if 0.5 * kin / (y[4] * y[4]) >= 1.0:
            return LOCATED, y[4], 0.0, 0
        for _ in range(max_steps):
            eps0 = 0.5 * kin / (y[4] * y[4])
            got = self._step(method, y, f, t, h, max_err)
            if isinstance(got, int):
                return got, math.nan, math.nan, accepted
            y1, f1, kin1, t, h, taken = got
            accepted += 1
            eps1 = 0.5 * kin1 / (y1[4] * y1[4])
            if eps1 >= 1.0:
                lo, hi, glo, ghi, side = 0.0, 1.0, eps0 - 1.0, eps1 - 1.0, 0
                if ghi == 0.0:
                    return LOCATED, y1[4], y1[5], accepted
                for _it in range(MAX_LOCATE):
                    th = (lo * ghi - hi * glo) / (ghi - glo)
                    if not (lo < th < hi):
                        th = 0.5 * (lo + hi)
                    loc, eps = self._eps_at(y, f, y1, f1, taken, th)
                    g = eps - 1.0
                    if g == 0.0:
                        break
                    if g < 0.0:
                        lo, glo = th, g
                        if side == -1:
                            ghi *= 0.5
                        side = -1
                    else:
                        hi, ghi = th, g
                        if side == 1:
                            glo *= 0.5
                        side = 1
                    if hi - lo <= 1e-15:
                        break
                return LOCATED, loc[4], loc[5], accepted
            y, f, kin = y1, f1, kin1
        return COMPLETE, math.nan, math.nan, accepted

    def surface(self, init, h_c, method="rkf", max_err=1e-10, max_steps=1_000_000):
        """phase B: (status, N on the surface, accepted)"""
        y, f, _kin = self._start(init)
        t, h, accepted = 0.0, self.r.FIRST_DT, 0
        if y[4] <= h_c:
            return PAST_SURFACE, math.nan, 0
        for _ in range(max_steps):
            got = self._step(method, y, f, t, h, max_err)
            if isinstance(got, int):
                return got, math.nan, accepted
            y1, f1, _kin1, t, h, taken = got
            accepted += 1
            if y1[4] <= h_c < y[4]:
                th = _locate(-y[4], -f[4], -y1[4], -f1[4], taken, -h_c)
                return LOCATED, _hermite(y[5], f[5], y1[5], f1[5], taken, th), accepted
            y, f = y1, f1
        return COMPLETE, math.nan, accepted


def host_eom(artifact):
    """eom(x0, x1, xd0, xd1, p) of the host-compiled generated function (``BackgroundTwin.eom``): the restatement then differs from the
    twin in the integrator alone"""
    from background_reference import BackgroundTwin

    twin = BackgroundTwin(artifact)

    def eom(a, b, c, d, p):
        return tuple(float(v) for v in twin.eom(p, [[a, b, c, d]])[0])

    return eom


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    artifact: object  # host artefact (the twin's), or a compiled one
    model: object
    p: np.ndarray
    x: np.ndarray  # (B, 2) centres
    v: np.ndarray  # (B, 2) centre velocities (ignored by slow_roll)
    velocity: str


@functools.lru_cache(maxsize=None)
def double_quadratic_model():
    from inflatox_amd import InflationModelBuilder

    phi, chi, m1, m2 = sp.symbols("phi chi m1 m2")
    V = (m1**2 * phi**2 + m2**2 * chi**2) / 2
    return InflationModelBuilder.new([phi, chi], [[1, 0], [0, 1]], V, model_name="double_quadratic", init_sympy_printing=False, silent=True).build()


def _named_pars(art, **values):
    p = np.zeros(art.n_parameters)
    for name, value in values.items():
        p[int(art.symbol_dictionary[name][5:-1])] = value
    return p


@functools.lru_cache(maxsize=None)
def case(name, device=False):
    """The stencils of a truth case, 8 to 12 e-folds before the end of inflation.  ``device``: with a compiled artefact."""
    import background_truth as bt
    import workloads

    if name == "hyperbolic":
        spec, art = workloads.artifact_for("hyperbolic")
        model, p = workloads.model_for("hyperbolic"), np.asarray(spec.args, dtype=np.float64)
        x = np.array([[7.3, 0.4], [6.9, -0.7], [7.6, 0.1]])
        v = np.array([[-0.8, 1e-4], [-0.8, -2e-4], [-0.8, 5e-5]])
        velocity = "fixed"
    elif name == "double_quadratic":
        from inflatox_amd import Compiler

        model = double_quadratic_model()
        art = Compiler(model, silent=True).compile() if device else host_artifact_of(model, name=name)
        p = _named_pars(art, m1=1.0, m2=3.0)
        x = np.array([[6.0, 2.0], [5.5, 3.0], [6.3, 0.8]])
        v = np.zeros((3, 2))
        velocity = "slow_roll"
    elif name == "fuzz0":
        model = bt.zoo_model(name).model
        art = bt.device_artifact(name) if device else bt.host_artifact(name)
        p = np.array([1.0, 1.2, 0.8])[: art.n_parameters]
        x = np.array([[3.0, 0.5], [2.93, -0.4], [3.1, 0.9]])
        v = np.array([[-0.12, -0.05], [-0.12, 0.04], [-0.12, -0.08]])
        velocity = "fixed"
    else:
        raise KeyError(name)
    return Case(name, art, model, p, x, v, velocity)


CASES = ("hyperbolic", "double_quadratic", "fuzz0")


@functools.lru_cache(maxsize=None)
def case_functions(name):
    """(truth right-hand side g, geometry) of a case, from the sympy model alone"""
    import background_truth as bt

    c = case(name)
    return bt.truth_functions(c.model, c.artifact.symbol_dictionary), geometry(c.model, c.artifact.symbol_dictionary)


@functools.lru_cache(maxsize=None)
def case_truth(name, h=H_DEFAULT):
    """(N (B, 3, 3), H_c (B,), N_c (B,), H_star (B,)) of a case: computed once and shared"""
    c = case(name)
    g, geom = case_functions(name)
    rows = [truth_members(g, geom, c.p, c.x[b], c.v[b], (h, h), RULES[c.velocity]) for b in range(c.x.shape[0])]
    out = tuple(np.array([r[k] for r in rows]) for k in range(4))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_twin(name):
    return DeltaNTwin(case(name).artifact)


def members_error(got, want):
    """worst |N - truth| over the members, absolute (N is of order 10)"""
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want))))


# ---- the exact cases ---------------------------------------------------------------------------------------------------------------
POWER_H_END = 2.0  # the surface of the power-law case: H falls from 8 at the start to 2, N = 8 ln 4


def power_law_case(device=False):
    """Power-law inflation V = V0 exp(-lam phi) (``background_reference``): (artifact, p, x (B, 2), explicit velocities (B, 3, 3, 2) on
    the attractor at every member's own phi, h).  N = -phi / lam + const to any surface of constant H: N_,phi = -1 / lam, every other
    derivative vanishes."""
    import background_reference as br

    model = br.power_law_model()
    if device:
        art, p = br.power_law_artifact()
    else:
        art = host_artifact_of(model, name="power_law")
        p = _named_pars(art, V0=br.V0, lam=br.LAM)
    phi1 = br.power_law_init()[0]
    x = np.array([[phi1, 0.0], [phi1 + 0.7, 0.3], [phi1 + 1.5, -2.0]])
    h = H_DEFAULT
    phi = x[:, 0, None, None] + (np.arange(3)[None, :, None] - 1) * h + np.zeros((1, 1, 3))
    vel = np.stack([2.0 / (br.LAM * np.exp(br.LAM * (phi - phi1) / 2.0)), np.zeros_like(phi)], axis=-1)
    return art, p, x, vel, h


# ---- the recorded errors and the bound ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stepper_code_hash():
    """the hash of the code (comments aside) of the two headers that make the stepper: the state of the code a profile belongs to"""
    from inflatox_amd.compiler import _code_only

    h = hashlib.sha256()
    for f in ("inflx_background.h", "inflx_deltan.h"):
        with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
            h.update(_code_only(fh.read()).encode())
    return h.hexdigest()[:16]


def recorded():
    with open(PROFILE) as fh:
        return json.load(fh)


def bound(name, solver, max_err):
    """b: what |N_members - truth| may be -- 1e-10 plus twice the host twin's recorded worst error for this case, solver and max_err"""
    return 1e-10 + 2.0 * recorded()["members"][f"{name}/{solver}/{max_err:g}"]


def linear_end_members(c, h_c, h, max_err):
    """``efolds_map``-style N: every member to its OWN epsilon_H = 1, linear in epsilon_H across the last step (the host twin of the plain
    stepper): (B, 3, 3)"""
    from background_reference import BackgroundTwin

    _g, geom = case_functions(c.name)
    plain = BackgroundTwin(c.artifact)
    out = np.empty((c.x.shape[0], 3, 3))
    for b in range(c.x.shape[0]):
        states = member_states(geom, c.p, c.x[b], c.v[b], (h, h), RULES[c.velocity])
        for m in range(9):
            rows = 64
            while True:
                _o, meta = plain.solve(c.p, states[m], rows, "rkf", max_err=max_err, stop_at_end=True)
                if meta["status"] == ENDED:
                    break
                rows *= 2
                assert rows < 1 << 22
            out[b, m // 3, m % 3] = meta["N_end"]
    return out


def pzeta_against_modes(n_exit=6.0):
    """One hyperbolic trajectory from (9, 0.4) at rest: the mode that leaves the horizon ``n_exit`` e-folds later, P_R at the end of
    inflation from the mode functions (``ModesTwin.power_spectra``) against P_zeta of the delta-N stencil around the state at that
    exit with the exit velocity ('fixed') and with 'slow_roll' velocities: (P_R, P_zeta fixed, P_zeta slow_roll, f_NL fixed, f_NL
    slow_roll).  The two agree only to slow-roll order."""
    import modes_reference as mo
    from background_sampled_reference import SampledTwin

    c = case("hyperbolic")
    x0, v0 = np.array([[9.0, 0.4]]), np.zeros((1, 2))
    ps = mo.ModesTwin(c.artifact).power_spectra(c.p, [n_exit], x0, v0, max_err=1e-10)
    out, meta = SampledTwin(c.artifact).solve(c.p, np.concatenate([x0[0], v0[0]]), [n_exit], 1_000_000, "rkf", max_err=1e-10, stop_at_end=True)
    state = out[0]
    twin = case_twin("hyperbolic")
    fixed = twin.delta_n(c.p, state[None, :2], state[None, 2:4]).dn
    slow = twin.delta_n(c.p, state[None, :2], None, velocity="slow_roll").dn
    assert fixed.status[0] == LOCATED and slow.status[0] == LOCATED
    return float(ps.P_R[0, 0]), float(fixed.P_zeta[0]), float(slow.P_zeta[0]), float(fixed.f_NL[0]), float(slow.f_NL[0])


def measure():
    members, derivs, notes = {}, {}, {}
    for name in CASES:
        c = case(name)
        truth_n, truth_hc, truth_nc, _hs = case_truth(name)
        g, geom = case_functions(name)
        for solver in ("rk4", "rkf"):
            for max_err in MAX_ERRS:
                got = case_twin(name).delta_n(c.p, c.x, c.v, velocity=c.velocity, max_err=max_err, solver=solver)
                assert np.all(got.dn.status == LOCATED), (name, solver, max_err, got.dn.status)
                key = f"{name}/{solver}/{max_err:g}"
                members[key] = members_error(got.dn.N_members, truth_n)
                print(f"{name} {solver} max_err {max_err:g}: worst |twin - truth| of N_members {members[key]:.3e}, H_c {np.abs(got.dn.H_end - truth_hc).max():.3e}, "
                      f"N_c {np.abs(got.N_c - truth_nc).max():.3e}; {got.accepted.min()} .. {got.accepted.max()} steps", flush=True)  # fmt: skip
        # recorded, not asserted: truncation of the default h, N_,IJ against truth for three h, and the same from a linear N_end
        def second(n, h):
            return np.array([formulas(n[b], *geom(*c.x[b], c.p)[:2], (h, h), 1.0)[1] for b in range(n.shape[0])])

        half = case_truth(name, H_DEFAULT / 2)[0]
        trunc = float(np.max(np.abs(second(truth_n, H_DEFAULT) - second(half, H_DEFAULT / 2))))
        notes[f"{name}/truncation"] = trunc
        print(f"{name}: truth N_,IJ at h = {H_DEFAULT:g} against h / 2: {trunc:.3e}", flush=True)
        for h in (1e-2, 1e-3, 1e-4):
            want = second(case_truth(name, h)[0], h)
            got = case_twin(name).delta_n(c.p, c.x, c.v, velocity=c.velocity, h=h)
            derivs[f"{name}/located/{h:g}"] = float(np.max(np.abs(got.dn.N_IJ - want)))
            lin = second(linear_end_members(c, truth_hc, h, 1e-10), h)
            own = np.array([[truth_end(g, s, c.p)[1] for s in member_states(geom, c.p, c.x[b], c.v[b], (h, h), RULES[c.velocity])] for b in range(c.x.shape[0])])
            derivs[f"{name}/linear_end/{h:g}"] = float(np.max(np.abs(lin - second(own.reshape(-1, 3, 3), h))))
            print(f"{name} h = {h:g}: |N_,IJ - truth| located {derivs[f'{name}/located/{h:g}']:.3e}, linear N_end (own eps = 1 surface, own truth) "
                  f"{derivs[f'{name}/linear_end/{h:g}']:.3e}", flush=True)  # fmt: skip
    pr, pz_fixed, pz_slow, f_fixed, f_slow = pzeta_against_modes()
    notes["hyperbolic/P_R_end"], notes["hyperbolic/P_zeta_fixed"], notes["hyperbolic/P_zeta_slow_roll"] = pr, pz_fixed, pz_slow
    notes["hyperbolic/f_NL_fixed"], notes["hyperbolic/f_NL_slow_roll"] = f_fixed, f_slow
    print(f"hyperbolic: P_R at the end from the mode functions {pr:.6g}; P_zeta 'fixed' {pz_fixed:.6g}, 'slow_roll' {pz_slow:.6g}; f_NL {f_fixed:.5f}, {f_slow:.5f}", flush=True)
    import background_reference as br

    art, p, x, vel, h = power_law_case()
    got = DeltaNTwin(art).delta_n(p, x, vel, H_end=POWER_H_END)
    assert np.all(got.dn.status == LOCATED)
    t = np.exp(br.LAM * (x[:, 0, None, None] + (np.arange(3)[None, :, None] - 1) * h - br.power_law_init()[0]) / 2.0) + np.zeros((1, 1, 3))
    members["power_law/rkf/1e-10"] = members_error(got.dn.N_members, br.P_POW * np.log(br.P_POW / POWER_H_END / t))
    print(f"power law rkf max_err 1e-10: worst |twin - exact| of N_members {members['power_law/rkf/1e-10']:.3e}", flush=True)
    return {
        "stepper_code": stepper_code_hash(),
        "what": "worst absolute |host twin - truth| of N_members over the three stencils of tests/deltan_reference.py case(name), h = 1e-2; truth: DOP853 at rtol 1e-13 on "
                "the Euler-Lagrange background with terminal events on epsilon_H = 1 (centre) and H = H_c (members); power_law: against the exact N = 8 ln(t_c / t) of "
                "the attractor, explicit velocities, H_end = 2",
        "bound": "tests assert b = 1e-10 + 2 x the value recorded here on N_members, b / h on N_,I and 4 b / h^2 on N_,IJ",
        "members": members,
        "derivatives": derivs,
        "derivatives_what": "recorded, not asserted: worst |N_,IJ - truth| at max_err = 1e-10 (rkf) for h = 1e-2, 1e-3, 1e-4 -- 'located': the twin's stencil against the "
                            "truth's at the same h; 'linear_end': the same second differences of N_end as efolds_map computes it (every member to its own epsilon_H = 1, "
                            "linear in epsilon_H across the last step) against the truth's N at each member's own epsilon_H = 1",
        "notes": notes,
        "notes_what": "truncation: the truth's N_,IJ at h = 1e-2 against h = 5e-3; hyperbolic/P_*: one trajectory from (9, 0.4) at rest, the mode that leaves the horizon 6 "
                      "e-folds later -- P_R at the end of inflation from the host twin of power_spectra against P_zeta (and f_NL) of the stencil around the exit state "
                      "under the two velocity rules; they agree to slow-roll order only",
    }  # fmt: skip


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    result = measure()
    with open(PROFILE, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
