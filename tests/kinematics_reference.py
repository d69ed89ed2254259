"""Truth and host twin of the trajectory kinematics (csrc/inflx_kinematics.h) -- TEST INFRASTRUCTURE.

``truth_kinematics`` evaluates the six quantities of ``inflatox_amd.background.kinematics`` in 40-digit arithmetic by another route
than the code: the accelerations come from the Euler-Lagrange derivation of tests/background_truth.py (no connection, no inverse
metric), sigma_ddot from the chain rule on sigma_dot^2 = G_ab chi^a chi^b through those accelerations, the turn rate as the norm
|D_t T|_G of the covariant derivative of the unit tangent through Christoffel symbols formed here, its sign from the projection on
the normal, and V_N and |dV|^2 through the inverse metric.  The code forms none of these: it evaluates 3 + d_a V chi^a / (H kin)
and the cross form (d_0 V chi_1 - d_1 V chi_0) / sqrt(det G).

``allowance`` is the bound the kinematics issue sets: the project's parity bar, 1e-10, applied to the size of the terms a quantity
is built from.  ``KinematicsTwin`` compiles tests/kinematics_twin.cpp -- the generated headers and csrc/inflx_kinematics.h for the
CPU.  ``zoo_states`` gives the states of a zoo model that the CPU and the GPU tests share, and ``zoo_truth`` their truth, computed
once.
"""

from __future__ import annotations

import ctypes as C
import functools
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import sympy as sp

import background_truth as bt

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "inflatox_amd", "csrc")
_DP = C.POINTER(C.c_double)

NAMES = ("eps_H", "eta_par", "omega", "sigma_dot", "V_sigma", "V_N")
RTOL = 1e-10  # the project's parity bar
DPS = 40
_H = sp.Symbol("H_hubble", positive=True)


# ---- the truth -------------------------------------------------------------------------------------------------------------------
def truth_expressions(fields, metric, potential, tangents):
    """[eps_H, eta_par, omega (signed), sigma_dot, V_sigma, V_N, S^2 = |dV|^2_G] as sympy expressions of the fields, the velocities,
    the parameters and the Hubble rate (``_H``)."""
    n = len(fields)
    G = sp.Matrix(n, n, lambda a, b: sp.sympify(metric[a][b]))
    Ginv = G.inv()
    V = sp.sympify(potential)
    chi = list(tangents)
    eom, _V, kin = bt.euler_lagrange_eom(fields, metric, potential, tangents)
    acc = [-eom[a] - 3 * _H * chi[a] for a in range(n)]  # phi''^a
    sigma_dot = sp.sqrt(kin)
    # d/dt (G_ab chi^a chi^b) = d_c G_ab chi^c chi^a chi^b + 2 G_ab chi^a phi''^b = 2 sigma_dot sigma_ddot
    dkin = sum(sp.diff(G[a, b], fields[c]) * chi[c] * chi[a] * chi[b] for a in range(n) for b in range(n) for c in range(n))
    dkin += 2 * sum(G[a, b] * chi[a] * acc[b] for a in range(n) for b in range(n))
    sigma_ddot = dkin / (2 * sigma_dot)
    # D_t T^a = dT^a/dt + Gamma^a_bc chi^b T^c,  T^a = chi^a / sigma_dot
    gamma = [[[sum(Ginv[a, d] * (sp.diff(G[d, b], fields[c]) + sp.diff(G[d, c], fields[b]) - sp.diff(G[b, c], fields[d])) for d in range(n)) / 2
               for c in range(n)] for b in range(n)] for a in range(n)]  # fmt: skip
    T = [chi[a] / sigma_dot for a in range(n)]
    DT = [acc[a] / sigma_dot - chi[a] * sigma_ddot / kin + sum(gamma[a][b][c] * chi[b] * T[c] for b in range(n) for c in range(n)) for a in range(n)]
    turn = sp.sqrt(sum(G[a, b] * DT[a] * DT[b] for a in range(n) for b in range(n)))  # |D_t T|_G
    root = sp.sqrt(G.det())
    N_low = [root * T[1], -root * T[0]]  # N_a = sqrt(det G) eps_ab T^b
    side = -sum(N_low[a] * DT[a] for a in range(n))  # D_t T = -Omega N: the sign of Omega
    dV = [sp.diff(V, f) for f in fields]
    v_sigma = sum(T[a] * dV[a] for a in range(n))
    v_n = sum(Ginv[a, b] * N_low[b] * dV[a] for a in range(n) for b in range(n))
    s2 = sum(Ginv[a, b] * dV[a] * dV[b] for a in range(n) for b in range(n))
    return [kin / (2 * _H**2), -sigma_ddot / (_H * sigma_dot), sp.sign(side) * turn / _H, sigma_dot, v_sigma, v_n, s2]


def truth_function(fields, metric, potential, tangents, param_slots=None):
    """f(y (5,), p) -> the seven values of ``truth_expressions`` at the float64 state y and parameter row p, evaluated at ``DPS``
    digits, as mpf.  ``param_slots`` as for ``background_truth.point_function``."""
    import mpmath
    from sympy.printing.c import C99CodePrinter

    exprs = truth_expressions(fields, metric, potential, tangents)
    plain = C99CodePrinter()._print_Symbol
    free = set().union(*[e.free_symbols for e in exprs]) - set(fields) - set(tangents) - {_H}
    if param_slots is None:
        names = sorted(plain(s) for s in free)
        slot = {s: names.index(plain(s)) for s in free}
    else:
        slot = {s: int(param_slots[plain(s)][5:-1]) for s in free}
    params = sorted(free, key=slot.get)
    fn = sp.lambdify([*fields, *tangents, _H, *params], exprs, modules="mpmath", cse=True)

    def f(y, p):
        with mpmath.workdps(DPS):
            return [+v for v in fn(*[mpmath.mpf(float(v)) for v in y], *[mpmath.mpf(float(p[slot[s]])) for s in params])]

    return f


def truth_table(f, states, pars):
    """(n, 7) float64 of ``truth_function`` f over the states (n, 5), parameter rows (n, n_par) or one row (n_par,)."""
    pars = np.asarray(pars)
    return np.array([[float(v) for v in f(states[k], pars[k] if pars.ndim == 2 else pars)] for k in range(states.shape[0])])


def allowance(truth, H):
    """(6, n): the largest |got - truth| allowed for each quantity; ``truth`` (n, 7) from ``truth_table``, ``H`` (n,).  With S =
    sqrt(|dV|^2_G): eps_H and sigma_dot 1e-10 of themselves, V_sigma and V_N 1e-10 S, omega 1e-10 S / (sigma_dot |H|), eta_par
    1e-10 (3 + S / (sigma_dot |H|))."""
    eps, sd, S = truth[:, 0], truth[:, 3], np.sqrt(truth[:, 6])
    ratio = S / (sd * np.abs(H))
    return RTOL * np.stack([eps, 3.0 + ratio, ratio, sd, S, S])


def worst_ratios(got, truth, H):
    """{quantity: max |got - truth| / allowance}; ``got`` (6, n)"""
    r = np.abs(np.asarray(got) - truth[:, :6].T) / allowance(truth, H)
    return {name: float(r[q].max()) for q, name in enumerate(NAMES)}


# ---- the states the CPU and the GPU tests share ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _zoo_truth_function(name):
    z = bt.zoo_model(name)
    return truth_function(z.model.coordinates, z.model.metric, z.model.potential, z.model.coordinate_tangents, bt.host_artifact(name).symbol_dictionary)


@functools.lru_cache(maxsize=None)
def zoo_states(name):
    """(states (257, 5), pars (257, n_par)): the lanes of ``background_truth.batch(name)`` with H from the Friedmann constraint of
    the Euler-Lagrange derivation in 40-digit arithmetic, rounded to float64."""
    import mpmath

    z = bt.zoo_model(name)
    init, pars = bt.batch(name)
    energy = bt.point_function(z.model.coordinates, z.model.coordinate_tangents, bt._derivation(z.model)[1:], bt.host_artifact(name).symbol_dictionary, modules="mpmath")
    with mpmath.workdps(DPS):
        H = [float(mpmath.sqrt((V + kin / 2) / 3)) for V, kin in (energy(*[mpmath.mpf(float(v)) for v in pt], [mpmath.mpf(float(v)) for v in p]) for pt, p in zip(init, pars))]
    states = np.concatenate([init, np.array(H)[:, None]], axis=1)
    states.setflags(write=False)
    return states, pars


@functools.lru_cache(maxsize=None)
def zoo_truth(name, n):
    """``truth_table`` of the first n states of ``zoo_states(name)``: computed once and shared."""
    states, pars = zoo_states(name)
    table = truth_table(_zoo_truth_function(name), states[:n], pars[:n])
    table.setflags(write=False)
    return table


# ---- the host build --------------------------------------------------------------------------------------------------------------
class KinematicsTwin:
    """tests/kinematics_twin.cpp built for the CPU from an artefact's generated headers, contraction off like ``BackgroundTwin`` (so
    that its epsilon_H can be compared bit for bit with the integrator twins')."""

    def __init__(self, artifact, cxx: str = "g++"):
        texts = (artifact._build[0], artifact.eom_header_text(), artifact.kinematics_header_text())
        sources = [os.path.join(CSRC, "inflx_kinematics.h"), os.path.join(HERE, "kinematics_twin.cpp")]
        tag = hashlib.sha1(("".join(texts) + "".join(open(f).read() for f in sources)).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_kinematics_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, kin_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".kin.h", ".so"))
        if not os.path.exists(so):
            for path, text in zip((hdr, eom_hdr, kin_hdr), texts):
                with open(path, "w") as fh:
                    fh.write(text)
            tmp = so + f".{os.getpid()}.tmp"
            cmd = [
                cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas", f"-I{CSRC}",
                f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_KIN_HEADER="{kin_hdr}"', sources[1], "-o", tmp,
            ]  # fmt: skip
            subprocess.run(cmd, check=True)
            os.replace(tmp, so)
        self.lib = C.CDLL(so)
        self.lib.twin_kinematics.argtypes = [_DP, C.c_size_t, _DP, C.c_size_t, C.c_size_t, C.c_size_t, _DP]
        self.lib.twin_kinematics.restype = None
        self.lib.twin_kin_point.argtypes = [_DP, _DP, C.c_size_t, _DP]
        self.lib.twin_kin_point.restype = None

    def kinematics(self, pars, states, traj_len=1):
        """(6, n) at the states (n, ld >= 5); ``pars`` (n_par,) or (n / traj_len, n_par)"""
        p = np.ascontiguousarray(pars, dtype=np.float64)
        y = np.ascontiguousarray(states, dtype=np.float64)
        n, ld = y.shape
        out = np.empty((6, n))
        self.lib.twin_kinematics(p.ctypes.data_as(_DP), 0 if p.ndim == 1 else p.shape[1], y.ctypes.data_as(_DP), n, ld, traj_len, out.ctypes.data_as(_DP))
        return out


# ---- the flat plane in two charts ------------------------------------------------------------------------------------------------
def plane_models():
    """(polar, cartesian): the flat plane as G = diag(1, r^2), V = r^2 (a cos^2 theta + b sin^2 theta) / 2 and as G = 1,
    V = (a X^2 + b Y^2) / 2 -- one geometry and one potential in two charts of the same orientation."""
    from inflatox_amd import InflationModelBuilder

    a, b = sp.symbols("a b")
    r, th = sp.symbols("r theta")
    X, Y = sp.symbols("X Y")
    kw = dict(silent=True, init_sympy_printing=False, simplify=False, assertions=False)
    polar = InflationModelBuilder.new([r, th], [[1, 0], [0, r**2]], r**2 * (a * sp.cos(th) ** 2 + b * sp.sin(th) ** 2) / 2, model_name="plane_polar", **kw).build()
    cart = InflationModelBuilder.new([X, Y], [[1, 0], [0, 1]], (a * X**2 + b * Y**2) / 2, model_name="plane_cartesian", **kw).build()
    return polar, cart


def host_artifact_of(model, cse=False):
    """``background_truth.host_artifact`` for any model: the generated headers and the parameter numbering, no hipcc step."""
    from inflatox_amd import Compiler
    from inflatox_amd.compiler import CompilationArtifact

    comp = Compiler(model, silent=True, cse=cse)
    header = comp._generate_hip_header()
    art = CompilationArtifact(comp.symbol_dict, f"/nonexistent/{model.model_name}.hsaco", 2, len(comp.symbol_dict) - 2, auto_cleanup=False)
    art._build = (header, [], "")
    art._eom_recipe = (model, dict(comp._param_slots), comp.cse, comp.max_cses)
    return art


def plane_states(n=65, seed=5):
    """(polar (n, 5), cartesian (n, 5), a, b): n corresponding states with r in [0.5, 3]; the Cartesian components are computed from
    the polar ones in 40-digit arithmetic and rounded, so that the two float64 states differ by half an ulp per component at most."""
    import mpmath

    rng = np.random.default_rng(seed)
    r, th = rng.uniform(0.5, 3.0, n), rng.uniform(-np.pi, np.pi, n)
    rd, thd = rng.uniform(-0.4, 0.4, n), rng.uniform(-0.4, 0.4, n)
    a, b = 1.3, 0.6
    polar, cart = np.empty((n, 5)), np.empty((n, 5))
    with mpmath.workdps(DPS):
        for k in range(n):
            R, T, Rd, Td = (mpmath.mpf(float(v)) for v in (r[k], th[k], rd[k], thd[k]))
            c, s = mpmath.cos(T), mpmath.sin(T)
            X, Y = R * c, R * s
            Xd, Yd = Rd * c - R * s * Td, Rd * s + R * c * Td
            V = (a * X**2 + b * Y**2) / 2
            H = mpmath.sqrt((V + (Rd**2 + R**2 * Td**2) / 2) / 3)
            polar[k] = [float(v) for v in (R, T, Rd, Td, H)]
            cart[k] = [float(v) for v in (X, Y, Xd, Yd, H)]
    return polar, cart, a, b
