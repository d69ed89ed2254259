"""Truth and host twin of the entropic masses (csrc/inflx_masses.h) -- TEST INFRASTRUCTURE.

``truth_masses`` evaluates the eight quantities of ``inflatox_amd.background.masses`` in 40-digit arithmetic by routes the code does
not take:

* h(v) = V_;ab v^a v^b from the Euler-Lagrange connection of tests/background_truth.py: the vector (d_a G_cb - d_c G_ab / 2) v^a v^b
  solved for Gamma^d_ab v^a v^b by LU decomposition -- no Christoffel symbol of inflatox_amd.symbolic, no inverse metric;
* V_TN by polarisation, [h(chi + n) - h(chi - n)] / 4;
* the normal through the inverse metric, n^a = G^ab n_b with n_b = sqrt(det G) eps_bc chi^c;
* R from the full Riemann tensor R^a_bcd = d_c Gamma^a_bd - d_d Gamma^a_bc + Gamma^a_ce Gamma^e_bd - Gamma^a_de Gamma^e_bc of
  Christoffel symbols formed here, contracted with the inverse metric;
* the trace G^ab V_;ab from the Laplace-Beltrami divergence form (1 / sqrt g) d_a (sqrt g G^ab d_b V);
* eps_H and omega from tests/kinematics_reference.py (omega as |D_t T|_G with the sign of its projection on N).

The code forms V_;ab from first-kind symbols and the adjugate, contracts it with chi and eps^be chi_e / sqrt(det G), and takes R
from 2 R_0101 / det G with R_0101 written in second derivatives of the metric and products of first-kind symbols.

``allowance`` is the bound the masses issue sets: the project's parity bar, 1e-10, applied to the sum of the absolute values of the
terms a quantity is built from, as ``kinematics_reference.allowance`` does it.  The terms: of V_XY the |d_a d_b V u^a w^b| and
|Gamma^c_ab d_c V u^a w^b| over all index values, divided by kin; of R the |G^bd| times every |d Gamma| and |Gamma Gamma| of the
Ricci tensor; of eps_H itself; of omega the kinematics' S / (sigma_dot |H|), S = |dV|_G; of M_eff2 and mu_s2 the three terms
V_NN / H^2 (the terms of V_NN over H^2), eps_H R (eps_H times the terms of R) and omega^2 or 3 omega^2 (the square of omega's).

``MassesTwin`` compiles tests/masses_twin.cpp -- the generated headers and csrc/inflx_masses.h for the CPU.  ``zoo_truth`` is the
truth at ``kinematics_reference.zoo_states``, computed once and shared by the CPU and the GPU tests.
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
import kinematics_reference as kr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "inflatox_amd", "csrc")
_DP = C.POINTER(C.c_double)

NAMES = ("V_TT", "V_TN", "V_NN", "ricci", "eps_H", "omega", "M_eff2", "mu_s2")
RTOL = kr.RTOL  # the project's parity bar
DPS = kr.DPS
_H = kr._H
# columns of a truth table: the eight quantities, then ...
TRACE, S_TT, S_TN, S_NN, S_R, S2, SIGMA_DOT = 8, 9, 10, 11, 12, 13, 14


# ---- the truth -------------------------------------------------------------------------------------------------------------------
def truth_expressions(fields, metric, potential, tangents):
    """[the eight quantities, the Laplace-Beltrami trace, the term sizes of V_TT, V_TN, V_NN and R, S^2 = |dV|^2_G, sigma_dot] as
    sympy expressions of the fields, the velocities, the parameters and the Hubble rate."""
    n = len(fields)
    G = sp.Matrix(n, n, lambda a, b: sp.sympify(metric[a][b]))
    Ginv = G.inv()
    V = sp.sympify(potential)
    chi = list(tangents)
    dV = [sp.diff(V, f) for f in fields]
    kin = sum(G[a, b] * chi[a] * chi[b] for a in range(n) for b in range(n))

    def h(v):  # V_;ab v^a v^b, the connection term from the Euler-Lagrange form
        force = [sum((sp.diff(G[c, b], fields[a]) - sp.diff(G[a, b], fields[c]) / 2) * v[a] * v[b] for a in range(n) for b in range(n)) for c in range(n)]
        conn = G.LUsolve(sp.Matrix(force))  # Gamma^d_ab v^a v^b
        return sum(sp.diff(V, fields[a], fields[b]) * v[a] * v[b] for a in range(n) for b in range(n)) - sum(conn[c] * dV[c] for c in range(n))

    root = sp.sqrt(G.det())
    n_low = [root * chi[1], -root * chi[0]]  # n_a = sqrt(det G) eps_ab chi^b
    nv = [sum(Ginv[a, b] * n_low[b] for b in range(n)) for a in range(n)]
    v_tt = h(chi) / kin
    v_nn = h(nv) / kin
    v_tn = (h([chi[a] + nv[a] for a in range(n)]) - h([chi[a] - nv[a] for a in range(n)])) / (4 * kin)
    gamma = [[[sum(Ginv[a, d] * (sp.diff(G[d, b], fields[c]) + sp.diff(G[d, c], fields[b]) - sp.diff(G[b, c], fields[d])) for d in range(n)) / 2
               for c in range(n)] for b in range(n)] for a in range(n)]  # fmt: skip

    def riemann(a, b, c, d):
        return (sp.diff(gamma[a][b][d], fields[c]) - sp.diff(gamma[a][b][c], fields[d])
                + sum(gamma[a][c][e] * gamma[e][b][d] - gamma[a][d][e] * gamma[e][b][c] for e in range(n)))  # fmt: skip

    ricci = sum(Ginv[b, d] * riemann(a, b, a, d) for a in range(n) for b in range(n) for d in range(n))
    trace = sum(sp.diff(root * sum(Ginv[a, b] * dV[b] for b in range(n)), fields[a]) for a in range(n)) / root
    kin_truth = kr.truth_expressions(fields, metric, potential, tangents)
    eps, omega, s2, sigma_dot = kin_truth[0], kin_truth[2], kin_truth[6], kin_truth[3]
    m_eff2 = v_nn / _H**2 + eps * ricci - omega**2
    mu_s2 = v_nn / _H**2 + eps * ricci + 3 * omega**2

    def size(u, w):  # the terms of V_;ab u^a w^b / kin
        return sum(sp.Abs(u[a]) * sp.Abs(w[b]) * (sp.Abs(sp.diff(V, fields[a], fields[b])) + sum(sp.Abs(gamma[c][a][b] * dV[c]) for c in range(n)))
                   for a in range(n) for b in range(n)) / kin  # fmt: skip

    size_r = sum(
        sp.Abs(Ginv[b, d]) * (sp.Abs(sp.diff(gamma[a][b][d], fields[a])) + sp.Abs(sp.diff(gamma[a][b][a], fields[d]))
                              + sum(sp.Abs(gamma[a][a][e] * gamma[e][b][d]) + sp.Abs(gamma[a][d][e] * gamma[e][b][a]) for e in range(n)))
        for a in range(n) for b in range(n) for d in range(n)
    )  # fmt: skip
    return [v_tt, v_tn, v_nn, ricci, eps, omega, m_eff2, mu_s2, trace, size(chi, chi), size(chi, nv), size(nv, nv), size_r, s2, sigma_dot]


def truth_function(fields, metric, potential, tangents, param_slots=None):
    """f(y (5,), p) -> the fifteen values of ``truth_expressions`` at the float64 state y and parameter row p, evaluated at ``DPS``
    digits, as mpf.  ``param_slots`` as for ``background_truth.point_function``."""
    import mpmath
    from sympy.printing.c import C99CodePrinter

    exprs = [sp.sympify(e) for e in truth_expressions(fields, metric, potential, tangents)]
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
            return [+mpmath.mpf(v) for v in fn(*[mpmath.mpf(float(v)) for v in y], *[mpmath.mpf(float(p[slot[s]])) for s in params])]

    return f


def model_truth_function(model, artifact):
    return truth_function(model.coordinates, model.metric, model.potential, model.coordinate_tangents, artifact.symbol_dictionary)


def truth_table(f, states, pars):
    """(n, 15) float64 of ``truth_function`` f over the states (n, 5), parameter rows (n, n_par) or one row (n_par,)."""
    pars = np.asarray(pars)
    return np.array([[float(v) for v in f(states[k], pars[k] if pars.ndim == 2 else pars)] for k in range(states.shape[0])])


def allowance(truth, H):
    """(8, n): the largest |got - truth| allowed for each quantity (module docstring); ``truth`` (n, 15) from ``truth_table``,
    ``H`` (n,)."""
    H2 = np.asarray(H) ** 2
    eps = truth[:, 4]
    ratio = np.sqrt(truth[:, S2]) / (truth[:, SIGMA_DOT] * np.abs(H))
    base = truth[:, S_NN] / H2 + eps * truth[:, S_R]
    return RTOL * np.stack([truth[:, S_TT], truth[:, S_TN], truth[:, S_NN], truth[:, S_R], eps, ratio, base + ratio**2, base + 3.0 * ratio**2])


def worst_ratios(got, truth, H):
    """{quantity: max |got - truth| / allowance}; ``got`` (8, n).  A quantity whose terms all vanish (R of a flat metric in flat
    coordinates) has allowance 0 and must be met exactly: its ratio is 0 then and infinite otherwise."""
    err = np.abs(np.asarray(got) - truth[:, :8].T)
    allow = allowance(truth, H)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / allow)
    return {name: float(r[q].max()) for q, name in enumerate(NAMES)}


# ---- the states the CPU and the GPU tests share ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _zoo_truth_function(name):
    return model_truth_function(bt.zoo_model(name).model, bt.host_artifact(name))


@functools.lru_cache(maxsize=None)
def zoo_truth(name, n):
    """``truth_table`` of the first n states of ``kinematics_reference.zoo_states(name)``: computed once and shared."""
    states, pars = kr.zoo_states(name)
    table = truth_table(_zoo_truth_function(name), states[:n], pars[:n])
    table.setflags(write=False)
    return table


# ---- the host build --------------------------------------------------------------------------------------------------------------
class MassesTwin:
    """tests/masses_twin.cpp built for the CPU from an artefact's generated headers, contraction off like ``KinematicsTwin`` (so that
    its eps_H and omega can be compared bit for bit with that twin's)."""

    def __init__(self, artifact, cxx: str = "g++"):
        texts = (artifact._build[0], artifact.eom_header_text(), artifact.kinematics_header_text(), artifact.masses_header_text())
        sources = [os.path.join(CSRC, "inflx_masses.h"), os.path.join(HERE, "masses_twin.cpp")]
        tag = hashlib.sha1(("".join(texts) + "".join(open(f).read() for f in sources)).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_masses_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, kin_hdr, mass_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".kin.h", ".mass.h", ".so"))
        if not os.path.exists(so):
            for path, text in zip((hdr, eom_hdr, kin_hdr, mass_hdr), texts):
                with open(path, "w") as fh:
                    fh.write(text)
            tmp = so + f".{os.getpid()}.tmp"
            cmd = [
                cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas", f"-I{CSRC}",
                f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_KIN_HEADER="{kin_hdr}"', f'-DINFLX_MASS_HEADER="{mass_hdr}"',
                sources[1], "-o", tmp,
            ]  # fmt: skip
            subprocess.run(cmd, check=True)
            os.replace(tmp, so)
        self.lib = C.CDLL(so)
        self.lib.twin_masses.argtypes = [_DP, C.c_size_t, _DP, C.c_size_t, C.c_size_t, C.c_size_t, _DP]
        self.lib.twin_masses.restype = None
        self.lib.twin_mass_point.argtypes = [_DP, _DP, C.c_size_t, _DP]
        self.lib.twin_mass_point.restype = None

    def masses(self, pars, states, traj_len=1):
        """(8, n) at the states (n, ld >= 5); ``pars`` (n_par,) or (n / traj_len, n_par)"""
        p = np.ascontiguousarray(pars, dtype=np.float64)
        y = np.ascontiguousarray(states, dtype=np.float64)
        n, ld = y.shape
        out = np.empty((8, n))
        self.lib.twin_masses(p.ctypes.data_as(_DP), 0 if p.ndim == 1 else p.shape[1], y.ctypes.data_as(_DP), n, ld, traj_len, out.ctypes.data_as(_DP))
        return out

    def mass_point(self, pars, points):
        """(n, 4): inflx_mass_point's o[0..3] at the points (n, 4) = (x0, x1, xd0, xd1), one parameter row for all"""
        p = np.ascontiguousarray(pars, dtype=np.float64)
        pts = np.ascontiguousarray(points, dtype=np.float64)
        out = np.empty((pts.shape[0], 4))
        self.lib.twin_mass_point(p.ctypes.data_as(_DP), pts.ctypes.data_as(_DP), pts.shape[0], out.ctypes.data_as(_DP))
        return out


# ---- models with known answers ---------------------------------------------------------------------------------------------------
def sphere_model():
    """A sphere of radius r in the chart (x0, x1) = (polar angle, azimuth), G = diag(r^2, r^2 sin^2 x0), with a potential that
    depends on both angles: R = 2 / r^2."""
    from inflatox_amd import InflationModelBuilder

    r, a = sp.symbols("r a")
    u, w = sp.symbols("u w")
    kw = dict(silent=True, init_sympy_printing=False, simplify=False, assertions=False)
    return InflationModelBuilder.new([u, w], [[r**2, 0], [0, r**2 * sp.sin(u) ** 2]], a * (2 + sp.cos(u) + sp.sin(u) * sp.cos(w) / 2), model_name="sphere", **kw).build()


def parameter_row(artifact, **values):
    """the artefact's parameter row with the named parameters set"""
    p = np.zeros(artifact.n_parameters)
    for name, value in values.items():
        p[int(artifact.symbol_dictionary[name][5:-1])] = value
    return p


# ---- the doc model along its gradient ---------------------------------------------------------------------------------------------
def doc_gradient_states(n_side=4):
    """(states (n_side^2, 5), points (n_side^2, 2)) of the doc model (m = 1): points inside (0, 2.5) x (0, pi) away from the axes,
    chi = -G^ab d_b V there and H from the Friedmann constraint, in 40-digit arithmetic and rounded.  There T = -v, the sweeps'
    first basis vector, so that V_TT = v00, V_NN = v11 and V_TN = +-v10."""
    import mpmath
    from workloads import example_models

    spec = example_models.get("doc")
    r, th = spec.fields
    (m,) = sorted(sp.sympify(spec.potential).free_symbols - {r, th}, key=str)
    V = sp.sympify(spec.potential).subs(m, 1)
    G = sp.Matrix(spec.metric)
    grad_up = G.inv() * sp.Matrix([sp.diff(V, r), sp.diff(V, th)])
    kin = (grad_up.T * G * grad_up)[0]
    fn = sp.lambdify([r, th], [-grad_up[0], -grad_up[1], sp.sqrt((V + kin / 2) / 3)], modules="mpmath")
    pts = np.array([[rr, tt] for rr in np.linspace(0.6, 2.2, n_side) for tt in np.linspace(0.4, 2.8, n_side)])
    with mpmath.workdps(DPS):
        rest = np.array([[float(v) for v in fn(mpmath.mpf(float(a)), mpmath.mpf(float(b)))] for a, b in pts])
    return np.concatenate([pts, rest], axis=1), pts
