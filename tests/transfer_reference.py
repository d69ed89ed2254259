"""Truths and host twin of the transfer functions (csrc/inflx_transfer.h) -- TEST INFRASTRUCTURE.

Two truths, both scipy's DOP853 at rtol = 1e-12:

* ``plane_truth`` (a), flat charts: the k = 0 field-basis perturbation system on the Cartesian plane with V = (a X^2 + b Y^2) / 2,

      Q''^a + 3 H Q'^a + [V_ab - a^-3 d/dt(a^3 chi_a chi_b / H)] Q^b = 0,

  integrated with the background from initial data on the super-horizon constraint -- Q = n (the unit normal, T turned
  counter-clockwise), d/dt(Q . T) = 2 Omega, i.e. Q' = Omega T + H dq_dN n (``plane_truth``) -- and projected on T and on the
  counter-clockwise normal:
  Q_s = Q . n and R = H Q . T / sigma_dot.  It uses neither omega nor mu_s2, no adiabatic-entropic split and none of the project's
  code.
* ``zoo_truth`` (b), curved zoo: the three equations of csrc/inflx_transfer.h with the Euler-Lagrange right-hand side of
  tests/background_truth.py and omega, mu_s2 from ``masses_reference.truth_expressions`` (the Riemann tensor, the inverse metric, the
  turn rate as |D_t T|), integrated in N so that the samples are met exactly.

``TransferTwin`` compiles tests/transfer_twin.cpp -- the generated headers and csrc/inflx_transfer.h for the CPU, contraction off.

``python tests/transfer_reference.py`` measures the twin's own step-control error against truth (b) -- the worst |twin - truth| over
T_SS and T_RS, 65 lanes, all samples, per model and solver at max_err = 1e-8 and 1e-10 -- and writes it to
profiles/background_transfer.json; ``bound`` is what the tests assert: 1e-10 plus twice that.
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

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "inflatox_amd", "csrc")
PROFILE = os.path.join(ROOT, "profiles", "background_transfer.json")
_DP = C.POINTER(C.c_double)

LANES = 65
MAX_ERRS = (1e-8, 1e-10)
COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW, TARGET = 0, 1, 2, 3, 4, 5


class TwinSolution(NamedTuple):
    """``inflatox_amd.background.TransferSolution``'s members, plus ``accepted`` (B,) and ``final`` (B, 10): y[0..8] and t where each
    lane stopped."""

    T_SS: np.ndarray
    T_RS: np.ndarray
    t: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    states: np.ndarray
    n_stored: np.ndarray
    N_end: np.ndarray
    T_SS_end: np.ndarray
    T_RS_end: np.ndarray
    status: np.ndarray
    accepted: np.ndarray
    final: np.ndarray


# ---- the host build --------------------------------------------------------------------------------------------------------------
class TransferTwin:
    """tests/transfer_twin.cpp built for the CPU from an artefact's generated headers, contraction off like ``MassesTwin``;
    ``contract="fast"`` lets the compiler fuse a*b+c into FMAs as hipcc does for the kernels (``SampledTwin`` has the same switch)."""

    def __init__(self, artifact, cxx: str = "g++", contract: str = "off"):
        texts = (artifact._build[0], artifact.eom_header_text(), artifact.kinematics_header_text(), artifact.masses_header_text())
        sources = [os.path.join(CSRC, "inflx_background.h"), os.path.join(CSRC, "inflx_transfer.h"), os.path.join(HERE, "transfer_twin.cpp")]
        tag = hashlib.sha1(("".join(texts) + "".join(open(f).read() for f in sources) + contract).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_transfer_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, kin_hdr, mass_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".kin.h", ".mass.h", ".so"))
        if not os.path.exists(so):
            for path, text in zip((hdr, eom_hdr, kin_hdr, mass_hdr), texts):
                with open(path, "w") as fh:
                    fh.write(text)
            tmp = so + f".{os.getpid()}.tmp"
            cmd = [
                cxx, "-O2", "-std=c++17", "-fPIC", "-shared", f"-ffp-contract={contract}", *(["-mfma"] if contract != "off" else []), "-fno-fast-math",
                "-Wno-unknown-pragmas", f"-I{CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_KIN_HEADER="{kin_hdr}"',
                f'-DINFLX_MASS_HEADER="{mass_hdr}"', sources[-1], "-o", tmp,
            ]  # fmt: skip
            subprocess.run(cmd, check=True)
            os.replace(tmp, so)
        self.lib = C.CDLL(so)
        self.lib.twin_transfer.argtypes = [_DP, C.c_size_t, _DP, _DP, C.c_size_t, _DP, C.c_uint, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, _DP, _DP]
        self.lib.twin_transfer.restype = None

    def solve(self, pars, samples, fields_init, derivatives_init, max_steps=100_000, max_err=1e-8, solver="rkf", *, dq_dN=None, dt=None, stop_at_end=True):
        """``inflatox_amd.background.transfer_functions``' arguments (checked there, not here) -> ``TwinSolution``"""
        x = np.ascontiguousarray(fields_init, dtype=np.float64)
        init = np.ascontiguousarray(np.concatenate([x, np.asarray(derivatives_init, dtype=np.float64)], axis=1))
        B = init.shape[0]
        p = np.ascontiguousarray(pars, dtype=np.float64)
        pts = np.ascontiguousarray(samples, dtype=np.float64)
        dq = None if dq_dN is None else np.ascontiguousarray(np.broadcast_to(np.asarray(dq_dN, dtype=np.float64), (B,)))
        out = np.empty((pts.size, 10, B))
        lanes = np.empty((B, 16))
        self.lib.twin_transfer(p.ctypes.data_as(_DP), 0 if p.ndim == 1 else p.shape[1], init.ctypes.data_as(_DP), None if dq is None else dq.ctypes.data_as(_DP), B,
                               pts.ctypes.data_as(_DP), pts.size, int(max_steps), 1 if solver == "rkf" else 0, float(max_err), float(dt or 0.0), int(stop_at_end),
                               out.ctypes.data_as(_DP), lanes.ctypes.data_as(_DP))  # fmt: skip
        status = lanes[:, 0].astype(np.int8)
        ended = status == ENDED
        return TwinSolution(out[:, 8].T, out[:, 9].T, out[:, 6].T, out[:, 5].T, out[:, 7].T, out[:, :5].transpose(2, 0, 1), lanes[:, 2].astype(np.uint32),
                            np.where(ended, lanes[:, 1], np.nan), np.where(ended, lanes[:, 3], np.nan), np.where(ended, lanes[:, 4], np.nan), status,
                            lanes[:, 5].astype(np.int64), lanes[:, 6:])  # fmt: skip


@functools.lru_cache(maxsize=None)
def zoo_twin(name):
    import background_truth as bt

    return TransferTwin(bt.host_artifact(name))


LONG_SAMPLES = np.array([0.0, 1.0, 2.0, 3.0])
LONG_MAX_ERR = 1e-12


def long_states(B, seed=1):
    """``hyper_states`` further up the potential, more than three e-folds from the end of inflation: at ``LONG_MAX_ERR`` every lane
    takes more than 256 accepted steps to N = 3"""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(5.2, 5.6, B), rng.uniform(-1, 1, B)], axis=1)
    v = np.stack([rng.uniform(-0.3, -0.1, B), rng.uniform(-4e-4, 4e-4, B)], axis=1)
    return x, v


def hyper_states(B, seed=0):
    """(fields (B, 2), velocities (B, 2)): inflating states of the hyperbolic example model at its parameters (1, 1, 1) -- epsilon_H
    below 0.1 -- that roll towards phi0 = 1 and turn (G_11 theta'^2 is up to a fifth of the kinetic energy): 0.5 to 2.5 e-folds to
    the end of inflation"""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(2.5, 4.0, B), rng.uniform(-1, 1, B)], axis=1)
    v = np.stack([rng.uniform(-0.3, -0.1, B), rng.uniform(-0.004, 0.004, B)], axis=1)
    return x, v


# ---- truth (a): the field-basis system on the Cartesian plane --------------------------------------------------------------------
def plane_truth(state, a, b, dq_dN, times):
    """The k = 0 field-basis system from the Cartesian state (X, Y, Xd, Yd[, H]) with V = (a X^2 + b Y^2) / 2: (len(times), 4) of
    Q_s / Q_s(0) = Q . n, R = H Q . T / sigma_dot (in units of S_star = Q_s(0) / sqrt(2 eps_star): multiply by sigma_dot_star / H_star),
    epsilon_H and N at ``times``.  n is T turned counter-clockwise, (-T_y, T_x).

    Initial data on the super-horizon constraint d/dt(H Q_sigma / sigma_dot) = 2 Omega H Q_s / sigma_dot with Q_sigma = Q . T = 0 and
    Q_s = 1: Q = n; with T' = Omega n and n' = -Omega T, Q' = (Q_sigma' - Omega Q_s) T + (Q_s' + Omega Q_sigma) n = Omega T + q' n,
    q' = H dq_dN.  Omega comes from the turning of the velocity itself, (T_x T_y' - T_y T_x'), not from the project's cross."""
    from scipy.integrate import solve_ivp

    X, Y, Xd, Yd = (float(v) for v in state[:4])
    H0 = math.sqrt(((a * X * X + b * Y * Y) / 2 + (Xd * Xd + Yd * Yd) / 2) / 3)

    def accel(s):
        return -a * s[0] - 3.0 * s[4] * s[2], -b * s[1] - 3.0 * s[4] * s[3]

    def turn(s):  # Omega = T x T' = (chi_x acc_y - chi_y acc_x) / kin
        ax, ay = accel(s)
        return (s[2] * ay - s[3] * ax) / (s[2] * s[2] + s[3] * s[3])

    def f(_t, s):
        x, y, cx, cy, H, _N, qx, qy, px, py = s
        ax, ay = accel(s)
        Hd = -(cx * cx + cy * cy) / 2  # (on the Friedmann constraint; the code integrates V - 3 H^2)
        chi, acc = (cx, cy), (ax, ay)
        # M_ab = V_ab - [3 chi_a chi_b + (acc_a chi_b + chi_a acc_b) / H - chi_a chi_b Hd / H^2]
        M = [[(a if i == 0 else b) * (i == j) - (3.0 * chi[i] * chi[j] + (acc[i] * chi[j] + chi[i] * acc[j]) / H - chi[i] * chi[j] * Hd / (H * H)) for j in range(2)]
             for i in range(2)]  # fmt: skip
        return [cx, cy, ax, ay, Hd, H, px, py, -3.0 * H * px - M[0][0] * qx - M[0][1] * qy, -3.0 * H * py - M[1][0] * qx - M[1][1] * qy]

    s0 = [X, Y, Xd, Yd, H0, 0.0]
    sd = math.hypot(Xd, Yd)
    T, n = (Xd / sd, Yd / sd), (-Yd / sd, Xd / sd)
    Om, qd = turn(s0), H0 * dq_dN
    y0 = [*s0, n[0], n[1], Om * T[0] + qd * n[0], Om * T[1] + qd * n[1]]
    sol = solve_ivp(f, (0.0, float(times[-1])), y0, method="DOP853", rtol=1e-12, atol=1e-14, t_eval=np.asarray(times, dtype=np.float64))
    assert sol.success
    out = np.empty((len(times), 4))
    for k, s in enumerate(sol.y.T):
        kin = s[2] * s[2] + s[3] * s[3]
        sdot = math.sqrt(kin)
        out[k] = [(-s[3] * s[6] + s[2] * s[7]) / sdot, s[4] * (s[2] * s[6] + s[3] * s[7]) / kin * (sd / H0), kin / (2 * s[4] * s[4]), s[5]]
    return out


PLANE_SAMPLES = np.array([0.0, 0.05, 0.2, 0.5])
PLANE_DQ = -0.3


@functools.lru_cache(maxsize=None)
def plane_case(n=17):
    """(polar artefact, Cartesian artefact, polar parameter row, Cartesian parameter row, polar states (n, 5), Cartesian states
    (n, 5), a, b): ``kinematics_reference.plane_states`` and the host artefacts of its two charts"""
    import kinematics_reference as kr
    import masses_reference as mr

    polar, cart = kr.plane_models()
    pa, ca = kr.host_artifact_of(polar), kr.host_artifact_of(cart)
    ps, cs, a, b = kr.plane_states(n)
    return pa, ca, mr.parameter_row(pa, a=a, b=b), mr.parameter_row(ca, a=a, b=b), ps, cs, a, b


def plane_error(sol, states, a, b, dq_dN=PLANE_DQ):
    """worst |T_SS - truth (a)|, |T_RS - truth (a)| of a solution at PLANE_SAMPLES from the Cartesian ``states``, the truth read at
    the times the solution located the samples at (the solution's own error in t is part of what is measured)"""
    worst = 0.0
    for k in range(states.shape[0]):
        tr = plane_truth(states[k], a, b, dq_dN, sol.t[k, 1:])
        eps_star = (states[k, 2] ** 2 + states[k, 3] ** 2) / (2 * states[k, 4] ** 2)
        t_ss = tr[:, 0] * np.sqrt(eps_star / tr[:, 2])
        worst = max(worst, float(np.abs(sol.T_SS[k, 1:] - t_ss).max()), float(np.abs(sol.T_RS[k, 1:] - tr[:, 1]).max()))
    return worst


def long_bound(solver):
    """``bound`` for the long run on the hyperbolic model (``long_states``)"""
    return 1e-10 + 2.0 * recorded()["hyperbolic"][f"{solver}/{LONG_MAX_ERR:g}"]


def plane_bound(solver, max_err):
    """``bound`` for truth (a): 1e-10 plus twice the host twin's recorded worst error on the Cartesian plane"""
    return 1e-10 + 2.0 * recorded()["plane"][f"{solver}/{max_err:g}"]


# ---- truth (b): the three equations on the curved zoo ----------------------------------------------------------------------------
def truth_rhs(model, slots):
    """g(x0, x1, xd0, xd1, H, p) -> (eom^0, eom^1, V, kin, eps_H, omega, mu_s2) in float64: the Euler-Lagrange derivation and the
    truth expressions of the masses, parameters in the slots of ``CompilationArtifact.symbol_dictionary``"""
    import sympy as sp
    from sympy.printing.c import C99CodePrinter

    import background_truth as bt
    import kinematics_reference as kr
    import masses_reference as mr

    eom, V, kin = bt._derivation(model)
    tr = mr.truth_expressions(model.coordinates, model.metric, model.potential, model.coordinate_tangents)
    exprs = [sp.sympify(e) for e in (*eom, V, kin, tr[4], tr[5], tr[7])]
    plain = C99CodePrinter()._print_Symbol
    fixed = [*model.coordinates, *model.coordinate_tangents, kr._H]
    free = sorted(set().union(*[e.free_symbols for e in exprs]) - set(fixed), key=lambda s: int(slots[plain(s)][5:-1]))
    idx = [int(slots[plain(s)][5:-1]) for s in free]
    fn = sp.lambdify([*fixed, *free], exprs, modules="math", cse=True)
    return lambda x0, x1, v0, v1, H, p: fn(x0, x1, v0, v1, H, *[p[k] for k in idx])


@functools.lru_cache(maxsize=None)
def _zoo_rhs(name):
    import background_truth as bt

    return truth_rhs(bt.zoo_model(name).model, bt.host_artifact(name).symbol_dictionary)


@functools.lru_cache(maxsize=None)
def workload_rhs(name):
    """``truth_rhs`` of an example model of ``workloads``"""
    import workloads

    return truth_rhs(workloads.model_for(name), workloads.artifact_for(name)[1].symbol_dictionary)


def default_dq_dN(eps, mu):
    """the documented default: the slowly decaying root of lambda^2 + (3 - eps) lambda + mu = 0, its real part when complex"""
    b1 = 3.0 - eps
    disc = b1 * b1 - 4.0 * mu
    return 0.5 * (math.sqrt(disc) - b1) if disc >= 0.0 else -0.5 * b1


def truth_lane(g, init, p, samples, dq_dN=None, to_end=False):
    """(S, 4): T_SS, T_RS, eps_H and t at the e-fold counts ``samples`` (> 0) of the trajectory from ``init`` (4,) with parameter row
    ``p`` and the model functions ``g`` (``truth_rhs``): y = (phi, chi, H, t, q, u, r) integrated in N (H > 0 along the trajectory).
    ``to_end``: the integration stops at epsilon_H = 1 (an event, located by DOP853's dense output), the samples after it are NaN,
    and (N_end, T_SS_end, T_RS_end) is returned as well."""
    from scipy.integrate import solve_ivp

    V, kin = g(*init, 1.0, p)[2:4]
    H0 = math.sqrt((V + 0.5 * kin) / 3.0)
    _, _, _, _, eps_star, _om, mu = g(*init, H0, p)
    dq = default_dq_dN(eps_star, mu) if dq_dN is None else float(dq_dN)

    def f(_N, s):
        e0, e1, V, _k, eps, om, mu2 = g(s[0], s[1], s[2], s[3], s[4], p)
        H = s[4]
        return [s[2] / H, s[3] / H, (-e0 - 3.0 * H * s[2]) / H, (-e1 - 3.0 * H * s[3]) / H, (V - 3.0 * H * H) / H, 1.0 / H,
                s[7] / H, -3.0 * s[7] - H * mu2 * s[6], 2.0 * om * s[6] * math.sqrt(eps_star / eps)]  # fmt: skip

    def end(_N, s):
        return g(s[0], s[1], s[2], s[3], s[4], p)[4] - 1.0

    end.terminal = True
    pts = np.asarray(samples, dtype=np.float64)
    y0 = [*map(float, init), H0, 0.0, 1.0, H0 * dq, 0.0]
    sol = solve_ivp(f, (0.0, float(pts[-1])), y0, method="DOP853", rtol=1e-12, atol=1e-14, t_eval=pts, events=end if to_end else None)
    assert sol.success and (to_end or sol.y.shape[1] == pts.size)
    out = np.full((pts.size, 4), np.nan)
    for k, s in enumerate(np.asarray(sol.y).reshape(9, -1).T):
        eps = g(s[0], s[1], s[2], s[3], s[4], p)[4]
        out[k] = [s[6] * math.sqrt(eps_star / eps), s[8], eps, s[5]]
    if not to_end:
        return out
    assert sol.status == 1, "the trajectory did not reach epsilon_H = 1 before the last sample"
    s = sol.y_events[0][0]
    return out, (float(sol.t_events[0][0]), s[6] * math.sqrt(eps_star), s[8])


def truth_final(g, init, p, t_end, dq_dN=None):
    """(q, u, r) at the time ``t_end`` of the trajectory from ``init`` (4,): the three equations integrated in t, DOP853 at rtol 1e-13"""
    from scipy.integrate import solve_ivp

    V, kin = g(*init, 1.0, p)[2:4]
    H0 = math.sqrt((V + 0.5 * kin) / 3.0)
    eps_star, _om, mu = g(*init, H0, p)[4:]
    dq = default_dq_dN(eps_star, mu) if dq_dN is None else float(dq_dN)

    def f(_t, s):
        e0, e1, V, _k, eps, om, mu2 = g(s[0], s[1], s[2], s[3], s[4], p)
        H = s[4]
        return [s[2], s[3], -e0 - 3.0 * H * s[2], -e1 - 3.0 * H * s[3], V - 3.0 * H * H, s[6], -3.0 * H * s[6] - H * H * mu2 * s[5],
                2.0 * om * H * s[5] * math.sqrt(eps_star / eps)]  # fmt: skip

    sol = solve_ivp(f, (0.0, float(t_end)), [*map(float, init), H0, 1.0, H0 * dq, 0.0], method="DOP853", rtol=1e-13, atol=1e-15)
    assert sol.success
    return sol.y[5:, -1]


def end_truth(g, init, p, dN, dq_dN=None):
    """((N_end, T_SS_end, T_RS_end) of the truth, (bound on |T_SS_end - truth|, bound on |T_RS_end - truth|)) for end values that are
    linear across a last step of at most ``dN`` e-folds.  Linear interpolation of a function f over an interval of length dN is
    within dN^2 / 8 max|f''| of it; the fraction of the step comes from the same interpolation of epsilon_H, which misplaces N_end by
    at most dN^2 / 8 max|eps''| / min|eps'| and the end value by max|f'| times that.  The derivatives are taken from the truth on
    [N_end - dN, N_end + dN] by differences; the bound is twice the sum (the step's ends carry the integration error, far below),
    plus 1e-8."""
    from scipy.integrate import solve_ivp

    _out, (n_end, ss_end, rs_end) = truth_lane(g, init, p, [1e3], dq_dN, to_end=True)
    V, kin = g(*init, 1.0, p)[2:4]
    H0 = math.sqrt((V + 0.5 * kin) / 3.0)
    eps_star, _om, mu = g(*init, H0, p)[4:]
    dq = default_dq_dN(eps_star, mu) if dq_dN is None else float(dq_dN)

    def f(_N, s):
        e0, e1, V, _k, eps, om, mu2 = g(s[0], s[1], s[2], s[3], s[4], p)
        H = s[4]
        return [s[2] / H, s[3] / H, (-e0 - 3.0 * H * s[2]) / H, (-e1 - 3.0 * H * s[3]) / H, (V - 3.0 * H * H) / H, 1.0 / H,
                s[7] / H, -3.0 * s[7] - H * mu2 * s[6], 2.0 * om * s[6] * math.sqrt(eps_star / eps)]  # fmt: skip

    grid = np.linspace(max(0.0, n_end - dN), n_end + dN, 81)
    sol = solve_ivp(f, (0.0, grid[-1]), [*map(float, init), H0, 0.0, 1.0, H0 * dq, 0.0], method="DOP853", rtol=1e-12, atol=1e-14, t_eval=grid)
    assert sol.success
    eps = np.array([g(s[0], s[1], s[2], s[3], s[4], p)[4] for s in sol.y.T])
    h = grid[1] - grid[0]
    d1 = lambda v: np.gradient(v, h)  # noqa: E731
    bounds = []
    for v in (sol.y[6] * math.sqrt(eps_star), sol.y[8]):
        shift = np.abs(d1(d1(eps))).max() / np.abs(d1(eps)).min()
        bounds.append(2.0 * dN * dN / 8.0 * (np.abs(d1(d1(v))).max() + np.abs(d1(v)).max() * shift) + 1e-8)
    return (n_end, ss_end, rs_end), tuple(bounds)


def zoo_truth_lane(name, init, p, samples, dq_dN=None):
    return truth_lane(_zoo_rhs(name), init, p, samples, dq_dN)


@functools.lru_cache(maxsize=None)
def zoo_truth(name, n_lanes=LANES):
    """(samples (4,), truth (n_lanes, 4, 4)): ``zoo_truth_lane`` with the default dq_dN of the first lanes of
    ``background_truth.batch(name)`` at ``background_truth.samples_for(name, "N")``: computed once and shared."""
    import background_truth as bt

    init, pars = bt.batch(name)
    samples = np.asarray(bt.samples_for(name, "N"))
    truth = np.array([zoo_truth_lane(name, init[k], pars[k], samples) for k in range(n_lanes)])
    truth.setflags(write=False)
    return samples, truth


def zoo_error(sol, truth):
    """worst |T_SS - truth|, |T_RS - truth| over the lanes and samples of ``zoo_truth``"""
    return float(max(np.max(np.abs(sol.T_SS - truth[:, :, 0])), np.max(np.abs(sol.T_RS - truth[:, :, 1]))))


# ---- the recorded step-control error and the bound -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stepper_code_hash():
    """the hash of the code (comments aside) of the two headers that make the stepper: the state of the code a profile belongs to"""
    from inflatox_amd.compiler import _code_only

    h = hashlib.sha256()
    for f in ("inflx_background.h", "inflx_transfer.h"):
        with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
            h.update(_code_only(fh.read()).encode())
    return h.hexdigest()[:16]


def recorded():
    with open(PROFILE) as fh:
        return json.load(fh)


def bound(name, solver, max_err):
    """what |T - truth (b)| may be: 1e-10 plus twice the host twin's recorded worst error for this model, solver and max_err -- a
    margin for other libm and contraction choices, not for defects"""
    return 1e-10 + 2.0 * recorded()["zoo"][f"{name}/{solver}/{max_err:g}"]


def measure():
    import background_truth as bt

    zoo = {}
    for name in bt.GPU_MODELS:
        init, pars = (v[:LANES] for v in bt.batch(name))
        samples, truth = zoo_truth(name)
        assert np.isfinite(truth).all()
        for solver in ("rk4", "rkf"):
            for max_err in MAX_ERRS:
                sol = zoo_twin(name).solve(pars, samples, init[:, :2], init[:, 2:], max_err=max_err, solver=solver, stop_at_end=False)
                assert np.all(sol.status == TARGET), (name, solver, max_err)
                zoo[f"{name}/{solver}/{max_err:g}"] = zoo_error(sol, truth)
                print(f"{name} {solver} max_err {max_err:g}: worst |twin - truth| {zoo[f'{name}/{solver}/{max_err:g}']:.3e}", flush=True)
    _pa, ca, _pp, cp, _ps, cs, a, b = plane_case()
    plane = {}
    for solver in ("rk4", "rkf"):
        for max_err in MAX_ERRS:
            sol = TransferTwin(ca).solve(cp, PLANE_SAMPLES, cs[:, :2], cs[:, 2:4], max_err=max_err, solver=solver, dq_dN=PLANE_DQ, stop_at_end=False)
            assert np.all(sol.status == TARGET)
            plane[f"{solver}/{max_err:g}"] = plane_error(sol, cs, a, b)
            print(f"plane {solver} max_err {max_err:g}: worst |twin - truth (a)| {plane[f'{solver}/{max_err:g}']:.3e}", flush=True)
    import workloads

    spec, art = workloads.artifact_for("hyperbolic")
    g = workload_rhs("hyperbolic")
    x, v = long_states(33)
    truth = np.array([truth_lane(g, [*x[k], *v[k]], spec.args, LONG_SAMPLES[1:]) for k in range(33)])
    hyper = {}
    for solver in ("rk4", "rkf"):
        sol = TransferTwin(art).solve(spec.args, LONG_SAMPLES, x, v, max_err=LONG_MAX_ERR, solver=solver)
        assert np.all(sol.status == TARGET) and sol.accepted.min() > 256, sol.accepted.min()
        hyper[f"{solver}/{LONG_MAX_ERR:g}"] = float(max(np.abs(sol.T_SS[:, 1:] - truth[:, :, 0]).max(), np.abs(sol.T_RS[:, 1:] - truth[:, :, 1]).max()))
        print(f"hyperbolic {solver}: {sol.accepted.min()} .. {sol.accepted.max()} steps, worst |twin - truth (b)| {hyper[f'{solver}/{LONG_MAX_ERR:g}']:.3e}", flush=True)
    doc = {
        "stepper_code": stepper_code_hash(),
        "hyperbolic": hyper,
        "hyperbolic_what": "worst |host twin - truth (b)| over T_SS and T_RS at N = 1, 2, 3, the first 33 lanes of transfer_reference.long_states on the "
                           "hyperbolic example model, default dq_dN; every lane takes more than 256 accepted steps",
        "plane": plane,
        "plane_what": "worst |host twin - truth (a)| over T_SS and T_RS, 17 states of kinematics_reference.plane_states on the Cartesian plane, "
                      "samples N = 0.05, 0.2, 0.5, dq_dN = -0.3, stop_at_end off; truth: the k = 0 field-basis system, DOP853 at rtol 1e-12",
        "what": "worst |host twin - truth (b)| over T_SS and T_RS, 65 lanes x 4 samples of background_truth.batch, default dq_dN, stop_at_end off; "
                "truth: DOP853 in N at rtol 1e-12 (tests/transfer_reference.py)",
        "bound": "tests assert 1e-10 + 2 x the value recorded here",
        "zoo": zoo,
    }  # fmt: skip
    return doc


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    result = measure()
    if os.path.exists(PROFILE):
        with open(PROFILE) as fh:
            old = json.load(fh)
        result = {**old, **result}
    with open(PROFILE, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
