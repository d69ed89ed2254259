"""Truths and host twin of the mode functions and power spectra (csrc/inflx_modes.h) -- TEST INFRASTRUCTURE.

Three truths, all scipy's DOP853 at rtol = 1e-12:

* ``plane_truth`` (a), flat charts: the field-basis perturbation system on the Cartesian plane with V = (a X^2 + b Y^2) / 2,

      Q''^a + 3 H Q'^a + (k^2 / a^2) Q^a + [V_ab - a^-3 d/dt(a^3 chi_a chi_b / H)] Q^b = 0,

  complex, two solutions with Q^I_a = delta_Ia and Q'^I = (-i k / a - H) Q^I, projected on T and on e_s = T turned counter-clockwise
  at the evaluation point.  The sum over an orthonormal pair of initial conditions does not depend on the pair, so P_R, P_S and C_RS
  must be the project's.  It uses neither Omega nor any mass, no adiabatic-entropic split and none of the project's code.
* ``truth_lane`` (b), curved zoo: the four equations of csrc/inflx_modes.h with the Euler-Lagrange right-hand side of
  tests/background_truth.py and the coefficients from ``masses_reference.truth_expressions`` and
  ``kinematics_reference.truth_expressions`` (the Riemann tensor, the inverse metric), integrated in N so that the target is met
  exactly.
* ``power_law_formula`` (c), exact: power-law inflation a ~ t^p, p = 8, eps = 1 / p, nu = 3/2 + eps / (1 - eps):
  P_R = [2^(nu - 3/2) Gamma(nu) / Gamma(3/2)]^2 (1 - eps)^(2 nu - 1) H_k^2 / (8 pi^2 eps) on super-horizon scales.

``ModesTwin`` compiles tests/modes_twin.cpp -- the generated headers and csrc/inflx_modes.h for the CPU, contraction off.
``ModesTwin.power_spectra`` is ``inflatox_amd.background.power_spectra`` on the host: its stage 1 from ``SampledTwin`` (or from a
``SampledSolution`` handed in), its stage 2 from the twin.

Errors are relative to each spectrum's own scale: |dP_R| / P_R, |dP_S| / P_S and |dC_RS| / sqrt(P_R P_S) of the truth.

``python tests/modes_reference.py`` measures the twin's own step-control error against truths (a) and (b) -- per model and solver at
max_err = 1e-8 and 1e-10 -- and the error that a start at a finite N_sub leaves against (c), and writes them to
profiles/background_modes.json; ``bound`` is what the tests assert: 1e-10 plus twice that.
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
PROFILE = os.path.join(ROOT, "profiles", "background_modes.json")
_DP = C.POINTER(C.c_double)

LANES = 65
MAX_ERRS = (1e-8, 1e-10)
N_SUB = 3.0  # the lane-level truths start their modes at kappa = H0 e^N_SUB
COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW, TARGET = 0, 1, 2, 3, 4, 5


class TwinLanes(NamedTuple):
    """What ``ModesTwin.lanes`` returns: ``out`` (22, n) as ``InflatoxDevLib.mode_spectra``'s, ``N_end`` (n,) as the kernel leaves it,
    ``status`` (n,), ``accepted`` (n,) steps and ``final`` (n, 23): y[0..21] and t where each lane stopped (never a located state)."""

    out: np.ndarray
    N_end: np.ndarray
    status: np.ndarray
    accepted: np.ndarray
    final: np.ndarray


class TwinSpectra(NamedTuple):
    """``inflatox_amd.background.PowerSpectra``'s members, plus ``accepted`` (B, K)"""

    P_R: np.ndarray
    P_S: np.ndarray
    C_RS: np.ndarray
    k: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    modes: np.ndarray
    N_end: np.ndarray
    status: np.ndarray
    accepted: np.ndarray


# ---- the host build --------------------------------------------------------------------------------------------------------------
class ModesTwin:
    """tests/modes_twin.cpp built for the CPU from an artefact's generated headers, contraction off like ``TransferTwin``"""

    def __init__(self, artifact, cxx: str = "g++", contract: str = "off"):
        self.artifact = artifact
        texts = (artifact._build[0], artifact.eom_header_text(), artifact.kinematics_header_text(), artifact.masses_header_text())
        sources = [os.path.join(CSRC, "inflx_background.h"), os.path.join(CSRC, "inflx_modes.h"), os.path.join(HERE, "modes_twin.cpp")]
        tag = hashlib.sha1(("".join(texts) + "".join(open(f).read() for f in sources) + contract).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_modes_twin")
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
        self.lib.twin_modes.argtypes = [_DP, C.c_size_t, _DP, _DP, _DP, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, _DP, _DP]
        self.lib.twin_modes.restype = None

    def lanes(self, pars, init, kappa, n_target, max_steps=1_000_000, max_err=1e-8, solver="rkf", *, dt=None, stop_at_end=True) -> TwinLanes:
        """``InflatoxDevLib.mode_spectra``'s arguments: init (n, 4), kappa (n,), n_target (n,) (NaN: none)"""
        init = np.ascontiguousarray(init, dtype=np.float64)
        n = init.shape[0]
        p = np.ascontiguousarray(pars, dtype=np.float64)
        kappa = np.ascontiguousarray(np.broadcast_to(np.asarray(kappa, dtype=np.float64), (n,)))
        target = np.ascontiguousarray(np.broadcast_to(np.asarray(n_target, dtype=np.float64), (n,)))
        out = np.empty((22, n))
        lanes = np.empty((n, 26))
        self.lib.twin_modes(p.ctypes.data_as(_DP), 0 if p.ndim == 1 else p.shape[1], init.ctypes.data_as(_DP), kappa.ctypes.data_as(_DP), target.ctypes.data_as(_DP), n,
                            int(max_steps), 1 if solver == "rkf" else 0, float(max_err), float(dt or 0.0), int(stop_at_end), out.ctypes.data_as(_DP),
                            lanes.ctypes.data_as(_DP))  # fmt: skip
        return TwinLanes(out, lanes[:, 1], lanes[:, 0].astype(np.int8), lanes[:, 2].astype(np.int64), lanes[:, 3:])

    def stage1(self, pars, N_exit, fields_init, derivatives_init, N_sub, max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None, stop_at_end=True, stage1=None):
        """the front end's first stage: (start states (B, K, 4), H at the exits (B, K), status (B,), N_exit - N_sub (K,))"""
        n_exit = np.ascontiguousarray(N_exit, dtype=np.float64)
        x = np.ascontiguousarray(fields_init, dtype=np.float64)
        v = np.ascontiguousarray(derivatives_init, dtype=np.float64)
        B, K = x.shape[0], n_exit.size
        p = np.ascontiguousarray(pars, dtype=np.float64)
        starts = n_exit - N_sub
        pts, inverse = np.unique(np.concatenate([starts, n_exit]), return_inverse=True)
        if stage1 is None:
            from background_sampled_reference import SampledTwin

            st1 = SampledTwin(self.artifact)
            states, status1 = np.empty((B, pts.size, 5)), np.empty(B, dtype=np.int8)
            for b in range(B):
                o, meta = st1.solve(p if p.ndim == 1 else p[b], [*x[b], *v[b]], pts, max_steps, solver, max_err, dt, stop_at_end)
                states[b], status1[b] = o[:, :5], meta["status"]
        else:
            states, status1 = np.asarray(stage1.states), np.asarray(stage1.status)
        return states[:, inverse[:K], :4], states[:, inverse[K:], 4], status1, starts

    def power_spectra(self, pars, N_exit, fields_init, derivatives_init, *, N_eval=None, N_sub=5.0, max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None,
                      stop_at_end=True, stage1=None) -> TwinSpectra:  # fmt: skip
        """``inflatox_amd.background.power_spectra``'s arguments (checked there, not here) and its two stages, in its own words.
        ``stage1``: the ``SampledSolution`` of its first stage (a GPU test hands in the device's, which the front end's own run
        repeats bit for bit); None: ``SampledTwin``'s, lane by lane."""
        start, h_exit, status1, starts = self.stage1(pars, N_exit, fields_init, derivatives_init, N_sub, max_steps, max_err, solver, dt, stop_at_end, stage1)
        n_exit = np.ascontiguousarray(N_exit, dtype=np.float64)
        p = np.ascontiguousarray(pars, dtype=np.float64)
        B, K = start.shape[:2]
        kappa = h_exit * math.exp(N_sub)
        status = np.repeat(status1[:, None], K, axis=1).reshape(-1)
        out, n_end, accepted = np.full((22, B * K), np.nan), np.full(B * K, np.nan), np.zeros(B * K, dtype=np.int64)
        run = np.flatnonzero((np.isfinite(start).all(axis=2) & np.isfinite(h_exit)).reshape(-1))
        lane_start = np.tile(starts, B)
        if run.size:
            target = np.full(run.size, np.nan) if N_eval is None else N_eval - lane_start[run]
            lane_p = p if p.ndim == 1 else np.ascontiguousarray(np.repeat(p, K, axis=0)[run])
            got = self.lanes(lane_p, start.reshape(-1, 4)[run], kappa.reshape(-1)[run], target, max_steps, max_err, solver, dt=dt, stop_at_end=stop_at_end)
            valid = got.status == (ENDED if N_eval is None else TARGET)
            out[:, run] = np.where(valid[None, :], got.out, np.nan)
            n_end[run] = np.where(got.status == ENDED, got.N_end, np.nan)
            status[run] = got.status
            accepted[run] = got.accepted
        out = out.reshape(22, B, K)
        offset = lane_start.reshape(B, K)
        q = out[3:11].reshape(2, 2, 2, B, K)
        modes = np.moveaxis(q[:, :, 0] + 1j * q[:, :, 1], (0, 1), (2, 3))
        return TwinSpectra(out[0], out[1], out[2], h_exit * np.exp(n_exit)[None, :], out[19] + offset, out[21], modes, n_end.reshape(B, K) + offset,
                           status.reshape(B, K), accepted.reshape(B, K))  # fmt: skip


@functools.lru_cache(maxsize=None)
def zoo_twin(name):
    import background_truth as bt

    return ModesTwin(bt.host_artifact(name))


def friedmann_h(artifact_or_twin, pars, init):
    """H0 = sqrt((V + kin / 2) / 3) of lanes (n, 4), from a twin run of no steps (the stepper's own expression)"""
    twin = artifact_or_twin if isinstance(artifact_or_twin, ModesTwin) else ModesTwin(artifact_or_twin)
    return twin.lanes(pars, init, 1.0, np.nan, max_steps=0).final[:, 4]


def spectra_of(modes_q, kappa, eps):
    """(P_R, P_S, C_RS) of Qt^I_J (..., 2, 2) complex"""
    scale = kappa**2 / (8 * math.pi**2 * eps)
    qs, qn = modes_q[..., 0], modes_q[..., 1]
    return scale * (np.abs(qs) ** 2).sum(-1), scale * (np.abs(qn) ** 2).sum(-1), scale * (qs * qn.conj()).real.sum(-1)


def relative_error(got, want):
    """worst of |dP_R| / P_R, |dP_S| / P_S and |dC_RS| / sqrt(P_R P_S); ``got``, ``want``: (P_R, P_S, C_RS), arrays of one shape"""
    (gr, gs, gc), (wr, ws, wc) = got, want
    return float(max(np.max(np.abs(gr - wr) / wr), np.max(np.abs(gs - ws) / ws), np.max(np.abs(gc - wc) / np.sqrt(wr * ws))))


def wronskian_error(final, kappa):
    """worst |W_IJ - 2 i kappa delta_IJ| / (2 kappa) of the accepted final states (n, >= 22), with
    W_IJ = e^(3N) sum_a [Qt^I_a conj(Pt^J_a) - Pt^I_a conj(Qt^J_a)]"""
    y = np.asarray(final)
    q = (y[:, 6:14:2] + 1j * y[:, 7:14:2]).reshape(-1, 2, 2)
    pp = (y[:, 14:22:2] + 1j * y[:, 15:22:2]).reshape(-1, 2, 2)
    w = np.exp(3.0 * y[:, 5])[:, None, None] * (np.einsum("nia,nja->nij", q, pp.conj()) - np.einsum("nia,nja->nij", pp, q.conj()))
    want = 2j * np.asarray(kappa)[:, None, None] * np.eye(2)[None]
    return float(np.max(np.abs(w - want) / (2.0 * np.asarray(kappa)[:, None, None])))


# ---- truth (a): the field-basis system on the Cartesian plane --------------------------------------------------------------------
PLANE_KAPPA = 5.0  # kappa = PLANE_KAPPA H0
PLANE_TARGET = 0.5


def plane_truth(state, a, b, kappa, t_eval):
    """The field-basis system from the Cartesian state (X, Y, Xd, Yd[, H]) with V = (a X^2 + b Y^2) / 2 and k / a = kappa e^-N:
    (P_R, P_S, C_RS, eps_H, N) at the time ``t_eval``.  e_s = (-T_y, T_x)."""
    from scipy.integrate import solve_ivp

    X, Y, Xd, Yd = (float(v) for v in state[:4])
    H0 = math.sqrt(((a * X * X + b * Y * Y) / 2 + (Xd * Xd + Yd * Yd) / 2) / 3)

    def f(_t, s):
        x, y, cx, cy, H, N = (v.real for v in s[:6])
        ax, ay = -a * x - 3.0 * H * cx, -b * y - 3.0 * H * cy
        Hd = -(cx * cx + cy * cy) / 2  # (on the Friedmann constraint; the code integrates V - 3 H^2)
        chi, acc = (cx, cy), (ax, ay)
        M = np.array([[(a if i == 0 else b) * (i == j) - (3.0 * chi[i] * chi[j] + (acc[i] * chi[j] + chi[i] * acc[j]) / H - chi[i] * chi[j] * Hd / (H * H)) for j in range(2)]
                      for i in range(2)])  # fmt: skip
        k2 = kappa * kappa * math.exp(-2.0 * N)
        q, pq = s[6:10].reshape(2, 2), s[10:14].reshape(2, 2)  # [I][a]
        dp = -3.0 * H * pq - k2 * q - q @ M.T
        return np.concatenate([[cx, cy, ax, ay, Hd, H], pq.reshape(-1), dp.reshape(-1)])

    eye = np.eye(2, dtype=complex)
    y0 = np.concatenate([np.array([X, Y, Xd, Yd, H0, 0.0], dtype=complex), eye.reshape(-1), ((-1j * kappa - H0) * eye).reshape(-1)])
    sol = solve_ivp(f, (0.0, float(t_eval)), y0, method="DOP853", rtol=1e-12, atol=1e-14)
    assert sol.success
    s = sol.y[:, -1]
    cx, cy, H, N = s[2].real, s[3].real, s[4].real, s[5].real
    kin = cx * cx + cy * cy
    sd = math.sqrt(kin)
    q = s[6:10].reshape(2, 2)
    qs = (q[:, 0] * cx + q[:, 1] * cy) / sd
    qn = (-q[:, 0] * cy + q[:, 1] * cx) / sd
    eps = kin / (2 * H * H)
    return (*spectra_of(np.stack([qs, qn], axis=-1), kappa, eps), eps, N)


@functools.lru_cache(maxsize=None)
def plane_case(n=17):
    import transfer_reference as tr

    return tr.plane_case(n)


def plane_lanes():
    """(Cartesian states (17, 5), kappa (17,)) of truth (a): kappa = PLANE_KAPPA H0"""
    cs = plane_case()[5]
    return cs, PLANE_KAPPA * cs[:, 4]


def plane_error(lanes, states, kappa, a, b):
    """the relative error of a solution at PLANE_TARGET against truth (a), read at the times the solution located the target at"""
    want = np.array([plane_truth(states[k], a, b, kappa[k], lanes.out[20, k]) for k in range(states.shape[0])]).T
    assert np.abs(want[4] - PLANE_TARGET).max() < 1e-6  # (the truth's own N at the solution's t: the same point)
    return relative_error(lanes.out[:3], want[:3])


# ---- truth (b): the four equations on curved field spaces -------------------------------------------------------------------------
def truth_rhs(model, slots):
    """g(x0, x1, xd0, xd1, H, p) -> (eom^0, eom^1, V, kin, eps_H, omega, eta_par, V_TT, V_TN, V_NN, R) in float64: the Euler-Lagrange
    derivation and the truth expressions of the kinematics and the masses (T, N in their orientation), parameters in the slots of
    ``CompilationArtifact.symbol_dictionary``"""
    import sympy as sp
    from sympy.printing.c import C99CodePrinter

    import background_truth as bt
    import kinematics_reference as kr
    import masses_reference as mr

    eom, V, kin = bt._derivation(model)
    tr = mr.truth_expressions(model.coordinates, model.metric, model.potential, model.coordinate_tangents)
    kt = kr.truth_expressions(model.coordinates, model.metric, model.potential, model.coordinate_tangents)
    exprs = [sp.sympify(e) for e in (*eom, V, kin, tr[4], tr[5], kt[1], tr[0], tr[1], tr[2], tr[3])]
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
    import workloads

    return truth_rhs(workloads.model_for(name), workloads.artifact_for(name)[1].symbol_dictionary)


def _mode_rates(vals, H, k2, q, pq):
    """(dQ/dt, dP/dt) of the four equations, q and pq complex [I][J], from ``truth_rhs``'s values: e_s = -N, so
    M_sigma_s = -(V_TN + V_N sigma_dot / H) = -(V_TN + omega kin), and 2 vchi / H = 2 (eta_par - 3) kin"""
    _e0, _e1, _V, kin, eps, om, eta, vtt, vtn, vnn, ric = vals
    Om = om * H
    m_ss_, m_sn, m_nn = vtt + (3.0 - eps) * kin + 2.0 * (eta - 3.0) * kin, -(vtn + om * kin), vnn + 0.5 * kin * ric
    dq = np.stack([pq[:, 0] + Om * q[:, 1], pq[:, 1] - Om * q[:, 0]], axis=1)
    dp = np.stack([Om * pq[:, 1] - 3.0 * H * pq[:, 0] - (k2 + m_ss_) * q[:, 0] - m_sn * q[:, 1],
                   -Om * pq[:, 0] - 3.0 * H * pq[:, 1] - m_sn * q[:, 0] - (k2 + m_nn) * q[:, 1]], axis=1)  # fmt: skip
    return dq, dp


def _start(g, init, p, kappa):
    V, kin = g(*init, 1.0, p)[2:4]
    H0 = math.sqrt((V + 0.5 * kin) / 3.0)
    eye = np.eye(2, dtype=complex)
    return H0, eye.reshape(-1), ((-1j * kappa - H0) * eye).reshape(-1)


def truth_lane(g, init, p, kappa, n_target):
    """(P_R, P_S, C_RS, eps_H, t) at the local e-fold count ``n_target`` of the lane from ``init`` (4,) with parameter row ``p``, the
    model functions ``g`` (``truth_rhs``) and kappa: y = (phi, chi, H, t, Qt, Pt) integrated in N (H > 0 along the trajectory)."""
    from scipy.integrate import solve_ivp

    H0, q0, p0 = _start(g, init, p, kappa)

    def f(N, s):
        x0, x1, v0, v1, H = (v.real for v in s[:5])
        vals = g(x0, x1, v0, v1, H, p)
        dq, dp = _mode_rates(vals, H, kappa * kappa * math.exp(-2.0 * N), s[6:10].reshape(2, 2), s[10:14].reshape(2, 2))
        return np.concatenate([[v0, v1, -vals[0] - 3.0 * H * v0, -vals[1] - 3.0 * H * v1, vals[2] - 3.0 * H * H, 1.0], dq.reshape(-1), dp.reshape(-1)]) / H

    y0 = np.concatenate([np.array([*map(float, init), H0, 0.0], dtype=complex), q0, p0])
    sol = solve_ivp(f, (0.0, float(n_target)), y0, method="DOP853", rtol=1e-12, atol=1e-14)
    assert sol.success
    s = sol.y[:, -1]
    eps = g(s[0].real, s[1].real, s[2].real, s[3].real, s[4].real, p)[4]
    return (*spectra_of(s[6:10].reshape(2, 2), kappa, eps), eps, s[5].real)


def truth_final(g, init, p, kappa, t_end):
    """(16,) the mode components y[6..21] at the time ``t_end``: the four equations integrated in t, DOP853 at rtol 1e-13"""
    from scipy.integrate import solve_ivp

    H0, q0, p0 = _start(g, init, p, kappa)

    def f(_t, s):
        x0, x1, v0, v1, H, N = (v.real for v in s[:6])
        vals = g(x0, x1, v0, v1, H, p)
        dq, dp = _mode_rates(vals, H, kappa * kappa * math.exp(-2.0 * N), s[6:10].reshape(2, 2), s[10:14].reshape(2, 2))
        return np.concatenate([[v0, v1, -vals[0] - 3.0 * H * v0, -vals[1] - 3.0 * H * v1, vals[2] - 3.0 * H * H, H], dq.reshape(-1), dp.reshape(-1)])

    y0 = np.concatenate([np.array([*map(float, init), H0, 0.0], dtype=complex), q0, p0])
    sol = solve_ivp(f, (0.0, float(t_end)), y0, method="DOP853", rtol=1e-13, atol=1e-15)
    assert sol.success
    z = sol.y[6:, -1]
    return np.stack([z.real, z.imag], axis=1).reshape(-1)


def zoo_lanes(name, n_lanes=LANES):
    """(init (n, 4), pars (n, n_par), kappa (n,), n_target): the first lanes of ``background_truth.batch(name)``, each with the
    wavenumber kappa = H0 e^N_SUB, evaluated at the last of ``background_truth.samples_for(name, "N")``"""
    import background_truth as bt

    init, pars = (v[:n_lanes] for v in bt.batch(name))
    kappa = friedmann_h(zoo_twin(name), pars, init) * math.exp(N_SUB)
    return init, pars, kappa, float(bt.samples_for(name, "N")[-1])


@functools.lru_cache(maxsize=None)
def zoo_truth(name):
    """(5, LANES): ``truth_lane`` of ``zoo_lanes(name)``: computed once and shared"""
    init, pars, kappa, target = zoo_lanes(name)
    truth = np.array([truth_lane(_zoo_rhs(name), init[k], pars[k], kappa[k], target) for k in range(LANES)]).T
    truth.setflags(write=False)
    return truth


# ---- truth (c): power-law inflation ----------------------------------------------------------------------------------------------
POWER_N_EXIT = np.array([3.0, 4.0])
POWER_N_EVAL = 10.0


def power_law_formula(h_k):
    """the exact super-horizon curvature spectrum of power-law inflation with a ~ t^p, p = ``background_reference.P_POW``, for the
    mode that leaves the horizon (k = a H) at H = ``h_k``; the spectator's is the same"""
    import background_reference as br

    eps = 1.0 / br.P_POW
    nu = 1.5 + eps / (1.0 - eps)
    amp = (2.0 ** (nu - 1.5) * math.gamma(nu) / math.gamma(1.5)) ** 2 * (1.0 - eps) ** (2.0 * nu - 1.0)
    return amp * np.asarray(h_k) ** 2 / (8.0 * math.pi**2 * eps)


@functools.lru_cache(maxsize=None)
def power_law_case():
    """(artefact, parameter row, initial state (4,), H at the exits (2,)): on the attractor from t = 1, N = p ln t and H = p / t"""
    import background_reference as br

    art, p = br.power_law_artifact()
    return art, p, br.power_law_init(), br.P_POW * np.exp(-POWER_N_EXIT / br.P_POW)


@functools.lru_cache(maxsize=None)
def power_law_truth(n_sub=N_SUB):
    """(2, 2): P_R and P_S of the two modes at POWER_N_EVAL by DOP853 from the very initial conditions of the project -- the vacuum
    put in at a finite ``n_sub`` -- on the exact background"""
    import background_reference as br
    art, p, init, h_k = power_law_case()
    g = truth_rhs(br.power_law_model(), art.symbol_dictionary)
    out = np.empty((2, 2))
    for j, n_exit in enumerate(POWER_N_EXIT):
        n0 = n_exit - n_sub
        y = br.power_law_exact(math.exp(n0 / br.P_POW) - 1.0)
        got = truth_lane(g, y[:4], p, h_k[j] * math.exp(n_sub), POWER_N_EVAL - n0)
        out[:, j] = got[0], got[1]
    return out


def power_law_start_error(n_sub=N_SUB):
    """what the start at a finite N_sub leaves: the worst relative difference of ``power_law_truth`` from the formula, P_R and P_S"""
    want = power_law_formula(power_law_case()[3])
    return float(np.max(np.abs(power_law_truth(n_sub) - want[None, :]) / want[None, :]))


# ---- the long run on the hyperbolic model ----------------------------------------------------------------------------------------
HYPER_B, HYPER_K = 5, 52
HYPER_N_EXIT = np.linspace(3.0, 3.51, HYPER_K)
HYPER_MAX_ERR = 1e-10
HYPER_N_EVAL = 6.0


def hyper_states(B=HYPER_B, seed=3):
    """(fields (B, 2), velocities (B, 2)) high on the potential of the hyperbolic example model at its parameters (1, 1, 1), turning"""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(6.5, 7.0, B), rng.uniform(-1, 1, B)], axis=1)
    v = np.stack([rng.uniform(-0.3, -0.1, B), rng.uniform(-4e-4, 4e-4, B)], axis=1)
    return x, v


def hyper_error(solver):
    """the relative error of the twin's second stage against truth (b) on the lanes j = 0 and HYPER_K - 1 of every trajectory of
    ``hyper_states``, evaluated at N = HYPER_N_EVAL: (error, fewest accepted steps)"""
    import workloads

    spec, art = workloads.artifact_for("hyperbolic")
    twin, g = ModesTwin(art), workload_rhs("hyperbolic")
    x, v = hyper_states()
    cols = [0, HYPER_K - 1]
    n_exit = HYPER_N_EXIT[cols]
    start, h_exit, _status, starts = twin.stage1(spec.args, n_exit, x, v, N_SUB, max_err=HYPER_MAX_ERR, solver=solver)
    got = twin.power_spectra(spec.args, n_exit, x, v, N_eval=HYPER_N_EVAL, N_sub=N_SUB, max_err=HYPER_MAX_ERR, solver=solver)
    assert np.all(got.status == TARGET)
    want = np.array([[truth_lane(g, start[b, j], spec.args, h_exit[b, j] * math.exp(N_SUB), HYPER_N_EVAL - starts[j])[:3] for j in range(2)] for b in range(HYPER_B)])
    return relative_error((got.P_R, got.P_S, got.C_RS), tuple(np.moveaxis(want, 2, 0))), int(got.accepted.min())


def hyper_bound(solver):
    """``bound`` for the long run on the hyperbolic model"""
    return 1e-10 + 2.0 * recorded()["hyperbolic"][f"{solver}/{HYPER_MAX_ERR:g}"]


# ---- the recorded step-control error and the bound -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stepper_code_hash():
    """the hash of the code (comments aside) of the two headers that make the stepper: the state of the code a profile belongs to"""
    from inflatox_amd.compiler import _code_only

    h = hashlib.sha256()
    for f in ("inflx_background.h", "inflx_modes.h"):
        with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
            h.update(_code_only(fh.read()).encode())
    return h.hexdigest()[:16]


def recorded():
    with open(PROFILE) as fh:
        return json.load(fh)


def bound(name, solver, max_err):
    """what the relative error against truth (b) may be: 1e-10 plus twice the host twin's recorded worst error for this model, solver
    and max_err -- a margin for other libm and contraction choices, not for defects"""
    return 1e-10 + 2.0 * recorded()["zoo"][f"{name}/{solver}/{max_err:g}"]


def plane_bound(solver, max_err):
    return 1e-10 + 2.0 * recorded()["plane"][f"{solver}/{max_err:g}"]


def power_law_bound():
    """truth (c): twice the measured error that the start at N_SUB leaves against the formula"""
    return 2.0 * recorded()["power_law"]["start_error"]


def zoo_error(lanes, truth):
    return relative_error(lanes.out[:3], truth[:3])


def measure():
    import background_truth as bt

    zoo, wron = {}, {}
    for name in bt.GPU_MODELS:
        init, pars, kappa, target = zoo_lanes(name)
        truth = zoo_truth(name)
        assert np.isfinite(truth).all()
        for solver in ("rk4", "rkf"):
            for max_err in MAX_ERRS:
                got = zoo_twin(name).lanes(pars, init, kappa, target, max_err=max_err, solver=solver, stop_at_end=False)
                assert np.all(got.status == TARGET), (name, solver, max_err, got.status)
                key = f"{name}/{solver}/{max_err:g}"
                zoo[key], wron[key] = zoo_error(got, truth), wronskian_error(got.final, kappa)
                print(f"{name} {solver} max_err {max_err:g}: worst relative |twin - truth (b)| {zoo[key]:.3e}, Wronskian {wron[key]:.3e}, "
                      f"{got.accepted.min()} .. {got.accepted.max()} steps", flush=True)  # fmt: skip
    _pa, ca, _pp, cp, _ps, _cs, a, b = plane_case()
    cs, kappa = plane_lanes()
    plane = {}
    for solver in ("rk4", "rkf"):
        for max_err in MAX_ERRS:
            got = ModesTwin(ca).lanes(cp, cs[:, :4], kappa, PLANE_TARGET, max_err=max_err, solver=solver, stop_at_end=False)
            assert np.all(got.status == TARGET)
            plane[f"{solver}/{max_err:g}"] = plane_error(got, cs, kappa, a, b)
            print(f"plane {solver} max_err {max_err:g}: worst relative |twin - truth (a)| {plane[f'{solver}/{max_err:g}']:.3e}", flush=True)
    hyper = {}
    for solver in ("rk4", "rkf"):
        hyper[f"{solver}/{HYPER_MAX_ERR:g}"], fewest = hyper_error(solver)
        print(f"hyperbolic {solver}: worst relative |twin - truth (b)| {hyper[f'{solver}/{HYPER_MAX_ERR:g}']:.3e}, at least {fewest} steps", flush=True)
    start = power_law_start_error()
    print(f"power law: the start at N_sub = {N_SUB:g} leaves {start:.3e} against the formula (e^(-2 N_sub) = {math.exp(-2 * N_SUB):.3e})", flush=True)
    return {
        "stepper_code": stepper_code_hash(),
        "what": "worst relative |host twin - truth (b)| over P_R, P_S (own size) and C_RS (sqrt(P_R P_S)), 65 lanes of background_truth.batch, kappa = H0 e^3, "
                "evaluated at the last e-fold sample of background_truth.samples_for, stop_at_end off; truth: DOP853 in N at rtol 1e-12 (tests/modes_reference.py)",
        "bound": "tests assert 1e-10 + 2 x the value recorded here",
        "zoo": zoo,
        "wronskian": wron,
        "wronskian_what": "worst |W_IJ - 2 i kappa delta_IJ| / (2 kappa) of the same runs' accepted final states: recorded for information, asserted against the zoo bound",
        "plane": plane,
        "plane_what": "the same against truth (a): 17 states of kinematics_reference.plane_states on the Cartesian plane, kappa = 5 H0, evaluated at N = 0.5, "
                      "stop_at_end off; truth: the field-basis system, DOP853 at rtol 1e-12",
        "hyperbolic": hyper,
        "hyperbolic_what": "the same for the second stage of the front end on the hyperbolic example model at max_err = 1e-10: modes_reference.hyper_states, the first and "
                           "the last of the 52 wavenumbers, N_sub = 3, evaluated at N = 6; every lane takes more than 256 accepted steps",
        "power_law": {"start_error": start, "N_sub": N_SUB},
        "power_law_what": "worst relative difference, P_R and P_S of the modes with N_exit = 3 and 4 at N = 10, between DOP853 from the project's initial conditions "
                          "at N_sub = 3 on the exact power-law background and the exact super-horizon formula; tests assert twice this",
    }  # fmt: skip


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    result = measure()
    with open(PROFILE, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
