"""Horizon crossings on the host -- TEST INFRASTRUCTURE.

``CrossingTwin`` compiles tests/crossing_twin.cpp the way ``background_sampled_reference.SampledTwin`` compiles its twin: the artefact's
generated headers and csrc/inflx_crossing.h (over csrc/inflx_background.h and csrc/inflx_deltan.h) for the CPU, contraction off.
``restated_crossings`` states the rule again, independently of that header: the accepted steps come from the plain stepper's host build
(``background_reference.BackgroundTwin``, every step a row), the interpolant is ``background_target_reference.hermite`` (a cubic in
the power basis, not the header's basis functions) and the root of N + ln H - tau inside a step is scipy's brentq.
"""

from __future__ import annotations

import ctypes as C
import hashlib
import math
import os
import subprocess
import tempfile

import numpy as np

from background_reference import COMPLETE, ENDED
from background_target_reference import TARGET, hermite, rhs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "inflatox_amd", "csrc")
_DP = C.POINTER(C.c_double)

# constants of the pivot matching, restated here from their sources: CODATA k_B = 8.617333262e-5 eV / K, 1 Mpc = 3.0856775814913673e22 m,
# hbar c = 1.973269804e-16 GeV m, the FIRAS temperature and the standard-model entropy count today
K_B_GEV_PER_K = 8.617333262e-5 * 1e-9
MPC_M = 3.0856775814913673e22
HBAR_C_GEV_M = 1.973269804e-16
T0_K = 2.7255
GS0 = 2.0 + (7.0 / 8.0) * 2.0 * 3.0 * (4.0 / 11.0)


def reheating_offset_restated(k_mpc=0.05, w_reh=1.0 / 3.0, N_reh=0.0, g_reh=106.75, gs_reh=106.75):
    """A of the issue's pivot matching, term by term from the derivation: ln k_phys = L - ln a_0, ln a_0 = N_end + N_reh +
    ln(gs_reh / gs_0) / 3 + ln(T_reh / T_0), rho_reh = 3 H_end^2 exp(-3 (1 + w) N_reh) = pi^2 g T_reh^4 / 30."""
    k_gev = k_mpc * HBAR_C_GEV_M / MPC_M
    t0_gev = T0_K * K_B_GEV_PER_K
    ln_t_reh_minus_half_ln_h = 0.25 * math.log(30.0 * 3.0 / (math.pi**2 * g_reh)) - 0.75 * (1.0 + w_reh) * N_reh
    return math.log(k_gev) + N_reh + math.log(gs_reh / GS0) / 3.0 + ln_t_reh_minus_half_ln_h - math.log(t0_gev)


class CrossingTwin:
    """tests/crossing_twin.cpp built for the CPU from an artefact's generated headers."""

    SOURCES = [os.path.join(CSRC, f) for f in ("inflx_background.h", "inflx_deltan.h", "inflx_crossing.h")] + [os.path.join(HERE, "crossing_twin.cpp")]

    def __init__(self, artifact, cxx: str = "g++", contract: str = "off"):
        header_text = artifact._build[0]
        eom_text = artifact.eom_header_text()
        tag = hashlib.sha1((header_text + eom_text + "".join(open(f).read() for f in self.SOURCES) + contract).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_crossing_twin")
        os.makedirs(d, exist_ok=True)
        hdr, eom_hdr, so = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".so"))
        self.headers = (hdr, eom_hdr)
        if not os.path.exists(so):
            for path, text in ((hdr, header_text), (eom_hdr, eom_text)):
                with open(path, "w") as fh:
                    fh.write(text)
            tmp = so + f".{os.getpid()}.tmp"
            subprocess.run([cxx, "-O2", "-fPIC", "-shared", *self.compile_options(hdr, eom_hdr, contract), self.SOURCES[-1], "-o", tmp], check=True)
            os.replace(tmp, so)
        self.lib = C.CDLL(so)
        self.lib.twin_solve_crossings.argtypes = [_DP, _DP, C.c_double, _DP, C.c_uint, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, _DP, _DP, _DP]
        self.lib.twin_solve_crossings.restype = None
        self.lib.twin_inflation_end.argtypes = [_DP, _DP, C.c_size_t, C.c_int, C.c_double, C.c_double, _DP, _DP]
        self.lib.twin_inflation_end.restype = None
        self.lib.twin_locate.argtypes = [_DP, C.c_double, C.c_double]
        self.lib.twin_locate.restype = C.c_double

    @staticmethod
    def compile_options(hdr, eom_hdr, contract="off"):
        return ["-std=c++17", f"-ffp-contract={contract}", *(["-mfma"] if contract != "off" else []), "-fno-fast-math", "-Wno-unknown-pragmas", f"-I{CSRC}",
                f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"']  # fmt: skip

    def solve(self, p, init, samples, max_steps, offset=0.0, method="rkf", max_err=1e-8, dt=None, stop_at_end=True):
        """(out (S, 8): y[0..5], t, epsilon_H at every crossing, NaN where not emitted; dict with status, N_end, accepted, n_stored,
        n_before and step_of (S): the accepted step that emitted each crossing, 0 = init)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        init = np.ascontiguousarray(init, dtype=np.float64)
        samples = np.ascontiguousarray(samples, dtype=np.float64)
        out = np.empty((samples.size, 8))
        step_of = np.empty(samples.size)
        meta = np.empty(5)
        self.lib.twin_solve_crossings(p.ctypes.data_as(_DP), init.ctypes.data_as(_DP), float(offset), samples.ctypes.data_as(_DP), samples.size, int(max_steps),
                                      1 if method == "rkf" else 0, max_err, dt or 0.0, int(stop_at_end), out.ctypes.data_as(_DP), step_of.ctypes.data_as(_DP),
                                      meta.ctypes.data_as(_DP))  # fmt: skip
        return out, dict(status=int(meta[0]), N_end=meta[1], accepted=int(meta[2]), n_stored=int(meta[3]), n_before=int(meta[4]), step_of=step_of)

    def end(self, p, init, max_steps, method="rkf", max_err=1e-8, dt=None):
        """(out (8): y[0..5], t, epsilon_H at the located end of inflation, NaN unless ENDED; dict with status, accepted)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        init = np.ascontiguousarray(init, dtype=np.float64)
        out = np.empty(8)
        meta = np.empty(2)
        self.lib.twin_inflation_end(p.ctypes.data_as(_DP), init.ctypes.data_as(_DP), int(max_steps), 1 if method == "rkf" else 0, max_err, dt or 0.0,
                                    out.ctypes.data_as(_DP), meta.ctypes.data_as(_DP))  # fmt: skip
        return out, dict(status=int(meta[0]), accepted=int(meta[1]))

    def locate(self, ends, h, tau):
        ends = np.ascontiguousarray(ends, dtype=np.float64)
        return self.lib.twin_locate(ends.ctypes.data_as(_DP), float(h), float(tau))


def restated_crossings(stepper, p, init, samples, max_steps, offset=0.0, method="rkf", max_err=1e-8, dt=None, stop_at_end=True):
    """The rule of the issue in numpy, on the accepted steps of ``stepper`` (a ``BackgroundTwin``): (out (S, 8), dict with status, N_end,
    n_stored, n_before, step_of)."""
    from scipy.optimize import brentq

    samples = np.asarray(samples, dtype=np.float64)
    S = samples.size
    rows, meta = stepper.solve(p, init, max_steps + 1, method=method, max_err=max_err, dt=dt, stop_at_end=stop_at_end)
    last = meta["last_row"]
    y = rows[: last + 1, :6]
    t = rows[: last + 1, 6]
    eom = stepper.eom(p, y[:, :4])
    f = np.array([rhs(eom[k], y[k]) for k in range(last + 1)])
    out = np.full((S, 8), np.nan)
    step_of = np.full(S, np.nan)
    tau = offset + samples
    L = y[:, 5] + np.log(y[:, 4])

    def emit(j, state, time, step):
        kin = stepper.eom(p, state[None, :4])[0, 3]
        out[j, :6], out[j, 6], out[j, 7] = state, time, 0.5 * kin / state[4] ** 2
        step_of[j] = step

    n_before = int(np.sum(tau < L[0]))
    cursor = n_before
    if cursor < S and tau[cursor] == L[0]:
        emit(cursor, y[0], t[0], 0)
        cursor += 1
    status = None
    if last == 0 and meta["status"] == ENDED:  # past the end at the start
        status = ENDED
    elif cursor == S:
        status = TARGET
    k = 1
    while status is None and k <= last:
        h = t[k] - t[k - 1]
        ended_here = meta["status"] == ENDED and k == last
        while cursor < S and tau[cursor] <= L[k]:

            def g(th, target=tau[cursor]):
                return hermite(y[k - 1, 5], f[k - 1, 5], y[k, 5], f[k, 5], h, th) + math.log(hermite(y[k - 1, 4], f[k - 1, 4], y[k, 4], f[k, 4], h, th)) - target

            th = 1.0 if g(1.0) == 0.0 else brentq(g, 0.0, 1.0, xtol=1e-16, rtol=4 * np.finfo(float).eps, maxiter=200)
            state = hermite(y[k - 1], f[k - 1], y[k], f[k], h, th)
            if ended_here and meta["N_end"] < state[5]:
                break
            emit(cursor, state, t[k - 1] + th * h, k)
            cursor += 1
        if cursor == S:
            status = TARGET
        k += 1
    if status is None:
        status = meta["status"] if meta["status"] != COMPLETE or last < max_steps else COMPLETE
    return out, dict(status=status, N_end=meta["N_end"] if status == ENDED else math.nan, n_stored=cursor - n_before, n_before=n_before, step_of=step_of)
