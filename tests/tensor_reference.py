"""Truths and host twin of the tensor modes and the tensor power spectrum (csrc/inflx_tensor.h) -- TEST INFRASTRUCTURE.

Two truths:

* ``truth_lane`` (b'), curved zoo: the two complex equations of csrc/inflx_tensor.h,

      d ht/dt = pt,   d pt/dt = -3 H pt - kappa^2 e^-2N ht,   ht = 1 and pt = -i kappa - H0 at the start,

  on the independent Euler-Lagrange background of tests/background_truth.py, integrated in N by scipy's DOP853 at rtol = 1e-12 so
  that the target is met exactly.  It uses none of the project's stepper.
* ``power_law_formula`` (c'), exact: power-law inflation a ~ t^p, p = 8, eps = 1 / p, nu = 3/2 + eps / (1 - eps):
  P_T = [2^(nu - 3/2) Gamma(nu) / Gamma(3/2)]^2 (1 - eps)^(2 nu - 1) 2 H_k^2 / pi^2 on super-horizon scales, hence r = 16 eps = 2
  against ``modes_reference.power_law_formula``, n_s - 1 = n_t = -2 eps / (1 - eps) = -2/7 and no running.

``TensorTwin`` compiles tests/tensor_twin.cpp -- the generated headers and csrc/inflx_tensor.h for the CPU, contraction off.
``TensorTwin.tensor_spectra`` is ``inflatox_amd.background.tensor_spectra`` on the host: its stage 1 from ``SampledTwin`` (or from a
``SampledSolution`` handed in), its stage 2 from the twin.

Errors are relative to P_T's own size, |dP_T| / P_T of the truth.

``python tests/tensor_reference.py`` measures the twin's own step-control error against truth (b') -- per model and solver at
max_err = 1e-8 and 1e-10 -- and the error that a start at a finite N_sub leaves against (c'), and writes them to
profiles/background_tensor.json; ``bound`` is what the tests assert: 1e-10 plus twice that.
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
PROFILE = os.path.join(ROOT, "profiles", "background_tensor.json")
_DP = C.POINTER(C.c_double)

LANES = 65
MAX_ERRS = (1e-8, 1e-10)
N_SUB = 3.0  # the lane-level truths start their modes at kappa = H0 e^N_SUB
COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW, TARGET = 0, 1, 2, 3, 4, 5


class TwinLanes(NamedTuple):
    """What ``TensorTwin.lanes`` returns: ``out`` (8, n) as ``InflatoxDevLib.mode_spectra``'s with ``MODES_TENSOR``, ``N_end`` (n,) as
    the kernel leaves it, ``status`` (n,), ``accepted`` (n,) steps and ``final`` (n, 11): y[0..9] and t where each lane stopped (never
    a located state)."""

    out: np.ndarray
    N_end: np.ndarray
    status: np.ndarray
    accepted: np.ndarray
    final: np.ndarray


class TwinSpectra(NamedTuple):
    """``inflatox_amd.background.TensorSpectra``'s members, plus ``accepted`` (B, K)"""

    P_T: np.ndarray
    k: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    modes: np.ndarray
    N_end: np.ndarray
    status: np.ndarray
    accepted: np.ndarray


# ---- the host build --------------------------------------------------------------------------------------------------------------
class TensorTwin:
    """tests/tensor_twin.cpp built for the CPU from an artefact's generated headers, contraction off like ``ModesTwin``"""

    def __init__(self, artifact, cxx: str = "g++", contract: str = "off"):
        self.artifact = artifact
        texts = (artifact._build[0], artifact.eom_header_text())
        sources = [os.path.join(CSRC, "inflx_background.h"), os.path.join(CSRC, "inflx_tensor.h"), os.path.join(HERE, "tensor_twin.cpp")]
        tag = hashlib.sha1(("".join(texts) + "".join(open(f).read() for f in sources) + contract).encode()).hexdigest()[:16]
        d = os.path.join(tempfile.gettempdir(), "inflx_tensor_twin")
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
        self.lib.twin_tensor.argtypes = [_DP, C.c_size_t, _DP, _DP, _DP, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, _DP, _DP]
        self.lib.twin_tensor.restype = None

    @staticmethod
    def compile_options(hdr, eom_hdr, contract="off"):
        """what any build of tests/tensor_twin.cpp takes besides its output (the stand-alone program adds -DTENSOR_TWIN_MAIN)"""
        return ["-std=c++17", f"-ffp-contract={contract}", *(["-mfma"] if contract != "off" else []), "-fno-fast-math", "-Wno-unknown-pragmas", f"-I{CSRC}",
                f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"']  # fmt: skip

    def lanes(self, pars, init, kappa, n_target, max_steps=1_000_000, max_err=1e-8, solver="rkf", *, dt=None, stop_at_end=True) -> TwinLanes:
        """``InflatoxDevLib.mode_spectra``'s arguments: init (n, 4), kappa (n,), n_target (n,) (NaN: none)"""
        init = np.ascontiguousarray(init, dtype=np.float64)
        n = init.shape[0]
        p = np.ascontiguousarray(pars, dtype=np.float64)
        kappa = np.ascontiguousarray(np.broadcast_to(np.asarray(kappa, dtype=np.float64), (n,)))
        target = np.ascontiguousarray(np.broadcast_to(np.asarray(n_target, dtype=np.float64), (n,)))
        out = np.empty((8, n))
        lanes = np.empty((n, 14))
        self.lib.twin_tensor(p.ctypes.data_as(_DP), 0 if p.ndim == 1 else p.shape[1], init.ctypes.data_as(_DP), kappa.ctypes.data_as(_DP), target.ctypes.data_as(_DP), n,
                             int(max_steps), 1 if solver == "rkf" else 0, float(max_err), float(dt or 0.0), int(stop_at_end), out.ctypes.data_as(_DP),
                             lanes.ctypes.data_as(_DP))  # fmt: skip
        return TwinLanes(out, lanes[:, 1], lanes[:, 0].astype(np.int8), lanes[:, 2].astype(np.int64), lanes[:, 3:])

    def stage1(self, pars, N_exit, fields_init, derivatives_init, N_sub, max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None, stop_at_end=True, stage1=None):
        """the front end's first stage, ``ModesTwin.stage1``'s own code: (start states (B, K, 4), H at the exits (B, K), status (B,),
        N_exit - N_sub (K,))"""
        import modes_reference as mo

        return mo.ModesTwin.stage1(self, pars, N_exit, fields_init, derivatives_init, N_sub, max_steps, max_err, solver, dt, stop_at_end, stage1)

    def tensor_spectra(self, pars, N_exit, fields_init, derivatives_init, *, N_eval=None, N_sub=5.0, max_steps=1_000_000, max_err=1e-8, solver="rkf", dt=None,
                       stop_at_end=True, stage1=None) -> TwinSpectra:  # fmt: skip
        """``inflatox_amd.background.tensor_spectra``'s arguments (checked there, not here) and its two stages, in its own words.
        ``stage1``: the ``SampledSolution`` of its first stage (a GPU test hands in the device's); None: ``SampledTwin``'s."""
        start, h_exit, status1, starts = self.stage1(pars, N_exit, fields_init, derivatives_init, N_sub, max_steps, max_err, solver, dt, stop_at_end, stage1)
        n_exit = np.ascontiguousarray(N_exit, dtype=np.float64)
        p = np.ascontiguousarray(pars, dtype=np.float64)
        B, K = start.shape[:2]
        kappa = h_exit * math.exp(N_sub)
        status = np.repeat(status1[:, None], K, axis=1).reshape(-1)
        out, n_end, accepted = np.full((8, B * K), np.nan), np.full(B * K, np.nan), np.zeros(B * K, dtype=np.int64)
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
        out = out.reshape(8, B, K)
        offset = lane_start.reshape(B, K)
        return TwinSpectra(out[0], h_exit * np.exp(n_exit)[None, :], out[5] + offset, out[7], out[1] + 1j * out[2], n_end.reshape(B, K) + offset,
                           status.reshape(B, K), accepted.reshape(B, K))  # fmt: skip


@functools.lru_cache(maxsize=None)
def zoo_twin(name):
    import background_truth as bt

    return TensorTwin(bt.host_artifact(name))


def friedmann_h(twin, pars, init):
    """H0 = sqrt((V + kin / 2) / 3) of lanes (n, 4), from a twin run of no steps (the stepper's own expression)"""
    return twin.lanes(pars, init, 1.0, np.nan, max_steps=0).final[:, 4]


def p_t_of(ht, kappa):
    """P_T = 2 kappa^2 |ht|^2 / pi^2"""
    return 2.0 * np.asarray(kappa) ** 2 * np.abs(ht) ** 2 / math.pi**2


def relative_error(got, want):
    """worst |dP_T| / P_T, arrays of one shape"""
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.asarray(want)))


def wronskian_error(final, kappa):
    """worst |W - 2 i kappa| / (2 kappa) of the accepted final states (n, >= 10), W = e^(3N) (ht conj(pt) - pt conj(ht))"""
    y = np.asarray(final)
    ht, pt = y[:, 6] + 1j * y[:, 7], y[:, 8] + 1j * y[:, 9]
    w = np.exp(3.0 * y[:, 5]) * (ht * pt.conj() - pt * ht.conj())
    return float(np.max(np.abs(w - 2j * np.asarray(kappa)) / (2.0 * np.asarray(kappa))))


# ---- truth (b'): the two complex equations on the Euler-Lagrange background ---------------------------------------------------------
def _start(g, init, p):
    _e0, _e1, V, kin = g(*init, p)
    return math.sqrt((V + 0.5 * kin) / 3.0)


def truth_lane(g, init, p, kappa, n_target):
    """(P_T, eps_H, t) at the local e-fold count ``n_target`` of the lane from ``init`` (4,) with parameter row ``p``, the model
    functions ``g`` (``background_truth.truth_functions``: eom^0, eom^1, V, kin) and kappa: y = (phi, chi, H, t, ht, pt) integrated in
    N (H > 0 along the trajectory)."""
    from scipy.integrate import solve_ivp

    H0 = _start(g, init, p)

    def f(N, s):
        x0, x1, v0, v1, H = (v.real for v in s[:5])
        e0, e1, V, _kin = g(x0, x1, v0, v1, p)
        k2 = kappa * kappa * math.exp(-2.0 * N)
        return np.array([v0, v1, -e0 - 3.0 * H * v0, -e1 - 3.0 * H * v1, V - 3.0 * H * H, 1.0, s[7], -3.0 * H * s[7] - k2 * s[6]]) / H

    y0 = np.array([*map(float, init), H0, 0.0, 1.0, -1j * kappa - H0], dtype=complex)
    sol = solve_ivp(f, (0.0, float(n_target)), y0, method="DOP853", rtol=1e-12, atol=1e-14)
    assert sol.success
    s = sol.y[:, -1]
    kin = g(s[0].real, s[1].real, s[2].real, s[3].real, p)[3]
    return float(p_t_of(s[6], kappa)), 0.5 * kin / s[4].real ** 2, s[5].real


def truth_final(g, init, p, kappa, t_end):
    """(4,) the mode components y[6..9] at the time ``t_end``: the two equations integrated in t, DOP853 at rtol 1e-13"""
    from scipy.integrate import solve_ivp

    H0 = _start(g, init, p)

    def f(_t, s):
        x0, x1, v0, v1, H, N = (v.real for v in s[:6])
        e0, e1, V, _kin = g(x0, x1, v0, v1, p)
        k2 = kappa * kappa * math.exp(-2.0 * N)
        return np.array([v0, v1, -e0 - 3.0 * H * v0, -e1 - 3.0 * H * v1, V - 3.0 * H * H, H, s[7], -3.0 * H * s[7] - k2 * s[6]])

    y0 = np.array([*map(float, init), H0, 0.0, 1.0, -1j * kappa - H0], dtype=complex)
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
    """(3, LANES): ``truth_lane`` of ``zoo_lanes(name)``: computed once and shared"""
    import background_truth as bt

    init, pars, kappa, target = zoo_lanes(name)
    g = bt.truth_rhs(name)
    truth = np.array([truth_lane(g, init[k], pars[k], kappa[k], target) for k in range(LANES)]).T
    truth.setflags(write=False)
    return truth


@functools.lru_cache(maxsize=None)
def workload_rhs(name):
    import background_truth as bt
    import workloads

    return bt.truth_functions(workloads.model_for(name), workloads.artifact_for(name)[1].symbol_dictionary)


# ---- truth (c'): power-law inflation ---------------------------------------------------------------------------------------------
def power_law_formula(h_k):
    """the exact super-horizon tensor spectrum of power-law inflation with a ~ t^p, p = ``background_reference.P_POW``, for the mode
    that leaves the horizon (k = a H) at H = ``h_k``: 16 eps times ``modes_reference.power_law_formula``"""
    import background_reference as br

    eps = 1.0 / br.P_POW
    nu = 1.5 + eps / (1.0 - eps)
    amp = (2.0 ** (nu - 1.5) * math.gamma(nu) / math.gamma(1.5)) ** 2 * (1.0 - eps) ** (2.0 * nu - 1.0)
    return amp * 2.0 * np.asarray(h_k) ** 2 / math.pi**2


def power_law_exits(n_exit):
    """H at the exits ``n_exit`` on the attractor from t = 1: N = p ln t and H = p / t"""
    import background_reference as br

    return br.P_POW * np.exp(-np.asarray(n_exit, dtype=np.float64) / br.P_POW)


@functools.lru_cache(maxsize=None)
def power_law_truth(n_sub=N_SUB):
    """(2,): P_T of the two modes of ``modes_reference.POWER_N_EXIT`` at POWER_N_EVAL by DOP853 from the very initial conditions of
    the project -- the vacuum put in at a finite ``n_sub`` -- on the exact background"""
    import background_reference as br
    import background_truth as bt
    import modes_reference as mo

    art, p, _init, h_k = mo.power_law_case()
    g = bt.truth_functions(br.power_law_model(), art.symbol_dictionary)
    out = np.empty(2)
    for j, n_exit in enumerate(mo.POWER_N_EXIT):
        n0 = n_exit - n_sub
        y = br.power_law_exact(math.exp(n0 / br.P_POW) - 1.0)
        out[j] = truth_lane(g, y[:4], p, h_k[j] * math.exp(n_sub), mo.POWER_N_EVAL - n0)[0]
    return out


def power_law_start_error(n_sub=N_SUB):
    """what the start at a finite N_sub leaves: the worst relative difference of ``power_law_truth`` from the formula"""
    import modes_reference as mo

    return relative_error(power_law_truth(n_sub), power_law_formula(mo.power_law_case()[3]))


# ---- what the recorded errors allow in the observables -----------------------------------------------------------------------------
def stencil_bounds(k3, delta_r, delta_t):
    """What relative errors of at most ``delta_r`` of P_R and ``delta_t`` of P_T at each of three wavenumbers ``k3`` (..., 3) allow
    in the results of the three-point stencil: |d ln P| <= -ln(1 - delta) at each point, so a derivative moves by at most the sum of
    its weights' magnitudes times that: (n_s, alpha_s, n_t, r relative)."""
    from inflatox_amd.background import stencil_weights

    w1, w2 = stencil_weights(k3)
    lr, lt = -math.log1p(-delta_r), -math.log1p(-delta_t)
    return np.abs(w1).sum(-1).max() * lr, np.abs(w2).sum(-1).max() * lr, np.abs(w1).sum(-1).max() * lt, math.expm1(lr + lt)


# ---- the long run on the hyperbolic model ----------------------------------------------------------------------------------------
def hyper_error(solver):
    """the relative error of the twin's second stage against truth (b') on the lanes j = 0 and HYPER_K - 1 of every trajectory of
    ``modes_reference.hyper_states``, evaluated at N = HYPER_N_EVAL: (error, fewest accepted steps)"""
    import modes_reference as mo
    import workloads

    spec, art = workloads.artifact_for("hyperbolic")
    twin, g = TensorTwin(art), workload_rhs("hyperbolic")
    x, v = mo.hyper_states()
    cols = [0, mo.HYPER_K - 1]
    n_exit = mo.HYPER_N_EXIT[cols]
    start, h_exit, _status, starts = twin.stage1(spec.args, n_exit, x, v, N_SUB, max_err=mo.HYPER_MAX_ERR, solver=solver)
    got = twin.tensor_spectra(spec.args, n_exit, x, v, N_eval=mo.HYPER_N_EVAL, N_sub=N_SUB, max_err=mo.HYPER_MAX_ERR, solver=solver)
    assert np.all(got.status == TARGET)
    want = np.array([[truth_lane(g, start[b, j], spec.args, h_exit[b, j] * math.exp(N_SUB), mo.HYPER_N_EVAL - starts[j])[0] for j in range(2)] for b in range(mo.HYPER_B)])
    return relative_error(got.P_T, want), int(got.accepted.min())


def hyper_bound(solver):
    """``bound`` for the long run on the hyperbolic model"""
    import modes_reference as mo

    return 1e-10 + 2.0 * recorded()["hyperbolic"][f"{solver}/{mo.HYPER_MAX_ERR:g}"]


# ---- the recorded step-control error and the bound -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stepper_code_hash():
    """the hash of the code (comments aside) of the two headers that make the stepper: the state of the code a profile belongs to"""
    from inflatox_amd.compiler import _code_only

    h = hashlib.sha256()
    for f in ("inflx_background.h", "inflx_tensor.h"):
        with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
            h.update(_code_only(fh.read()).encode())
    return h.hexdigest()[:16]


def recorded():
    with open(PROFILE) as fh:
        return json.load(fh)


def bound(name, solver, max_err):
    """what the relative error against truth (b') may be: 1e-10 plus twice the host twin's recorded worst error for this model, solver
    and max_err -- a margin for other libm and contraction choices, not for defects"""
    return 1e-10 + 2.0 * recorded()["zoo"][f"{name}/{solver}/{max_err:g}"]


def power_law_bound():
    """truth (c'): twice the measured error that the start at N_SUB leaves against the formula"""
    return 2.0 * recorded()["power_law"]["start_error"]


def measure():
    import background_truth as bt
    import modes_reference as mo

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
                zoo[key], wron[key] = relative_error(got.out[0], truth[0]), wronskian_error(got.final, kappa)
                print(f"{name} {solver} max_err {max_err:g}: worst relative |twin - truth (b')| {zoo[key]:.3e}, Wronskian {wron[key]:.3e}, "
                      f"{got.accepted.min()} .. {got.accepted.max()} steps", flush=True)  # fmt: skip
    hyper = {}
    for solver in ("rk4", "rkf"):
        hyper[f"{solver}/{mo.HYPER_MAX_ERR:g}"], fewest = hyper_error(solver)
        print(f"hyperbolic {solver}: worst relative |twin - truth (b')| {hyper[f'{solver}/{mo.HYPER_MAX_ERR:g}']:.3e}, at least {fewest} steps", flush=True)
    start = power_law_start_error()
    print(f"power law: the start at N_sub = {N_SUB:g} leaves {start:.3e} against the formula (e^(-2 N_sub) = {math.exp(-2 * N_SUB):.3e})", flush=True)
    return {
        "stepper_code": stepper_code_hash(),
        "what": "worst relative |host twin - truth (b')| of P_T (own size), 65 lanes of background_truth.batch, kappa = H0 e^3, evaluated at the last e-fold sample "
                "of background_truth.samples_for, stop_at_end off; truth: DOP853 in N at rtol 1e-12 on the Euler-Lagrange background (tests/tensor_reference.py)",
        "bound": "tests assert 1e-10 + 2 x the value recorded here",
        "zoo": zoo,
        "wronskian": wron,
        "wronskian_what": "worst |W - 2 i kappa| / (2 kappa) of the same runs' accepted final states: recorded for information, asserted against the zoo bound",
        "hyperbolic": hyper,
        "hyperbolic_what": "the same for the second stage of the front end on the hyperbolic example model at max_err = 1e-10: modes_reference.hyper_states, the first and "
                           "the last of the 52 wavenumbers, N_sub = 3, evaluated at N = 6; every lane takes more than 256 accepted steps",
        "power_law": {"start_error": start, "N_sub": N_SUB},
        "power_law_what": "worst relative difference, P_T of the modes with N_exit = 3 and 4 at N = 10, between DOP853 from the project's initial conditions at "
                          "N_sub = 3 on the exact power-law background and the exact super-horizon formula; tests assert twice this",
    }  # fmt: skip


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    result = measure()
    with open(PROFILE, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
