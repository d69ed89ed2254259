"""Host twin and truths of the spectra sampled along a mode's evolution (csrc/inflx_evolution.h) -- TEST INFRASTRUCTURE.

``EvolutionTwin`` compiles tests/evolution_twin.cpp -- the generated headers, csrc/inflx_modes.h and csrc/inflx_evolution.h for the
CPU, contraction off -- and ``EvolutionTwin.spectra_evolution`` is ``inflatox_amd.background.spectra_evolution`` on the host: its
stage 1 from ``SampledTwin`` (or from a ``SampledSolution`` handed in), its stage 2 from the twin.  ``program`` builds the same file
with -DEVOLUTION_TWIN_MAIN as a stand-alone executable, with a sanitizer when asked, and ``run_program`` runs it.

The truth is ``modes_reference.truth_lane`` (b) at every sample: the lanes of ``modes_reference.zoo_lanes`` for the zoo models, and for
the hyperbolic example model -- which is no zoo model and has no ``background_truth.batch`` -- the 65 lanes of ``hyper_lanes``.  Errors
are ``modes_reference.relative_error``'s, relative to each spectrum's own scale.

``python tests/evolution_reference.py`` measures the twin's own step-control error against that truth at the samples of ``FRACTIONS``
-- per model and solver at max_err = 1e-8 and 1e-10 -- and the cross-check of ``transfer_from_spectra`` against
``transfer_functions`` between the two independent truths, and writes them to profiles/background_evolution.json; ``bound`` is what the
tests assert: 1e-10 plus twice the recorded value.
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

import modes_reference as mo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "inflatox_amd", "csrc")
PROFILE = os.path.join(ROOT, "profiles", "background_evolution.json")
_DP = C.POINTER(C.c_double)

LANES = mo.LANES
MAX_ERRS = mo.MAX_ERRS
FRACTIONS = np.array([0.0, 0.25, 0.5, 0.75, 1.0])  # the samples of a zoo run, as fractions of its target
CPU_MODELS = ("hyperbolic", "fuzz0", "fuzz2")  # what the CPU suite runs; the GPU suite runs background_truth.GPU_MODELS
HYPER_TARGET = 1.0
COMPLETE, ENDED, NONFINITE, REJECTED, UNDERFLOW, TARGET = 0, 1, 2, 3, 4, 5


class EvolutionLanes(NamedTuple):
    """What ``EvolutionTwin.lanes`` returns: ``out`` (22, n), ``N_end``, ``status``, ``accepted`` and ``final`` as ``modes_reference.TwinLanes``,
    ``sampled`` (S, 6, n) as ``InflatoxDevLib.mode_evolution``'s, ``cursor`` (n,) and ``step_of`` (n, S): the accepted step that emitted
    each sample (0: the initial state; -1: not emitted)."""

    out: np.ndarray
    N_end: np.ndarray
    status: np.ndarray
    accepted: np.ndarray
    final: np.ndarray
    sampled: np.ndarray
    cursor: np.ndarray
    step_of: np.ndarray


class TwinEvolution(NamedTuple):
    """``inflatox_amd.background.SpectraEvolution``'s members (``end``: a ``modes_reference.TwinSpectra``), plus ``accepted`` (B, K)"""

    P_R: np.ndarray
    P_S: np.ndarray
    C_RS: np.ndarray
    N: np.ndarray
    eps_H: np.ndarray
    k: np.ndarray
    end: mo.TwinSpectra
    status: np.ndarray
    accepted: np.ndarray


def _sources():
    return [os.path.join(CSRC, f) for f in ("inflx_background.h", "inflx_modes.h", "inflx_evolution.h")] + [os.path.join(HERE, "evolution_twin.cpp")]


def _build(artifact, flags, suffix, cxx="g++"):
    """tests/evolution_twin.cpp compiled with ``flags`` from the artefact's generated headers, cached by content: the path"""
    texts = (artifact._build[0], artifact.eom_header_text(), artifact.kinematics_header_text(), artifact.masses_header_text())
    sources = _sources()
    tag = hashlib.sha1(("".join(texts) + "".join(open(f).read() for f in sources) + " ".join(flags)).encode()).hexdigest()[:16]
    d = os.path.join(tempfile.gettempdir(), "inflx_evolution_twin")
    os.makedirs(d, exist_ok=True)
    hdr, eom_hdr, kin_hdr, mass_hdr, target = (os.path.join(d, f"{tag}{s}") for s in (".h", ".eom.h", ".kin.h", ".mass.h", suffix))
    if not os.path.exists(target):
        for path, text in zip((hdr, eom_hdr, kin_hdr, mass_hdr), texts):
            with open(path, "w") as fh:
                fh.write(text)
        tmp = target + f".{os.getpid()}.tmp"
        cmd = [cxx, "-std=c++17", *flags, "-fno-fast-math", "-Wno-unknown-pragmas", f"-I{CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"', f'-DINFLX_EOM_HEADER="{eom_hdr}"',
               f'-DINFLX_KIN_HEADER="{kin_hdr}"', f'-DINFLX_MASS_HEADER="{mass_hdr}"', sources[-1], "-o", tmp]  # fmt: skip
        subprocess.run(cmd, check=True)
        os.replace(tmp, target)
    return target


class EvolutionTwin:
    """tests/evolution_twin.cpp built for the CPU from an artefact's generated headers, contraction off like ``ModesTwin``"""

    def __init__(self, artifact, cxx: str = "g++", contract: str = "off"):
        self.artifact = artifact
        flags = ["-O2", "-fPIC", "-shared", f"-ffp-contract={contract}", *(["-mfma"] if contract != "off" else [])]
        self.lib = C.CDLL(_build(artifact, flags, ".so", cxx))
        self.lib.twin_evolution.argtypes = [_DP, C.c_size_t, _DP, _DP, _DP, _DP, _DP, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_double, C.c_double, C.c_int, _DP,
                                            _DP, _DP, C.POINTER(C.c_uint)]  # fmt: skip
        self.lib.twin_evolution.restype = None

    def lanes(self, pars, init, kappa, n_target, shift, samples, max_steps=1_000_000, max_err=1e-8, solver="rkf", *, dt=None, stop_at_end=True) -> EvolutionLanes:
        """``InflatoxDevLib.mode_evolution``'s arguments: init (n, 4), kappa, n_target (NaN: none) and shift (n,), samples (S,)"""
        init = np.ascontiguousarray(init, dtype=np.float64)
        n = init.shape[0]
        p = np.ascontiguousarray(pars, dtype=np.float64)
        kappa, target, shift = (np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,))) for a in (kappa, n_target, shift))
        pts = np.ascontiguousarray(samples, dtype=np.float64)
        S = pts.size
        out, sampled, lanes = np.empty((22, n)), np.empty((S, 6, n)), np.empty((n, 27))
        step_of = np.full((n, S), 0xFFFFFFFF, dtype=np.uint32)
        self.lib.twin_evolution(p.ctypes.data_as(_DP), 0 if p.ndim == 1 else p.shape[1], init.ctypes.data_as(_DP), kappa.ctypes.data_as(_DP), target.ctypes.data_as(_DP),
                                shift.ctypes.data_as(_DP), pts.ctypes.data_as(_DP), S, n, int(max_steps), 1 if solver == "rkf" else 0, float(max_err), float(dt or 0.0),
                                int(stop_at_end), out.ctypes.data_as(_DP), sampled.ctypes.data_as(_DP), lanes.ctypes.data_as(_DP),
                                step_of.ctypes.data_as(C.POINTER(C.c_uint)))  # fmt: skip
        return EvolutionLanes(out, lanes[:, 1], lanes[:, 0].astype(np.int8), lanes[:, 2].astype(np.int64), lanes[:, 3:26], sampled, lanes[:, 26].astype(np.int64),
                              step_of.astype(np.int64) - (step_of == 0xFFFFFFFF) * (1 << 32))  # fmt: skip

    def spectra_evolution(self, pars, N_exit, samples, fields_init, derivatives_init, *, since="exit", N_eval=None, N_sub=5.0, max_steps=1_000_000, max_err=1e-8,
                          solver="rkf", dt=None, stop_at_end=True, stage1=None) -> TwinEvolution:  # fmt: skip
        """``inflatox_amd.background.spectra_evolution``'s arguments (checked there, not here) and its two stages, in its own words;
        ``stage1`` as in ``ModesTwin.power_spectra``"""
        start, h_exit, status1, starts = mo.ModesTwin.stage1(self, pars, N_exit, fields_init, derivatives_init, N_sub, max_steps, max_err, solver, dt, stop_at_end, stage1)
        n_exit = np.ascontiguousarray(N_exit, dtype=np.float64)
        pts = np.ascontiguousarray(samples, dtype=np.float64)
        p = np.ascontiguousarray(pars, dtype=np.float64)
        B, K = start.shape[:2]
        S = pts.size
        kappa = h_exit * math.exp(N_sub)
        status = np.repeat(status1[:, None], K, axis=1).reshape(-1)
        out, n_end, accepted = np.full((22, B * K), np.nan), np.full(B * K, np.nan), np.zeros(B * K, dtype=np.int64)
        sampled = np.full((S, 6, B * K), np.nan)
        run = np.flatnonzero((np.isfinite(start).all(axis=2) & np.isfinite(h_exit)).reshape(-1))
        lane_start = np.tile(starts, B)
        shift = np.tile(np.full(K, -N_sub) if since == "exit" else starts, B)
        if run.size:
            target = np.full(run.size, np.nan) if N_eval is None else N_eval - lane_start[run]
            lane_p = p if p.ndim == 1 else np.ascontiguousarray(np.repeat(p, K, axis=0)[run])
            got = self.lanes(lane_p, start.reshape(-1, 4)[run], kappa.reshape(-1)[run], target, shift[run], pts, max_steps, max_err, solver, dt=dt, stop_at_end=stop_at_end)
            valid = got.status == (ENDED if N_eval is None else TARGET)
            out[:, run] = np.where(valid[None, :], got.out, np.nan)
            n_end[run] = np.where(got.status == ENDED, got.N_end, np.nan)
            status[run] = got.status
            accepted[run] = got.accepted
            sampled[:, :, run] = got.sampled
        out = out.reshape(22, B, K)
        offset = lane_start.reshape(B, K)
        q = out[3:11].reshape(2, 2, 2, B, K)
        modes = np.moveaxis(q[:, :, 0] + 1j * q[:, :, 1], (0, 1), (2, 3))
        end = mo.TwinSpectra(out[0], out[1], out[2], h_exit * np.exp(n_exit)[None, :], out[19] + offset, out[21], modes, n_end.reshape(B, K) + offset,
                             status.reshape(B, K), accepted.reshape(B, K))  # fmt: skip
        planes = np.moveaxis(sampled, 0, 2).reshape(6, B, K, S)
        where = pts[None, None, :] + (n_exit[None, :, None] if since == "exit" else 0.0)
        n = np.where(np.isnan(planes[3]), np.nan, np.broadcast_to(where, planes[3].shape))
        return TwinEvolution(planes[0], planes[1], planes[2], n, planes[5], end.k, end, end.status, end.accepted)


# ---- the stand-alone program -----------------------------------------------------------------------------------------------------
def program(artifact, sanitize: str | None = "address,undefined"):
    """tests/evolution_twin.cpp with -DEVOLUTION_TWIN_MAIN as an executable of its own, with -fsanitize=``sanitize``: its path"""
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-DEVOLUTION_TWIN_MAIN"]
    if sanitize:
        flags += [f"-fsanitize={sanitize}", "-fno-sanitize-recover=all"]
    return _build(artifact, flags, ".san" if sanitize else ".exe")


def run_program(exe, pars, init, kappa, n_target, shift, samples, max_steps, max_err=1e-8, solver="rkf", dt=None, stop_at_end=True):
    """the program on n lanes: (status (n,), cursor (n,), sampled (S, 6, n)); raises when it fails, a sanitizer's report included"""
    init = np.asarray(init, dtype=np.float64)
    n, S = init.shape[0], len(samples)
    p = np.broadcast_to(np.asarray(pars, dtype=np.float64), (n, np.asarray(pars).shape[-1]))
    rows = [[n, p.shape[1], S, int(max_steps), 1 if solver == "rkf" else 0, int(stop_at_end), repr(float(max_err)), repr(float(dt or 0.0))]]
    rows += [p.reshape(-1), init.reshape(-1)] + [np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)) for a in (kappa, n_target, shift)] + [np.asarray(samples, dtype=np.float64)]
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as fh:
        for row in rows:
            fh.write(" ".join(v if isinstance(v, str) else repr(float(v)) if isinstance(v, (float, np.floating)) else str(v) for v in row) + "\n")
        path = fh.name
    try:
        proc = subprocess.run([exe, path], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    finally:
        os.remove(path)
    if proc.returncode != 0 or proc.stderr.strip():
        raise RuntimeError(f"{exe} exited with {proc.returncode}:\n{proc.stderr}")
    table = np.array([[float(v) for v in line.split()] for line in proc.stdout.strip().splitlines()])
    assert table.shape == (n, 2 + 6 * S)
    return table[:, 0].astype(np.int8), table[:, 1].astype(np.int64), table[:, 2:].T.reshape(S, 6, n)


# ---- lanes, truths and the recorded error -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin_for(name):
    import background_truth as bt
    import workloads

    return EvolutionTwin(workloads.artifact_for(name)[1] if name == "hyperbolic" else bt.host_artifact(name))


@functools.lru_cache(maxsize=None)
def modes_twin_for(name):
    import workloads

    return mo.ModesTwin(workloads.artifact_for(name)[1]) if name == "hyperbolic" else mo.zoo_twin(name)


@functools.lru_cache(maxsize=None)
def hyper_lanes(n_lanes=LANES):
    """``modes_reference.zoo_lanes``' counterpart for the hyperbolic example model: (init (n, 4), pars (n, 3), kappa (n,), target) -- the
    turning states of ``modes_reference.hyper_states``, one parameter row for all, kappa = H0 e^N_SUB, evaluated at N = HYPER_TARGET"""
    import workloads

    spec, _art = workloads.artifact_for("hyperbolic")
    x, v = mo.hyper_states(n_lanes, seed=11)
    init = np.concatenate([x, v], axis=1)
    pars = np.ascontiguousarray(np.tile(np.asarray(spec.args, dtype=np.float64), (n_lanes, 1)))
    kappa = mo.friedmann_h(modes_twin_for("hyperbolic"), pars, init) * math.exp(mo.N_SUB)
    return init, pars, kappa, HYPER_TARGET


def lanes_of(name, n_lanes=LANES):
    return hyper_lanes(n_lanes) if name == "hyperbolic" else mo.zoo_lanes(name, n_lanes)


def rhs_of(name):
    return mo.workload_rhs(name) if name == "hyperbolic" else mo._zoo_rhs(name)


def samples_of(name):
    """the five samples of a model's run: FRACTIONS of its target (the last one is the target itself, bit for bit)"""
    return FRACTIONS * lanes_of(name)[3]


def vacuum(g, init, p, kappa):
    """(P_R, P_S, C_RS, eps_H, t) of the initial state from the truth's own model functions"""
    V, kin = g(*init, 1.0, p)[2:4]
    H0 = math.sqrt((V + 0.5 * kin) / 3.0)
    eps = g(*init, H0, p)[4]
    amp = kappa * kappa / (8.0 * math.pi**2 * eps)
    return amp, amp, 0.0, eps, 0.0


@functools.lru_cache(maxsize=None)
def truth_at_samples(name):
    """(5 samples, 5, LANES): ``modes_reference.truth_lane`` of ``lanes_of(name)`` at every sample of ``samples_of(name)`` (the vacuum at
    the sample 0; ``modes_reference.zoo_truth`` at the last one of a zoo model): computed once and shared"""
    init, pars, kappa, _target = lanes_of(name)
    g, pts = rhs_of(name), samples_of(name)
    truth = np.empty((pts.size, 5, LANES))
    for s, x in enumerate(pts):
        if x == 0.0:
            truth[s] = np.array([vacuum(g, init[k], pars[k], kappa[k]) for k in range(LANES)]).T
        elif s == pts.size - 1 and name != "hyperbolic":
            truth[s] = mo.zoo_truth(name)
        else:
            truth[s] = np.array([mo.truth_lane(g, init[k], pars[k], kappa[k], x) for k in range(LANES)]).T
    truth.setflags(write=False)
    return truth


def sample_error(sampled, truth):
    """the worst ``modes_reference.relative_error`` over the samples: ``sampled`` (S, >= 3, n), ``truth`` (S, >= 3, n)"""
    return max(mo.relative_error(sampled[s, :3], truth[s, :3]) for s in range(truth.shape[0]))


@functools.lru_cache(maxsize=None)
def stepper_code_hash():
    """the hash of the code (comments aside) of the three headers that make a sampled lane: the state of the code a profile belongs to"""
    from inflatox_amd.compiler import _code_only

    h = hashlib.sha256()
    for f in ("inflx_background.h", "inflx_modes.h", "inflx_evolution.h"):
        with open(os.path.join(CSRC, f), encoding="utf-8") as fh:
            h.update(_code_only(fh.read()).encode())
    return h.hexdigest()[:16]


def recorded():
    with open(PROFILE) as fh:
        return json.load(fh)


def bound(name, solver, max_err):
    """what the relative error against truth (b) may be at any sample: 1e-10 plus twice the host twin's recorded worst error for this
    model, solver and max_err"""
    return 1e-10 + 2.0 * recorded()["zoo"][f"{name}/{solver}/{max_err:g}"]


# ---- the cross-check with the super-horizon transfer functions -------------------------------------------------------------------
CROSS_N_SUB = 3.0
CROSS_N_EXIT = 3.0  # the mode starts with the trajectory
CROSS_MAX_ERR = 1e-10


def cross_case():
    """(parameter row, fields (1, 2), velocities (1, 2)): the first turning trajectory of ``modes_reference.hyper_states``"""
    import workloads

    spec, _art = workloads.artifact_for("hyperbolic")
    x, v = mo.hyper_states(1)
    return np.asarray(spec.args, dtype=np.float64), x, v


def transfer_from(p_r, p_s, c_rs, ref):
    """``inflatox_amd.background.transfer_from_spectra`` restated on three arrays (S,): (T_RS, T_SS)"""
    t_ss = np.sqrt(p_s / p_s[ref])
    return (c_rs / t_ss - c_rs[ref]) / p_s[ref], t_ss


CROSS_AFTER_EXIT = np.array([4.0, 4.25, 4.5, 4.75, 5.0])  # e-folds after the exit; the first is the reference sample


def cross_lane(solver="rkf"):
    """The lane of the cross-check and the state at its reference sample: (init (4,), kappa, local samples (5,), reference state (4,)),
    from the host twins' own stage 1 (``SampledTwin``) at CROSS_MAX_ERR: the mode starts with the trajectory, leaves the horizon at
    N = CROSS_N_EXIT and is sampled CROSS_AFTER_EXIT e-folds later; the trajectory ends inflation at N = 8.16."""
    from background_sampled_reference import SampledTwin

    p, x, v = cross_case()
    art = modes_twin_for("hyperbolic").artifact
    pts = np.concatenate([[CROSS_N_EXIT], CROSS_N_EXIT + CROSS_AFTER_EXIT[:1]])
    states, meta = SampledTwin(art).solve(p, [*x[0], *v[0]], pts, 1_000_000, solver, CROSS_MAX_ERR, None, False)
    assert meta["status"] == TARGET
    init = np.array([*x[0], *v[0]])
    return init, states[0, 4] * math.exp(CROSS_N_SUB), CROSS_N_SUB + CROSS_AFTER_EXIT, np.array(states[1, :4])


def cross_truths():
    """(T_RS, T_SS) (2, 5) of the two independent truths at the samples after the reference: from ``modes_reference.truth_lane`` through
    ``transfer_from``, and from ``transfer_reference.truth_lane`` started at the reference state with its default dq/dN"""
    import transfer_reference as tr

    p, _x, _v = cross_case()
    init, kappa, local, ref_state = cross_lane()
    g = mo.workload_rhs("hyperbolic")
    spectra = np.array([mo.truth_lane(g, init, p, kappa, n)[:3] for n in local]).T
    from_modes = np.array(transfer_from(*spectra, 0))
    got = tr.truth_lane(tr.workload_rhs("hyperbolic"), ref_state, p, CROSS_AFTER_EXIT[1:] - CROSS_AFTER_EXIT[0])
    from_transfer = np.concatenate([[[0.0], [1.0]], np.array([got[:, 1], got[:, 0]])], axis=1)
    return from_modes, from_transfer, spectra


def cross_twins(solver="rkf"):
    """the same from the two host twins at CROSS_MAX_ERR: ``EvolutionTwin.lanes`` and ``TransferTwin.solve``; and the twin's spectra"""
    import transfer_reference as tr

    p, _x, _v = cross_case()
    init, kappa, local, ref_state = cross_lane()
    ev = twin_for("hyperbolic").lanes(p, init[None], kappa, np.nan, 0.0, local, max_err=CROSS_MAX_ERR, solver=solver, stop_at_end=False)
    assert ev.status[0] == TARGET and ev.accepted[0] >= 257
    spectra = ev.sampled[:, :3, 0].T
    from_modes = np.array(transfer_from(*spectra, 0))
    sol = tr.TransferTwin(modes_twin_for("hyperbolic").artifact).solve(p, CROSS_AFTER_EXIT - CROSS_AFTER_EXIT[0], ref_state[None, :2], ref_state[None, 2:],
                                                                       max_err=CROSS_MAX_ERR, solver=solver, stop_at_end=False)  # fmt: skip
    assert sol.status[0] == TARGET
    return from_modes, np.array([sol.T_RS[0], sol.T_SS[0]]), spectra


def measure():
    import background_truth as bt

    zoo = {}
    for name in ("hyperbolic", *bt.GPU_MODELS):
        init, pars, kappa, target = lanes_of(name)
        truth, pts = truth_at_samples(name), samples_of(name)
        assert np.isfinite(truth).all()
        for solver in ("rk4", "rkf"):
            for max_err in MAX_ERRS:
                got = twin_for(name).lanes(pars, init, kappa, target, 0.0, pts, max_err=max_err, solver=solver, stop_at_end=False)
                assert np.all(got.status == TARGET) and np.isfinite(got.sampled).all(), (name, solver, max_err, got.status)
                key = f"{name}/{solver}/{max_err:g}"
                zoo[key] = sample_error(got.sampled, truth)
                print(f"{name} {solver} max_err {max_err:g}: worst relative |twin - truth (b)| over the five samples {zoo[key]:.3e}", flush=True)
    (m_rs, m_ss), (t_rs, t_ss), _spectra = cross_truths()
    cross = {"truth_T_RS": float(np.max(np.abs(m_rs - t_rs))), "truth_T_SS": float(np.max(np.abs(m_ss - t_ss))),
             "T_RS": [float(v) for v in m_rs], "T_SS": [float(v) for v in m_ss], "T_RS_transfer": [float(v) for v in t_rs], "T_SS_transfer": [float(v) for v in t_ss]}  # fmt: skip
    for solver in ("rk4", "rkf"):
        (a_rs, a_ss), (b_rs, b_ss), _sp = cross_twins(solver)
        cross[f"twin_T_RS/{solver}"] = float(np.max(np.abs(a_rs - m_rs)) + np.max(np.abs(b_rs - t_rs)))
        cross[f"twin_T_SS/{solver}"] = float(np.max(np.abs(a_ss - m_ss)) + np.max(np.abs(b_ss - t_ss)))
    print("cross-check:", json.dumps(cross, indent=1), flush=True)
    return {
        "stepper_code": stepper_code_hash(),
        "what": "worst relative |host twin - truth (b)| over P_R, P_S (own size) and C_RS (sqrt(P_R P_S)) and over the five samples at 0, 1/4, 1/2, 3/4 and 1 x the target: "
                "65 lanes of modes_reference.zoo_lanes (hyperbolic: evolution_reference.hyper_lanes, to N = 1), kappa = H0 e^3, stop_at_end off; truth: "
                "modes_reference.truth_lane at every sample, the vacuum at 0 (tests/evolution_reference.py)",
        "bound": "tests assert 1e-10 + 2 x the value recorded here",
        "zoo": zoo,
        "cross": cross,
        "cross_what": "the first trajectory of modes_reference.hyper_states, N_sub = 3, the mode leaving the horizon at N = 3: T_RS and T_SS from the sample 4 e-folds "
                      "after the exit to those 4.25, 4.5, 4.75 and 5 e-folds after it (the trajectory ends inflation at N = 8.16, so no later sample exists). "
                      "truth_*: worst absolute difference between transfer_from_spectra of modes_reference.truth_lane and transfer_reference.truth_lane started at the "
                      "reference state with its default dq/dN; twin_*: the two host twins' (max_err 1e-10) summed worst absolute differences from their own truths. Tests "
                      "assert |twin - twin| <= 2 x truth_* + twin_*",
    }  # fmt: skip


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    result = measure()
    with open(PROFILE, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
