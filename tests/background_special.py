"""Special-function models under the background solver -- TEST INFRASTRUCTURE shared by tests/test_background_special.py (host builds)
and tests/test_background_special_gpu.py (the device).

The models are ``background_truth.special_model``: ``bessel_skew`` and ``kummer_curved`` are the value models, with seeded batches and
truths like every zoo model; ``j52_wall`` is the model of the status tests, whose lanes are literal and listed here.

The wall: V = b + a J_5/2(phi) - c phi on a flat field space, a = 1, b = 2 c + 10.  J_nu is defined for phi >= 0 only.  A field that
starts just above phi = 0 and moves towards it is turned round by the slope c before it gets there when c is large; its first
adaptive trial steps are long enough for a Runge-Kutta stage to land at phi < 0, where the function returns NaN and sets its bit,
the trial is not finite and the step control retries it at a fifth of the step (csrc/inflx_background.h, inflx_bg_step_taken).  Such a
lane finishes COMPLETE with every stored state inside the domain and the bit set: ``WALL_RECOVERED``.  With a small c the field
reaches phi = 0: ``WALL_EXIT``.
"""

from __future__ import annotations

import functools
import math
import os
import sys

if __name__ == "__main__":  # run as a script (the measurements at the end): the repository root on the path, as under pytest
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

import background_truth as bt
from background_reference import BackgroundTwin, Restatement

SF_EDOM = 1  # csrc/inflx_sf.h: INFLX_SF_EDOM
LANES = 16  # trajectories of a value model that are integrated, on the host and on the device
STATES = 65  # states of a point-level call: a wavefront and one
WALL_ROWS, WALL_MAX_ERR = 120, 1e-6

#: per solver, the lanes (c, (phi, theta, phidot, thetadot)) that leave the domain in a trial step and recover; adaptive, WALL_ROWS rows
WALL_RECOVERED = {
    "rkf": ((1e4, (5.2e-5, 0.0, -1.0, 0.0)), (1e4, (6e-5, 0.0, -1.0, 0.0))),
    "rk4": ((1e4, (5.2e-5, 0.0, -1.0, 0.0)), (1e4, (6e-5, 0.0, -1.0, 0.0)), (1e3, (5.2e-4, 0.0, -1.0, 0.0))),
}
#: the lane that reaches phi = 0, and the fixed step of its fixed-step run
WALL_EXIT = (1.0, (5.2e-4, 0.0, -1.0, 0.0))
WALL_EXIT_DT = 1e-5
#: lanes that stay far inside the domain (phi >= 0.5 throughout WALL_ROWS rows): the company of the leaving lane
WALL_INSIDE_C = 1.0


def wall_pars(c):
    """the parameter row of ``j52_wall`` for the slope c: a = 1, b = 2 c + 10"""
    art = bt.host_artifact("j52_wall")
    p = np.zeros(art.n_parameters)
    for name, value in (("a", 1.0), ("b", 2.0 * c + 10.0), ("c", c)):
        p[int(art.symbol_dictionary[name][5:-1])] = value
    return p


def wall_lanes(lanes):
    """(init (n, 4), pars (n, 3)) of lanes given as (c, state)"""
    return np.array([s for _, s in lanes], dtype=np.float64), np.array([wall_pars(c) for c, _ in lanes])


def wall_inside(n=7):
    """n lanes of ``j52_wall`` that start at phi in [1, 2.5] with small velocities and stay inside the domain"""
    rng = np.random.default_rng(4152)
    init = np.stack([rng.uniform(1.0, 2.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(-0.1, 0.1, n), rng.uniform(-0.1, 0.1, n)], axis=1)
    return init, np.tile(wall_pars(WALL_INSIDE_C), (n, 1))


class CountingRestatement(Restatement):
    """The restatement with a count of the trial steps that were not finite"""

    def __init__(self, eom, p):
        super().__init__(eom, p)
        self.nonfinite_trials = 0

    def trial(self, method, y, f, h, adaptive):
        out, err = super().trial(method, y, f, h, adaptive)
        if not (all(math.isfinite(v) for v in out) and math.isfinite(err)):
            self.nonfinite_trials += 1
        return out, err


@functools.lru_cache(maxsize=None)
def twin(name, contract="off"):
    return BackgroundTwin(bt.host_artifact(name), contract=contract)


def rows_of(sol):
    """(B, rows, 7) of an ``EoMSolution``: y[0..5] and t, the columns of the twins' rows"""
    return np.concatenate([np.asarray(sol.states), np.asarray(sol.N)[..., None], np.asarray(sol.t)[..., None]], axis=2)


def matched_difference(a, b, eom, p):
    """Two adaptive runs of one lane, rows (R, 7) = y[0..5], t, compared at matched accepted steps.  The step sizes of an adaptive
    run follow the error estimate, a difference of nearly equal numbers, so two roundings of the same algorithm accept steps whose t
    differ in the last digits, and where the state changes fast (chi' = c = 1e4 on the wall) that alone moves the state by
    y'(t) dt.  Returned: (worst |a.y - b.y - f(b.y) (a.t - b.t)| of each value's scale -- the difference of the states carried to
    the same time, to first order --, worst |a.t - b.t| / b.t)."""
    rhs = Restatement(eom, p).rhs
    f = np.array([rhs(list(row[:6]))[0] for row in b])
    dt = (a[:, 6] - b[:, 6])[:, None]
    state = float(np.max(np.abs(a[:, :6] - b[:, :6] - f * dt) / bt.scale_of(b[:, :6])))
    return state, float(np.max(np.abs(dt[1:, 0]) / b[1:, 6]))


def wall_recovered_twins(solver, contract):
    """(rows (n, WALL_ROWS, 7) of the ``WALL_RECOVERED`` lanes of the solver on the host twin, their parameter rows)"""
    init, pars = wall_lanes(WALL_RECOVERED[solver])
    return np.array([twin("j52_wall", contract).solve(pars[k], init[k], WALL_ROWS, solver, max_err=WALL_MAX_ERR)[0] for k in range(init.shape[0])]), pars


def measure_wall_d():
    """{solver: {"state", "t"}}: ``matched_difference`` of the host twin with FMA contraction against the twin without, worst lane"""
    eom = bt.truth_rhs("j52_wall")
    d = {}
    for solver in ("rk4", "rkf"):
        (fast, pars), (off, _) = wall_recovered_twins(solver, "fast"), wall_recovered_twins(solver, "off")
        pairs = [matched_difference(fast[k], off[k], eom, pars[k]) for k in range(off.shape[0])]
        d[solver] = dict(state=max(s for s, _ in pairs), t=max(t for _, t in pairs), unmatched=float(np.max(np.abs(fast - off) / bt.scale_of(off))))
    return d


def wall_bound(solver):
    """(bar on the matched states, bar on the relative time difference): 1e-10 + 2 d each, d as recorded in the profile"""
    import json

    with open(_profile_path("special")) as fh:
        d = json.load(fh)["d_j52_wall"][solver]
    return 1e-10 + 2.0 * d["state"], 1e-10 + 2.0 * d["t"]


# ---- every other family on bessel_skew: the device against the host twin, lane by lane -------------------------------------------
# Fixed dt, so that the accepted steps of all builds are the same and a lane-by-lane bar applies: 1e-10 + 2 d of each value's scale,
# d the host twin's difference with and without FMA contraction on the same call.  `python tests/background_special.py` measures d
# on the CPU and writes it into the family's profiles/background_<family>.json under "d_bessel_skew".
PARITY_MODEL = "bessel_skew"
PARITY_LANES, PARITY_DT = 8, 2e-2
PARITY_FAMILIES = ("transfer", "modes", "tensor", "evolution", "deltan", "crossing", "inflation_end", "distribution")
PROFILE_OF = {"inflation_end": "crossing"}  # (the family whose profile holds the figure: inflation_end is in the crossing object)


def _fields(result, names):
    return {n: np.asarray(getattr(result, n)) for n in names}


def parity_results(family, solver, kind):
    """{name: array} of one call of ``family`` on the first 8 lanes of ``batch("bessel_skew")`` at a fixed step; ``kind``: "off" or
    "fast" (the host twin built without / with FMA contraction) or "gpu" (``inflatox_amd.background`` on the device)"""
    import kinematics_reference as kr

    init, pars = (np.array(a[:PARITY_LANES]) for a in bt.batch(PARITY_MODEL))
    x, v = init[:, :2], init[:, 2:]
    gpu = kind == "gpu"
    art = bt.device_artifact(PARITY_MODEL) if gpu else bt.host_artifact(PARITY_MODEL)
    if gpu:
        from inflatox_amd import background as bg
    kw = dict(solver=solver, dt=PARITY_DT, stop_at_end=False)
    if family == "transfer":
        import transfer_reference as tr

        samples = [0.2, 0.5, 1.0]
        r = bg.transfer_functions(art, pars, samples, x, v, 400, **kw) if gpu else tr.TransferTwin(art, contract=kind).solve(pars, samples, x, v, 400, **kw)
        return _fields(r, ("T_SS", "T_RS", "t", "N", "eps_H", "states", "n_stored", "T_SS_end", "T_RS_end", "status"))
    if family in ("modes", "tensor", "evolution"):
        spectra = dict(N_eval=1.6, N_sub=0.5, max_steps=2000, **kw)
        if family == "modes":
            import modes_reference as mo

            r = bg.power_spectra(art, pars, [0.8], x, v, **spectra) if gpu else mo.ModesTwin(art, contract=kind).power_spectra(pars, [0.8], x, v, **spectra)
            return _fields(r, ("P_R", "P_S", "C_RS", "k", "N", "eps_H", "modes", "status"))
        if family == "tensor":
            import tensor_reference as te

            r = bg.tensor_spectra(art, pars, [0.8], x, v, **spectra) if gpu else te.TensorTwin(art, contract=kind).tensor_spectra(pars, [0.8], x, v, **spectra)
            return _fields(r, ("P_T", "k", "N", "eps_H", "modes", "status"))
        import evolution_reference as ev

        r = (bg.spectra_evolution(art, pars, [0.8], [0.2, 0.5], x, v, **spectra) if gpu
             else ev.EvolutionTwin(art, contract=kind).spectra_evolution(pars, [0.8], [0.2, 0.5], x, v, **spectra))  # fmt: skip
        return {**_fields(r, ("P_R", "P_S", "C_RS", "N", "eps_H", "k", "status")), **{"end_" + n: a for n, a in _fields(r.end, ("P_R", "P_S", "C_RS", "status")).items()}}
    if family == "deltan":
        import deltan_reference as dr

        # the model never ends inflation: the surface of every stencil is H = 0.98 H_0 of its centre, which all nine members start above
        h_end = 0.98 * kr.zoo_states(PARITY_MODEL)[0][:PARITY_LANES, 4]
        dn = dict(h=1e-2, velocity="fixed", H_end=h_end, max_steps=2000, max_err=1e-10, solver=solver, dt=PARITY_DT)
        r = bg.delta_N(art, pars, x, v, **dn) if gpu else dr.DeltaNTwin(art, contract=kind).delta_n(pars, x, v, **dn).dn
        return _fields(r, ("N", "H_end", "N_members", "N_I", "N_IJ", "N_cov", "grad2", "f_NL", "P_zeta", "status"))
    if family == "crossing":
        import crossing_reference as cr

        # ln(a H) of every lane counted from its own ln H_0
        offset = np.log(kr.zoo_states(PARITY_MODEL)[0][:PARITY_LANES, 4])
        ln_k = np.array([0.3, 0.8])
        if gpu:
            r = bg.horizon_crossings(art, pars, ln_k, x, v, offset=offset, max_steps=400, max_err=1e-8, **kw)
            return _fields(r, ("states", "N", "t", "eps_H", "n_stored", "status"))
        twin = cr.CrossingTwin(art, contract=kind)
        runs = [twin.solve(pars[k], init[k], ln_k, 400, offset[k], solver, 1e-8, PARITY_DT, False) for k in range(PARITY_LANES)]
        out = np.array([o for o, _ in runs])
        return dict(states=out[:, :, :5], N=out[:, :, 5], t=out[:, :, 6], eps_H=out[:, :, 7], n_stored=np.array([m["n_stored"] for _, m in runs]),
                    status=np.array([m["status"] for _, m in runs]))  # fmt: skip
    if family == "inflation_end":
        import crossing_reference as cr

        # (no lane of this model ends inflation: what is compared is that every lane runs its 200 steps and reports so)
        if gpu:
            r = bg.inflation_end(art, pars, x, v, max_steps=200, max_err=1e-8, solver=solver, dt=PARITY_DT)
            return dict(state=np.asarray(r.state), eps_H=np.asarray(r.eps_H), status=np.asarray(r.status))
        twin = cr.CrossingTwin(art, contract=kind)
        runs = [twin.end(pars[k], init[k], 200, solver, 1e-8, PARITY_DT) for k in range(PARITY_LANES)]
        out = np.array([o for o, _ in runs])
        return dict(state=out[:, :5], eps_H=out[:, 7], status=np.array([m["status"] for _, m in runs]))
    if family == "distribution":
        import distribution_reference as di

        # (the twin has one build: d = 0, and the counts are integers)
        run = dict(seed=11, noise_scale=0.5, max_steps=100, solver=solver, dt=PARITY_DT)
        r = bg.stochastic_distribution(art, pars, x, v, 8, 4, (0.0, 1.0), **run) if gpu else di.DistributionTwin(art).run(pars, init, 8, 4, (0.0, 1.0), **run)
        return _fields(r, ("hist", "below", "above", "counts"))
    raise KeyError(family)


def parity_difference(a, b):
    """worst |a - b| over the floating-point members of two ``parity_results``, of each value's scale; NaN where NaN, and integer
    members (statuses, counts) equal"""
    worst = 0.0
    assert a.keys() == b.keys()
    for name in a:
        u, w = np.asarray(a[name]), np.asarray(b[name])
        assert u.shape == w.shape, (name, u.shape, w.shape)
        if np.issubdtype(w.dtype, np.integer) or np.issubdtype(u.dtype, np.integer):
            assert np.array_equal(u.astype(np.int64), w.astype(np.int64)), (name, u, w)
            continue
        assert np.array_equal(np.isnan(u), np.isnan(w)), name
        if np.isfinite(w).any():
            worst = max(worst, float(np.nanmax(np.abs(u - w) / bt.scale_of(np.abs(w)))))
    return worst


def _profile_path(family):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return os.path.join(root, "profiles", f"background_{PROFILE_OF.get(family, family)}.json")


def _d_key(family):
    return "d_" + PARITY_MODEL + ("_inflation_end" if family == "inflation_end" else "")


def parity_bound(family, solver):
    """1e-10 + 2 d, d as recorded in the family's profile"""
    import json

    with open(_profile_path(family)) as fh:
        return 1e-10 + 2.0 * json.load(fh)[_d_key(family)][solver]


def measure_parity_d():
    """{family: {solver: d}}: the host twin with FMA contraction against the twin without (the distribution twin has one build)"""
    d = {}
    for family in PARITY_FAMILIES:
        d[family] = {}
        for solver in ("rk4", "rkf"):
            off = parity_results(family, solver, "off")
            d[family][solver] = 0.0 if family == "distribution" else parity_difference(parity_results(family, solver, "fast"), off)
            finite = {n: int(np.isfinite(a).sum()) for n, a in off.items() if not np.issubdtype(np.asarray(a).dtype, np.integer)}
            print(f"{family} {solver}: d = {d[family][solver]:.3e}; finite values {finite}; status {np.unique(off.get('status', off.get('counts')))}", flush=True)
    return d


if __name__ == "__main__":
    import json

    path = _profile_path("special")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["d_j52_wall"] = measure_wall_d()
    doc["d_j52_wall_what"] = ("matched_difference of the WALL_RECOVERED lanes, the host twin built with -ffp-contract=fast -mfma against -ffp-contract=off: state (of each "
                              "value's scale, at matched accepted steps) and t (relative); unmatched: the rows as they are, whose t differ; tests assert 1e-10 + 2 x state")  # fmt: skip
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    for family, d in measure_parity_d().items():
        path = _profile_path(family)
        doc = json.load(open(path)) if os.path.exists(path) else {}
        doc[_d_key(family)] = d
        doc[_d_key(family) + "_what"] = ("worst difference, of each value's scale, between the host twin built with -ffp-contract=fast -mfma and with -ffp-contract=off on "
                                          "background_special.parity_results (8 lanes of bessel_skew, fixed dt); tests assert 1e-10 + 2 x this")  # fmt: skip
        with open(path, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")
