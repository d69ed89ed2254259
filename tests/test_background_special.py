"""Special-function models under the background solver, without a GPU: the conditions on the models of
``background_truth.special_model`` (domain, V >= 0.25, positive energy), the host twins of the kinematics, the masses and the
trajectories against 40-digit and DOP853 truths under the bars of the existing zoo, the noise header against sympy, and the status
premises of tests/test_background_special_gpu.py on the ``j52_wall`` lanes: a trial step that leaves a function's domain and is
retried leaves the status word set on a lane that ends COMPLETE inside the domain."""

if __name__ == "__main__":  # run as a script (the profile writer at the end): the repository root on the path, as under pytest
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import itertools
import math
import re
import types

import numpy as np
import pytest
import sympy as sp

import background_special as bs
import background_truth as bt
import kinematics_reference as kr
import masses_reference as mr
from background_reference import COMPLETE, NONFINITE, UNDERFLOW
from background_sampled_reference import SampledTwin
from background_target_reference import TARGET

MODELS = bt.SPECIAL_VALUE_MODELS
MAX_ERR = 1e-8  # solve_eom_sampled's default
RATIOS = {}  # worst ratio to each bar, per model and family: what `python tests/test_background_special.py` writes to profiles/


def test_set_sf_errors_is_public():
    from inflatox_amd import background

    assert "set_sf_errors" in background.__all__ and "set_sf_errors" in background.__doc__
    opened = []
    art = types.SimpleNamespace(_background_dylib=types.SimpleNamespace(set_sf_errors=opened.append))
    background.set_sf_errors(art, "nan")
    background.set_sf_errors(art, "raise")
    assert opened == ["nan", "raise"]  # the words reach the artefact's handle as they are
    with pytest.raises(ValueError, match='sf_errors must be "raise" or "nan"'):
        background.set_sf_errors(art, "NaN")
    assert opened == ["nan", "raise"]


@pytest.mark.parametrize("name", MODELS)
def test_the_box_is_inside_the_domain_with_margin(name):
    """Over a 13 x 13 grid of the box and the eight corners of the parameter ranges: V >= 0.25, the metric positive definite, and the
    generated equations of motion finite with the status word clear; the 257 lanes of the batch have their own parameter rows, all
    inside their ranges."""
    z, art = bt.zoo_model(name), bt.host_artifact(name)
    ranges = {par: (lo, hi) for par, lo, hi in z.par_ranges}
    slot_name = {int(s[5:-1]): n for n, s in art.symbol_dictionary.items() if s.startswith("args")}
    bounds = [ranges.get(slot_name[k], (0.5, 1.8)) for k in range(art.n_parameters)]
    init, pars = bt.batch(name)
    assert init.shape == (257, 4) and len({tuple(p) for p in pars}) == 257
    for k, (lo, hi) in enumerate(bounds):
        assert np.all((pars[:, k] >= lo) & (pars[:, k] <= hi))
    G = sp.Matrix(z.model.metric)
    fn = bt.point_function(z.model.coordinates, z.model.coordinate_tangents, [z.model.potential, G[0, 0], G.det()], art.symbol_dictionary, bt.float_modules(z))
    twin = bs.twin(name)
    twin.sf_status_take()
    x0, x1, y0, y1 = z.box
    pts = np.array([[a, b, 0.3, -0.3] for a in np.linspace(x0, x1, 13) for b in np.linspace(y0, y1, 13)])
    v_min = math.inf
    for corner in itertools.product(*bounds):
        vals = np.array([fn(*pt, corner) for pt in pts], dtype=np.float64)
        assert np.all(vals[:, 1] > 0) and np.all(vals[:, 2] > 0)
        v_min = min(v_min, float(vals[:, 0].min()))
        assert np.isfinite(twin.eom(np.array(corner), pts)).all()
    print(f"{name}: min V over the box and the parameter corners {v_min:.3f}")
    assert v_min >= bt.V_MIN
    assert twin.sf_status_take() == 0


@pytest.mark.parametrize("name", MODELS)
def test_kinematics_twin_against_truth(name):
    """The host build of the generated kinematics header at 65 states against the 40-digit truth, under ``kinematics_reference.allowance``."""
    states, pars = (a[: bs.STATES] for a in kr.zoo_states(name))
    got = kr.KinematicsTwin(bt.host_artifact(name)).kinematics(pars, states)
    worst = kr.worst_ratios(got, kr.zoo_truth(name, bs.STATES), states[:, 4])
    RATIOS[f"{name}/kinematics"] = worst
    print(f"{name}: kinematics twin, worst error / allowance {worst}")
    assert np.isfinite(got).all() and max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("name", MODELS)
def test_masses_twin_against_truth(name):
    """The host build of the generated masses header -- second derivatives: Bessel orders shifted by two, hypergeometric parameters
    by two -- at 65 states against the 40-digit truth, under ``masses_reference.allowance``."""
    states, pars = (a[: bs.STATES] for a in kr.zoo_states(name))
    got = mr.MassesTwin(bt.host_artifact(name)).masses(pars, states)
    worst = mr.worst_ratios(got, mr.zoo_truth(name, bs.STATES), states[:, 4])
    RATIOS[f"{name}/masses"] = worst
    print(f"{name}: masses twin, worst error / allowance {worst}")
    assert np.isfinite(got).all() and max(worst.values()) <= 1.0, worst


def test_a_flipped_sign_in_a_shifted_order_fails_the_masses_check():
    """The check above has teeth: with K_(nu - 2) turned into K_(nu + 2) in the generated masses header of ``bessel_skew`` -- one sign
    in one shifted order -- the same comparison fails."""
    name = "bessel_skew"
    art = bt.host_artifact(name)
    text = art.masses_header_text()
    broken, n = re.subn(r"= args\[2\] - 2;", "= args[2] + 2;", text)
    assert n == 1
    proxy = types.SimpleNamespace(_build=art._build, eom_header_text=art.eom_header_text, kinematics_header_text=art.kinematics_header_text, masses_header_text=lambda: broken)
    states, pars = (a[: bs.STATES] for a in kr.zoo_states(name))
    worst = mr.worst_ratios(mr.MassesTwin(proxy).masses(pars, states), mr.zoo_truth(name, bs.STATES), states[:, 4])
    assert max(worst.values()) > 1e3, worst


def test_noise_header_against_sympy():
    """``bessel_skew``: the generated inflx_noise_point on the host -- I_0 in the metric reaches the Cholesky factor, I_1 the
    contracted connection -- against sympy in 40 digits at 25 points of the box, as tests/test_background_stochastic.py does it:
    e e^T = G^-1 and Gamma^a = G^bc Gamma^a_bc to 1e-13 of the largest entry."""
    import mpmath

    import stochastic_reference as sr

    name = "bessel_skew"
    z, art = bt.zoo_model(name), bt.host_artifact(name)
    assert "inflx_sf_bessel_I0" in art.noise_header_text() and "inflx_sf_bessel_I1" in art.noise_header_text()
    p = bt.batch(name)[1][0]
    _e, gam, Gi = sr.noise_expressions(z.model)
    exprs = [sp.sympify(e) for e in (Gi[0, 0], Gi[0, 1], Gi[1, 1], *gam)]
    params, slots = sr._slots(z.model, art.symbol_dictionary, exprs)
    fn = sp.lambdify([*z.model.coordinates, *params], exprs, modules="mpmath")
    rng = np.random.default_rng(12)
    pts = np.stack([rng.uniform(z.box[0], z.box[1], 25), rng.uniform(z.box[2], z.box[3], 25)], axis=1)
    got = sr.StochasticTwin(art).noise_point(p, pts)
    worst = [0.0, 0.0]
    with mpmath.workdps(40):
        for (x0, x1), g in zip(pts, got):
            want = [float(v) for v in fn(mpmath.mpf(float(x0)), mpmath.mpf(float(x1)), *[mpmath.mpf(float(p[k])) for k in slots])]
            assert all(math.isfinite(v) for v in want) and want[0] > 0 and want[0] * want[2] - want[1] ** 2 > 0
            eet = [g[0] * g[0], g[0] * g[1], g[1] * g[1] + g[2] * g[2]]
            worst[0] = max(worst[0], max(abs(a - b) for a, b in zip(eet, want[:3])) / max(abs(v) for v in want[:3]))
            worst[1] = max(worst[1], max(abs(g[3] - want[3]), abs(g[4] - want[4])) / max(abs(want[3]), abs(want[4])))
            assert g[0] > 0.0 and g[2] > 0.0
    RATIOS[f"{name}/noise"] = dict(eet=worst[0] / 1e-13, gamma=worst[1] / 1e-13)
    print(f"{name}: worst relative error of e e^T {worst[0]:.2e}, of Gamma^a {worst[1]:.2e}")
    assert worst[0] <= 1e-13 and worst[1] <= 1e-13


@pytest.mark.parametrize("name", MODELS)
def test_every_lane_has_a_finite_truth_inside_the_domain(name):
    """The 16 lanes that are integrated: a finite truth up to T = 2 with H > 0.05, and -- the condition on the Runge-Kutta stages --
    the status word of the host build is clear after every fixed-dt and every adaptive run of both steppers."""
    init, pars = bt.batch(name)
    for tr in bt.truths(name, bs.LANES, bt.T_ADAPTIVE):
        assert tr.success and tr.t[-1] == bt.T_ADAPTIVE and np.all(np.isfinite(tr.y)) and tr.y[4].min() > 0.05
    twin = bs.twin(name)
    twin.sf_status_take()
    for method, kw in itertools.product(("rk4", "rkf"), (dict(dt=bt.T_ORDER / 20), dict(max_err=MAX_ERR))):
        for k in range(bs.LANES):
            out, meta = twin.solve(pars[k], init[k], 200 if "max_err" in kw else 41, method, **kw)
            assert meta["status"] == COMPLETE and np.isfinite(out).all()
    assert twin.sf_status_take() == 0


@pytest.mark.parametrize("method", ["rk4", "rkf"])
@pytest.mark.parametrize("name", MODELS)
def test_host_steppers_are_fourth_order(name, method):
    """tests/test_background_truth.py's bound on 16 lanes: fixed dt = 1/n to T = 1, halving dt cuts the end-point error against DOP853
    by >= 14 on every lane and the error at n = 40 is above 1e-10."""
    twin = bs.twin(name)
    init, pars = bt.batch(name)

    def solve(n):
        runs = [twin.solve(pars[k], init[k], n + 1, method, dt=bt.T_ORDER / n) for k in range(bs.LANES)]
        assert all(meta["status"] == COMPLETE for _, meta in runs)
        return np.array([out[-1] for out, _ in runs])

    e40, ratios = bt.order_ratios(solve, name, bs.LANES)
    RATIOS[f"{name}/order/{method}"] = dict(order=14.0 / float(ratios.min()), floor=1e-10 / float(e40.min()))
    print(f"{name} {method}: error at n = 40 {e40.min():.2e} .. {e40.max():.2e}, ratios {ratios.min():.2f} .. {ratios.max():.2f}")
    assert e40.min() > 1e-10 and ratios.min() >= 14.0, (e40.min(), ratios.min(), int(np.argmin(ratios)))


@pytest.mark.parametrize("at", ["t", "N"])
@pytest.mark.parametrize("method", ["rk4", "rkf"])
@pytest.mark.parametrize("name", MODELS)
def test_adaptive_host_runs_against_truth(name, method, at):
    """tests/test_background_truth.py's bound on 16 lanes: ``SampledTwin`` at max_err = 1e-8, four samples up to T = 2, every lane's
    error against DOP853 at most four times the worst error of the pure-Python restatement on the independent right-hand side."""
    art = bt.host_artifact(name)
    init, pars = bt.batch(name)
    truth = bt.truths(name, bs.LANES, bt.T_ADAPTIVE)
    samples = bt.samples_for(name, at, bs.LANES)
    twin = SampledTwin(art)
    ref, got = np.empty(bs.LANES), np.empty(bs.LANES)
    for k in range(bs.LANES):
        rows = bt.restatement_at_samples(name, k, samples, at, method, MAX_ERR, bt.T_ADAPTIVE)
        ref[k] = bt.error_against_truth(rows, truth[k]) / MAX_ERR
        out, meta = twin.solve(pars[k], init[k], samples, 100_000, method, max_err=MAX_ERR, at=at, stop_at_end=False)
        assert meta["status"] == TARGET and meta["n_stored"] == 4 and np.all(out[:, 6] <= bt.T_ADAPTIVE * (1 + 1e-12))
        got[k] = bt.error_against_truth(out, truth[k]) / MAX_ERR
    RATIOS[f"{name}/adaptive/{method}/{at}"] = dict(host_to_bar=float(got.max() / (4.0 * ref.max())))
    print(f"{name} {method} at {at}: error / max_err, restatement {ref.max():.2f}, host build {got.max():.2f}")
    assert ref.max() * MAX_ERR >= 100 * bt.TRUTH_TOL
    assert got.max() <= 4.0 * ref.max(), (got.max(), ref.max(), int(np.argmax(got)))


# ---- the status premises on j52_wall ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_recovered_excursions_leave_the_word_set_on_complete_lanes(method):
    """The premise of the GPU status test, as a condition on its inputs.  Every ``WALL_RECOVERED`` lane of the solver, on the twin
    without contraction AND with contract="fast": COMPLETE with all 120 rows stored, every stored phi > 0 and every value finite, and
    the build's status word equal to INFLX_SF_EDOM after the run (clear before it); the restatement on the independent right-hand
    side ends COMPLETE too and counts at least one trial step that was not finite.  At least two lanes per solver."""
    lanes = bs.WALL_RECOVERED[method]
    assert len(lanes) >= 2
    init, pars = bs.wall_lanes(lanes)
    eom = bt.truth_rhs("j52_wall")
    for k in range(len(lanes)):
        for contract in ("off", "fast"):
            twin = bs.twin("j52_wall", contract)
            twin.sf_status_take()  # (reading clears it)
            out, meta = twin.solve(pars[k], init[k], bs.WALL_ROWS, method, max_err=bs.WALL_MAX_ERR)
            assert meta["status"] == COMPLETE and meta["last_row"] == bs.WALL_ROWS - 1, (k, contract, meta)
            assert np.isfinite(out).all() and out[:, 0].min() > 0.0
            assert twin.sf_status_take() == bs.SF_EDOM and twin.sf_status_take() == 0
        with np.errstate(all="ignore"):
            ref = bs.CountingRestatement(eom, pars[k])
            rows, meta = ref.solve(list(init[k]), bs.WALL_ROWS, method, max_err=bs.WALL_MAX_ERR)
        print(f"{method} lane {k}: {ref.nonfinite_trials} non-finite trial steps recovered, min phi over the stored states {rows[:, 0].min():.2e}")
        assert meta["status"] == COMPLETE and ref.nonfinite_trials >= 1 and rows[:, 0].min() > 0.0


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_a_lane_that_leaves_the_domain(method):
    """``WALL_EXIT``: c = 1 does not turn the field round and it reaches phi = 0.  The fixed-step run ends NONFINITE in both host
    builds with the word set: a stage of the step that crosses is NaN, and a fixed step has no shorter one to retry.  The ADAPTIVE run
    of the same lane cannot end NONFINITE: every trial that crosses is retried at a fifth of the step, the accepted steps pile up in
    front of phi = 0 and the lane ends UNDERFLOW when the step no longer moves t -- with the word set and every stored phi > 0
    (tests/test_background_stops.py pins the same status for a wall made of phi^(3/2)).  So an adaptive
    lane that truly leaves the domain is not NONFINITE, and under "raise" it does not fail the call: its status says what happened."""
    c, state = bs.WALL_EXIT
    p, init = bs.wall_pars(c), np.array(state)
    for contract in ("off", "fast"):
        twin = bs.twin("j52_wall", contract)
        twin.sf_status_take()
        out, meta = twin.solve(p, init, bs.WALL_ROWS, method, dt=bs.WALL_EXIT_DT)
        assert meta["status"] == NONFINITE and 0 < meta["last_row"] < bs.WALL_ROWS - 1, meta
        assert np.isnan(out[meta["last_row"] + 1 :]).all() and out[: meta["last_row"] + 1, 0].min() > 0.0
        assert twin.sf_status_take() == bs.SF_EDOM
        out, meta = twin.solve(p, init, bs.WALL_ROWS, method, max_err=bs.WALL_MAX_ERR)
        assert meta["status"] == UNDERFLOW and 0 < meta["last_row"] < bs.WALL_ROWS - 1, meta
        assert np.isnan(out[meta["last_row"] + 1 :]).all() and 0.0 < out[: meta["last_row"] + 1, 0].min() < 1e-15
        assert twin.sf_status_take() == bs.SF_EDOM


def test_the_company_of_the_leaving_lane_stays_inside():
    """The seven in-domain lanes of the GPU's exit test: COMPLETE on both builds, fixed step and adaptive, phi >= 0.5, word clear."""
    init, pars = bs.wall_inside()
    for contract, kw in itertools.product(("off", "fast"), (dict(dt=bs.WALL_EXIT_DT), dict(max_err=bs.WALL_MAX_ERR))):
        twin = bs.twin("j52_wall", contract)
        twin.sf_status_take()
        for k in range(init.shape[0]):
            out, meta = twin.solve(pars[k], init[k], bs.WALL_ROWS, "rkf", **kw)
            assert meta["status"] == COMPLETE and out[:, 0].min() >= 0.5
        assert twin.sf_status_take() == 0


if __name__ == "__main__":
    # the worst ratio to each bar of the host builds, into profiles/background_special.json under "cpu"
    import json
    import os
    import sys

    rc = pytest.main([__file__, "-q", "-x", "-p", "no:cacheprovider"])
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "background_special.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["what"] = ("worst ratio of an error to its bar per model and family (1 = at the bar), tests/test_background_special.py on the host builds (cpu) and "
                   "tests/test_background_special_gpu.py on the device (gpu); each file writes its key when run as a script")  # fmt: skip
    doc["cpu"] = sys.modules["test_background_special"].RATIOS if "test_background_special" in sys.modules else RATIOS
    with open(path, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    sys.exit(rc)
