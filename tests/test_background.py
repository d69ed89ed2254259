"""Background trajectories without a GPU: the generated equations of motion, the numpy restatement of the integrator against
analytic and scipy solutions, the host build of csrc/inflx_background.h against the restatement, argument checks and the public
surface (inflatox_amd.background)."""

import inspect
import math

import numpy as np
import pytest
import sympy

import workloads
from background_truth import truth_functions
from background_reference import (
    COMPLETE,
    ENDED,
    BackgroundTwin,
    Restatement,
    model_functions,
    power_law_artifact,
    power_law_exact,
    power_law_init,
    power_law_model,
    solve_ivp_reference,
)

MODELS = ("hyperbolic", "doc", "angular", "egno", "d5")
# Points and velocities per model: inside the sweep extent of the model, away from its coordinate singularities
BOXES = {
    "hyperbolic": ((0.2, 3.0), (-1.0, 1.0)),
    "doc": ((1.5, 3.0), (0.6, 1.0)),
    "angular": ((0.3, 1.5), (-1.0, 1.0)),
    "egno": ((0.6, 0.9), (0.2, 0.5)),
    "d5": ((1.0, 3.0), (0.3, 1.2)),
}


# velocity scale of the trajectories' initial conditions: V + G_ab xd^a xd^b / 2 > 0 (EGNO's V is negative in its box)
VELOCITY = {"hyperbolic": 0.2, "doc": 0.2, "angular": 0.2, "egno": 1.0, "d5": 0.2}


def initial_state(name, seed=3):
    return _points(name, 1, seed=seed)[0] * np.array([1, 1, VELOCITY[name], VELOCITY[name]])


def _points(name, n, seed=0):
    rng = np.random.default_rng(seed)
    (a0, b0), (a1, b1) = BOXES[name]
    return np.stack([rng.uniform(a0, b0, n), rng.uniform(a1, b1, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-0.5, 0.5, n)], axis=1)


@pytest.mark.parametrize("name", MODELS)
def test_generated_eom_matches_sympy(name):
    """inflx_eom_point (compiled for the host) against sympy at 200 seeded points: eom^a, V and G_ab xd^a xd^b of an Euler-Lagrange
    derivation that shares nothing with ``model.eom_fields`` (background_truth.euler_lagrange_eom), evaluated by lambdify in 40-digit
    arithmetic, are the truth; the generated code must be within four times the error of lambdify's own float64
    evaluation of the same expressions, or 1e-12 of the value's scale.  The two float64 programs round differently (shared nodes,
    pow chains of up to x^12 with up to 11 half-ulps), and EGNO's eom^a cancel to ~1e-7 at some points in both (its expressions
    are sums of ~100 rational terms): what is asserted is that the staged code is as accurate as the expression allows."""
    import mpmath

    spec, art = workloads.artifact_for(name)
    twin = BackgroundTwin(art)
    model = workloads.model_for(name)
    exact_fn = truth_functions(model, art.symbol_dictionary, modules="mpmath")
    float_fn = model_functions(model, art.symbol_dictionary)
    pts = _points(name, 200)
    got = twin.eom(spec.args, pts)
    with mpmath.workdps(40):
        mp_args = [mpmath.mpf(float(v)) for v in spec.args]
        exact = np.array([[float(v) for v in exact_fn(*[mpmath.mpf(float(v)) for v in pt], mp_args)] for pt in pts])
    plain = np.array([float_fn(*pt, spec.args) for pt in pts])
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(exact))
    scale = np.maximum(np.abs(exact), np.max(np.abs(exact), axis=0) * 1e-3)
    err_got = (np.abs(got - exact) / scale).max(axis=0)
    err_plain = (np.abs(plain - exact) / scale).max(axis=0)
    assert np.all(err_got <= np.maximum(4 * err_plain, 1e-12)), (name, err_got, err_plain)


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_restatement_on_the_power_law_attractor(method):
    model = power_law_model()
    art, p = power_law_artifact()
    eom = model_functions(model, art.symbol_dictionary)
    out, meta = Restatement(eom, p).solve(power_law_init(), 200, method, max_err=1e-10)
    assert meta["status"] == COMPLETE and meta["accepted"] == 199
    exact = power_law_exact(out[:, 6])
    rel = np.abs(out[:, :6] - exact) / np.maximum(np.abs(exact), 1.0)
    assert rel.max() <= 1e-8, rel.max(axis=0)
    assert out[-1, 6] > 1e-3


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_restatement_against_solve_ivp(method):
    spec, art = workloads.artifact_for("hyperbolic")
    eom = model_functions(workloads.model_for("hyperbolic"), art.symbol_dictionary)
    init = np.array([3.0, 0.5, 0.0, 0.1])
    out, meta = Restatement(eom, spec.args).solve(init, 300, method, max_err=1e-10)
    assert meta["status"] == COMPLETE
    sol = solve_ivp_reference(eom, spec.args, init, out[-1, 6])
    want = sol.sol(out[:, 6]).T
    assert np.max(np.abs(out[:, :6] - want)) <= 1e-7


@pytest.mark.parametrize("name", ["hyperbolic", "doc", "angular", "egno", "d5"])
@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_host_integrator_matches_restatement(name, method):
    """csrc/inflx_background.h built for the host: a fixed dt agrees with the restatement to 1e-13 relative; adaptive runs take the
    same accepted steps.  Both integrate the same model -- the generated inflx_eom_point, through the twin -- so that what is compared
    is the integrator alone (test_generated_eom_matches_sympy checks the model function against sympy)."""
    spec, art = workloads.artifact_for(name)
    twin = BackgroundTwin(art)

    def eom(a, b, c, d, p):
        return tuple(twin.eom(p, np.array([[a, b, c, d]]))[0])

    init = initial_state(name)
    ref = Restatement(eom, spec.args)
    got, gm = twin.solve(spec.args, init, 60, method, dt=1e-3)
    want, wm = ref.solve(init, 60, method, dt=1e-3)
    assert gm["status"] == wm["status"] == COMPLETE
    scale = np.maximum(np.abs(want), 1e-3)
    assert np.max(np.abs(got - want) / scale) <= 1e-13
    got, gm = twin.solve(spec.args, init, 40, method, max_err=1e-9)
    want, wm = ref.solve(init, 40, method, max_err=1e-9)
    assert gm["accepted"] == wm["accepted"] and gm["status"] == wm["status"]
    # (the step sizes go through pow(max_err/err, 1/5): libm's and Python's may differ in the last bit, and dt carries that forward)
    assert np.max(np.abs(got[:, 6] - want[:, 6]) / np.maximum(want[:, 6], 1e-300)) <= 1e-6


def test_host_integrator_end_of_inflation():
    spec, art = workloads.artifact_for("hyperbolic")
    twin = BackgroundTwin(art)
    eom = model_functions(workloads.model_for("hyperbolic"), art.symbol_dictionary)
    init = np.array([3.0, 0.5, 0.0, 0.1])
    got, gm = twin.solve(spec.args, init, 2000, "rkf", max_err=1e-10, stop_at_end=True)
    want, wm = Restatement(eom, spec.args).solve(init, 2000, "rkf", max_err=1e-10, stop_at_end=True)
    assert gm["status"] == wm["status"] == ENDED and gm["last_row"] == wm["last_row"]
    assert np.all(np.isnan(got[gm["last_row"] + 1 :]))
    assert abs(gm["N_end"] - wm["N_end"]) <= 1e-9 * wm["N_end"]


# ---- argument validation: nothing reaches the device -------------------------------------------------------------------------
def _art():
    return workloads.artifact_for("hyperbolic")


def test_bad_arguments_raise_before_the_device(monkeypatch):
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    spec, art = _art()
    p = spec.args
    x, v = [1.0, 0.0], [0.0, 0.0]
    with pytest.raises(_native.InflatoxShapeError):
        background.solve_eom(art, p[:2], 10, x, v)
    with pytest.raises(_native.InflatoxShapeError):
        background.solve_eom_batch(art, p, 10, np.zeros((3, 2)), np.zeros((2, 2)))
    with pytest.raises(_native.InflatoxShapeError):
        background.solve_eom_batch(art, np.zeros((2, 3)), 10, np.zeros((3, 2)), np.zeros((3, 2)))
    with pytest.raises(_native.InflatoxShapeError):
        background.solve_eom_batch(art, p, 10, np.zeros((3, 3)), np.zeros((3, 3)))
    for steps in (0, -1):
        with pytest.raises(ValueError):
            background.solve_eom(art, p, steps, x, v)
    for err in (0.0, -1e-6, float("nan")):
        with pytest.raises(ValueError):
            background.solve_eom(art, p, 10, x, v, max_err=err)
    with pytest.raises(ValueError):
        background.solve_eom(art, p, 10, x, v, solver="euler")
    with pytest.raises(ValueError):
        background.solve_eom(art, p, 10, x, v, dt=0.0)
    with pytest.raises(ValueError):
        background.solve_eom_batch(art, p, 10, [x], [v], substeps=0)
    with pytest.raises(_native.InflatoxShapeError):
        background.efolds_map(art, p, [0, 1, 0], 4, 4)
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    with pytest.raises(_native.InflatoxShapeError):
        background.solve_eom(three, p, 10, [1.0, 0.0, 0.0], [0.0, 0.0, 0.0])
    with pytest.raises(_native.InflatoxShapeError):
        background.efolds_map(three, p, [[0, 1], [0, 1]], 4, 4)


# ---- public surface -------------------------------------------------------------------------------------------------------------
def test_background_is_exported():
    import inflatox_amd

    assert "background" in inflatox_amd.__all__
    assert inflatox_amd.background.solve_eom is not None


def test_solve_eom_signature_is_the_references():
    from inflatox_amd.background import solve_eom

    params = list(inspect.signature(solve_eom).parameters.values())
    positional = [(q.name, q.default) for q in params if q.kind == q.POSITIONAL_OR_KEYWORD]
    E = inspect.Parameter.empty
    assert positional == [("artifact", E), ("pars", E), ("steps", E), ("fields_init", E), ("derivatives_init", E), ("max_err", 1e-6), ("solver", "rk4")]
    assert [(q.name, q.default) for q in params if q.kind == q.KEYWORD_ONLY] == [("dt", None)]


# core content tags of the example models: the sweep objects, profiles/ stamps and bench.py figures are untouched only if these
# stay as they are.  Last moved on purpose by the change of csrc/inflx_device_math.h that gives the half powers pow's results at
# -0.0 and -inf and the hoisted / shared quotients an upper end of their acceptance test (the tag covers the csrc headers); the
# values the sweeps store did not change: bench.py --dump-outputs at both commits, bit for bit, all five models
# (profiles/hpow_edge_fix_outputs.txt).  The records in profiles/ that are stamped with the former tags no longer match.
PARENT_TAGS = {
    "hyperbolic": "25b693eda26925832dba",
    "doc": "7527d626a66e2d73d15d",
    "angular": "68e866bfaefd5c101062",
    "egno": "a8ac75aff800c9874695",
    "d5": "5c1570102f32c29a8c69",
}


@pytest.mark.parametrize("name", MODELS)
def test_core_tags_unchanged(name):
    _, art = workloads.artifact_for(name)
    assert art._build[2] == PARENT_TAGS[name]


def test_groups_unchanged():
    from inflatox_amd.compiler import ALL_GROUPS, KERNEL_GROUPS

    assert ALL_GROUPS == 511 and sum(KERNEL_GROUPS.values()) == 511 and "background" not in KERNEL_GROUPS


def test_eom_header_stays_out_of_the_core_header():
    _, art = workloads.artifact_for("hyperbolic")
    assert "inflx_eom_point" not in art._build[0]
    assert "INFLX_FN void inflx_eom_point(" in art.eom_header_text()
