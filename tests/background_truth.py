"""An independent truth for the background solver on curved field spaces -- TEST INFRASTRUCTURE.

Everything else that checks the background solver starts from ``model.eom_fields``: the generated header, the host twin, the
restatement's model callable.  What is here does not.  ``euler_lagrange_eom`` derives the equations of motion from the Lagrangian
L = G_ab chi^a chi^b / 2 - V without the connection, the inverse metric or anything of inflatox_amd.symbolic;
``truth_trajectory`` integrates them with scipy's DOP853 at tolerances far below every bound that is asserted against it
(tests/test_background_truth.py validates it against 30-digit Taylor integration).  The model zoo is the fuzzed models of
tests/test_model_fuzz.py (diagonal metrics that depend on either field), two hand-written models with G_01 != 0 and the models of
``special_model``, which call Bessel and hypergeometric functions (``Compiler(link_gsl=True)``); ``batch`` gives each a seeded set
of initial states and per-lane parameter rows.
"""

from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np
import sympy as sp
from sympy.printing.c import C99CodePrinter

from test_model_fuzz import PARAMS, random_model, x, y

#: agreement of ``truth_trajectory`` with 30-digit integration that tests/test_background_truth.py asserts (absolute, every
#: component); every bound asserted against the truth is at least 100 times this
TRUTH_TOL = 1e-11
T_ORDER, T_ADAPTIVE = 1.0, 2.0
SAMPLES_T = np.array([0.35, 0.9, 1.45, 2.0])  # four sample points up to T = 2
GPU_FUZZ_SEEDS = (0, 1, 2, 3, 4, 5)


# ---- the derivation --------------------------------------------------------------------------------------------------------------
def euler_lagrange_eom(fields, metric, potential, tangents):
    """(eom^a, V, G_ab chi^a chi^b) with phi''^a = -eom^a - 3 H chi^a, from the Euler-Lagrange equations of
    a^3 (G_ab chi^a chi^b / 2 - V):  G_ab phi''^b = -[(d_c G_ab - d_a G_bc / 2) chi^b chi^c + d_a V] - 3 H G_ab chi^b,
    a linear system for phi'' that LU decomposition solves: no Christoffel symbol and no inverse metric is formed."""
    n = len(fields)
    G = sp.Matrix(n, n, lambda a, b: sp.sympify(metric[a][b]))
    V = sp.sympify(potential)
    chi = list(tangents)
    force = []
    for a in range(n):
        acc = sp.diff(V, fields[a])
        for b in range(n):
            for c in range(n):
                acc += (sp.diff(G[a, b], fields[c]) - sp.diff(G[b, c], fields[a]) / 2) * chi[b] * chi[c]
        force.append(-acc)
    accel = G.LUsolve(sp.Matrix(force))
    kin = sum(G[a, b] * chi[a] * chi[b] for a in range(n) for b in range(n))
    return [-accel[a] for a in range(n)], V, kin


def point_function(fields, tangents, exprs, param_slots=None, modules="math"):
    """f(x0, x1, xd0, xd1, p) -> tuple of the values of ``exprs``.  ``param_slots`` maps a parameter's printed name to its
    ``args[k]`` slot (``CompilationArtifact.symbol_dictionary``): p is the artefact's parameter row.  Without it the parameters
    are taken in the order of their names."""
    exprs = [sp.sympify(e) for e in exprs]
    plain = C99CodePrinter()._print_Symbol
    free = set().union(*[e.free_symbols for e in exprs]) - set(fields) - set(tangents)
    if param_slots is None:
        names = sorted(plain(s) for s in free)
        slot = {s: names.index(plain(s)) for s in free}
    else:
        slot = {s: int(param_slots[plain(s)][5:-1]) for s in free}
    params = sorted(free, key=slot.get)
    slots = [slot[s] for s in params]
    fn = sp.lambdify([*fields, *tangents, *params], exprs, modules=modules, cse=True)

    def f(a, b, c, d, p):
        return tuple(fn(a, b, c, d, *[p[k] for k in slots]))

    return f


def truth_functions(model, param_slots=None, modules="math"):
    """``point_function`` of the Euler-Lagrange derivation for ``model``: (eom^0, eom^1, V, G_ab chi^a chi^b)."""
    eom, V, kin = _derivation(model)
    return point_function(model.coordinates, model.coordinate_tangents, [*eom, V, kin], param_slots, modules)


@functools.lru_cache(maxsize=None)
def _derivation(model):
    return euler_lagrange_eom(model.coordinates, model.metric, model.potential, model.coordinate_tangents)


def model_eom_functions(model, param_slots=None, modules="math"):
    """``point_function`` of the project's own expressions, ``model.eom_fields``: (eom^0, eom^1)."""
    return point_function(model.coordinates, model.coordinate_tangents, list(model.eom_fields), param_slots, modules)


# ---- the integration -------------------------------------------------------------------------------------------------------------
def initial_y(rhs, init):
    """(phi^0, phi^1, chi^0, chi^1, H0, 0) with H0 from the Friedmann constraint."""
    _, _, V, kin = rhs(*init)
    return [float(init[0]), float(init[1]), float(init[2]), float(init[3]), math.sqrt((V + 0.5 * kin) / 3.0), 0.0]


def truth_trajectory(rhs, init, t_end):
    """scipy's DOP853 with dense output on y = (phi, chi, H, N) at rtol = 1e-13, atol = 1e-15; ``rhs(x0, x1, xd0, xd1)`` is the
    independent model function with its parameters bound.  Returns the OdeResult: ``.sol(t)`` is (6,) or (6, len(t))."""
    from scipy.integrate import solve_ivp

    def f(_t, s):
        a, b, V, _k = rhs(s[0], s[1], s[2], s[3])
        return [s[2], s[3], -a - 3.0 * s[4] * s[2], -b - 3.0 * s[4] * s[3], V - 3.0 * s[4] * s[4], s[4]]

    return solve_ivp(f, (0.0, t_end), initial_y(rhs, init), method="DOP853", rtol=1e-13, atol=1e-15, dense_output=True)


def taylor_trajectory(rhs_mp, init, times, dps=30):
    """The same system by mpmath's Taylor-series integrator at ``dps`` digits: (len(times), 6) of mpf."""
    import mpmath

    with mpmath.workdps(dps):
        s0 = [mpmath.mpf(float(v)) for v in init]
        _, _, V, kin = rhs_mp(*s0)
        y0 = [*s0, mpmath.sqrt((V + kin / 2) / 3), mpmath.mpf(0)]

        def f(_t, s):
            a, b, V, _k = rhs_mp(s[0], s[1], s[2], s[3])
            return [s[2], s[3], -a - 3 * s[4] * s[2], -b - 3 * s[4] * s[3], V - 3 * s[4] * s[4], s[4]]

        sol = mpmath.odefun(f, 0, y0)
        return [[+v for v in sol(t)] for t in times]


# ---- the model zoo ---------------------------------------------------------------------------------------------------------------
class ZooModel(NamedTuple):
    name: str
    model: object
    cse: bool
    box: tuple  # (x0 min, x0 max, x1 min, x1 max): the model's extent
    gsl: bool = False  # the model calls special functions: Compiler(link_gsl=True), truths through scipy / mpmath
    par_ranges: tuple = ()  # ((printed name, min, max), ...) of the parameters that are not drawn from [0.5, 1.8]


def _build(name, G, V):
    from inflatox_amd import InflationModelBuilder

    return InflationModelBuilder.new([x, y], G, V, model_name=name, silent=True, init_sympy_printing=False, simplify=False, assertions=False).build()


@functools.lru_cache(maxsize=None)
def nondiagonal_model(name):
    """Two smooth models with G_01 != 0, positive definite on their boxes for every parameter in [0.5, 1.8]:
    ``skew``  det G >= e^(-0.4) + b - a^2 / 9 > 0.8;   ``shear`` (cse=True)  G_00 >= 1.5, G_11 >= 1, |G_01| <= 0.45."""
    a, b, c = PARAMS
    if name == "skew":
        off = a * sp.sin(x) / 3
        G = [[1 + y**2, off], [off, sp.exp(x / 3) + b]]
        V = a * (2 + x**2 / 2 + y**2 / 3) + b * sp.cos(x * y / 2) / 2
        return ZooModel(name, _build(name, G, V), False, (0.3, 2.0, -1.0, 1.5))
    if name == "shear":
        off = c * sp.sin(x + y) / 4
        G = [[sp.cosh(y / 2) ** 2 + a, off], [off, 2 + sp.cos(x) + b * y**2]]
        V = a * sp.exp(-x / 3) * sp.sqrt(1 + c * y**2) + b * sp.log(2 + x**2) + c * (x**2 + y**2) / 7
        return ZooModel(name, _build(name, G, V), True, (0.2, 2.2, -1.2, 1.4))
    raise KeyError(name)


NONDIAGONAL = ("skew", "shear")

NU = sp.Symbol("nu")


@functools.lru_cache(maxsize=None)
def special_model(name):
    """Models that call the special functions of csrc/inflx_sf.h.  The equations of motion, the kinematics and the noise take first
    derivatives, which shift a Bessel order by one and both hypergeometric parameters by one; the masses take second ones.

    ``bessel_skew``: ``skew`` with I_0 in the metric -- it reaches the connection, the Ricci scalar and the noise's Cholesky factor --
    and J_0 and K_nu in the potential; nu in [2, 3.5], so that every shifted order nu - 2 .. nu + 2 stays >= 0, and the arguments
    x, x / 2 and x + 1 are positive on the box.  det G >= I_0(0.15) + b - a^2 / 9 > 1.1; V >= a (3 + J_0(2)) > 1.6.
    ``kummer_curved``: a curved diagonal metric and a potential with 1F1(a; c; -x / 2) and 2F1(a, 1/2; c; y / 3), a and c the model's
    parameters: c > 0 is never a non-positive integer, however often it is shifted up, and y / 3 stays in (-1/3, 1/2), inside
    2F1's -1 <= z < 1.  tests/test_background_special.py establishes V >= 0.25 over the box and the domain along the truth runs.
    ``j52_wall``: V = b + a J_5/2(phi) - c phi on a flat field space, J_nu defined for phi >= 0 only: a field that rolls towards
    phi = 0 under the slope -c meets the domain's edge.  For the status tests alone (``wall_lanes``); it has no box to draw from."""
    a, b, c = PARAMS
    if name == "bessel_skew":
        off = a * sp.sin(x) / 3
        G = [[1 + y**2, off], [off, sp.besseli(0, x / 2) + b]]
        V = a * (3 + sp.besselj(0, x) + y**2 / 3) + b * sp.besselk(NU, x + 1) / 2
        return ZooModel(name, _build(name, G, V), False, (0.3, 2.0, -1.0, 1.5), True, (("nu", 2.0, 3.5),))
    if name == "kummer_curved":
        G = [[sp.cosh(y / 2) ** 2, 0], [0, 1 + b * x**2 / 4]]
        V = b * (4 + sp.hyper((a,), (c,), -x / 2) + y**2 / 3) + sp.hyper((a, sp.Rational(1, 2)), (c,), y / 3) / 2
        return ZooModel(name, _build(name, G, V), False, (0.3, 2.0, -1.0, 1.5), True)
    if name == "j52_wall":
        V = b + a * sp.besselj(sp.Rational(5, 2), x) - c * x
        return ZooModel(name, _build(name, [[1, 0], [0, 1]], V), False, (0.0, 1.0, -1.0, 1.0), True)
    raise KeyError(name)


SPECIAL_VALUE_MODELS = ("bessel_skew", "kummer_curved")


def _hyper_scipy(ap, bq, z):
    """sympy's ``hyper`` for scipy: 1F1 and 2F1, the two that the special models use"""
    from scipy import special

    if (len(ap), len(bq)) == (1, 1):
        return special.hyp1f1(ap[0], bq[0], z)
    if (len(ap), len(bq)) == (2, 1):
        return special.hyp2f1(ap[0], ap[1], bq[0], z)
    raise NotImplementedError((ap, bq))


def float_modules(z):
    """``modules`` of a float64 ``point_function`` of a zoo model: the math module, or scipy for the special functions"""
    return [{"hyper": _hyper_scipy}, "scipy", "numpy"] if z.gsl else "math"


@functools.lru_cache(maxsize=None)
def zoo_model(name):
    """``"fuzz<seed>"``: ``random_model(seed)`` of tests/test_model_fuzz.py; ``"skew"`` / ``"shear"``: the non-diagonal models;
    ``"bessel_skew"`` / ``"kummer_curved"`` / ``"j52_wall"``: the models with special functions."""
    if name.startswith("fuzz"):
        model, _args, ext, cse = random_model(int(name[4:]))
        return ZooModel(name, model, cse, tuple(ext))
    if name in NONDIAGONAL:
        return nondiagonal_model(name)
    return special_model(name)


GPU_MODELS = tuple(f"fuzz{s}" for s in GPU_FUZZ_SEEDS) + NONDIAGONAL


@functools.lru_cache(maxsize=None)
def host_artifact(name):
    """The artefact of a zoo model as far as the host twins need it -- the generated core header, the parameter numbering and the
    recipe of the equations-of-motion header -- without a hipcc step."""
    from inflatox_amd import Compiler
    from inflatox_amd.compiler import CompilationArtifact

    z = zoo_model(name)
    comp = Compiler(z.model, silent=True, cse=z.cse, link_gsl=z.gsl)
    header = comp._generate_hip_header()
    art = CompilationArtifact(comp.symbol_dict, f"/nonexistent/{name}.hsaco", 2, len(comp.symbol_dict) - 2, auto_cleanup=False)
    art._build = (header, [], "")
    art._eom_recipe = (z.model, dict(comp._param_slots), comp.cse, comp.max_cses)
    return art


@functools.lru_cache(maxsize=None)
def device_artifact(name):
    from inflatox_amd import Compiler

    z = zoo_model(name)
    return Compiler(z.model, silent=True, cse=z.cse, link_gsl=z.gsl).compile()


V_MIN, VELOCITY, B_MAX = 0.25, 0.3, 257
# Which seeded draw is a model's batch: the first for which, on the HOST build and against the truth, the first 65 lanes keep
# H > 0.05 up to T = 2 (from other draws of fuzz1 and fuzz3 a lane rolls to where V < 0 and recollapses: N falls again and an e-fold
# sample is never reached), every lane's fixed-dt error at n = 40 is above 1.2e-10 and every lane's convergence ratio n = 20 -> 40
# is at least 14.5, rk4 and rkf (at n = 20 the fifth-order term of a few lanes of fuzz2 and fuzz4 is not yet small: ratios of 12 to
# 13.7 in most of their draws).  tests/test_background_truth.py asserts all three for the draws chosen; the GPU runs the same lanes.
BATCH_DRAW = {"fuzz1": 2, "fuzz2": 11, "fuzz3": 27, "fuzz4": 10}


def batch(name):
    return _batch(name, BATCH_DRAW.get(name, 0))


@functools.lru_cache(maxsize=None)
def _batch(name, draw):
    """(init (257, 4), pars (257, n_par)) of a zoo model: seeded draws of a state inside the model's extent with velocities in
    [-0.3, 0.3] and of a parameter row in [0.5, 1.8] (the range the fuzzed models are built for), every lane its own; of the draws,
    those at which the potential is at least 0.25 are taken, in order, so that the energy 3 H0^2 = V + G chi chi / 2 is positive
    and no lane starts on its way to H = 0.  Tests with fewer lanes take the first of these."""
    z = zoo_model(name)
    art = host_artifact(name)
    rng = np.random.default_rng(77_000 + 1000 * draw + sum(map(ord, name)))
    n = 16 * B_MAX
    x0, x1, y0, y1 = z.box
    init = np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n), rng.uniform(-VELOCITY, VELOCITY, n), rng.uniform(-VELOCITY, VELOCITY, n)], axis=1)
    pars = rng.uniform(0.5, 1.8, (n, art.n_parameters))
    for par, lo, hi in z.par_ranges:  # the same draw, carried to the parameter's own range
        k = int(art.symbol_dictionary[par][5:-1])
        pars[:, k] = lo + (pars[:, k] - 0.5) / 1.3 * (hi - lo)
    potential = point_function(z.model.coordinates, z.model.coordinate_tangents, [z.model.potential], art.symbol_dictionary, float_modules(z))
    keep = [k for k in range(n) if potential(*init[k], pars[k])[0] >= V_MIN][:B_MAX]
    assert len(keep) == B_MAX, (name, len(keep))
    init, pars = np.ascontiguousarray(init[keep]), np.ascontiguousarray(pars[keep])
    init.setflags(write=False)
    pars.setflags(write=False)
    return init, pars


@functools.lru_cache(maxsize=None)
def truth_rhs(name):
    """eom(x0, x1, xd0, xd1, p) of the Euler-Lagrange derivation in float64, parameters in the artefact's slots."""
    z = zoo_model(name)
    return truth_functions(z.model, host_artifact(name).symbol_dictionary, float_modules(z))


def bound(eom, p):
    return lambda a, b, c, d: eom(a, b, c, d, p)


@functools.lru_cache(maxsize=None)
def truths(name, n_lanes, t_end):
    """``truth_trajectory`` of the first ``n_lanes`` lanes of ``batch(name)``: computed once and shared."""
    init, pars = batch(name)
    eom = truth_rhs(name)
    return tuple(truth_trajectory(bound(eom, pars[k]), init[k], t_end) for k in range(n_lanes))


def scale_of(want):
    """a value's scale in comparisons against the restatement: its magnitude with a floor of 1e-3 (tests/test_background_gpu.py)"""
    return np.maximum(np.abs(want), 1e-3)


# ---- the restatement at sample points --------------------------------------------------------------------------------------------
def _hermite(y0, f0, y1, f1, h, th):
    """the dense output of csrc/inflx_background.h: the cubic through (y0, h f0) at theta = 0 and (y1, h f1) at theta = 1"""
    h00 = (1.0 + 2.0 * th) * (1.0 - th) ** 2
    h10 = th * (1.0 - th) ** 2
    h01 = th * th * (3.0 - 2.0 * th)
    h11 = th * th * (th - 1.0)
    return h00 * y0 + h10 * h * f0 + h01 * y1 + h11 * h * f1


@functools.lru_cache(maxsize=None)
def _restatement_run(name, lane, method, max_err, t_end):
    """The adaptive ``Restatement`` of one lane of ``batch(name)`` on the independent right-hand side, up to the first row at or
    past ``t_end`` (past it a lane's H may turn negative): (the restatement, its rows)."""
    from background_reference import COMPLETE, Restatement

    init, pars = batch(name)
    ref = Restatement(truth_rhs(name), pars[lane])
    rows = 128
    while True:
        out, meta = ref.solve(init[lane], rows, method, max_err=max_err)
        assert meta["status"] == COMPLETE
        if out[-1, 6] >= t_end:
            return ref, out[: int(np.argmax(out[:, 6] >= t_end)) + 1]
        rows *= 2


def restatement_at_samples(name, lane, samples, at, method, max_err, t_end):
    """The pure-Python ``Restatement`` (adaptive, on the independent right-hand side) read at ``samples`` the way
    ``solve_eom_sampled`` documents it: inside the accepted step that passes a sample, the cubic Hermite interpolant of the states
    and right-hand sides at the step's ends; for ``at="t"`` theta = (t_s - t0) / h, for ``at="N"`` the theta at which the
    interpolant of N is the sample (bisection).  Returns (S, 7): y[0..5] and t.  ``t_end`` bounds the times the samples are reached
    at."""
    ref, out = _restatement_run(name, lane, method, max_err, t_end)
    col = 6 if at == "t" else 5
    got = np.empty((len(samples), 7))
    for s, target in enumerate(samples):
        r = int(np.searchsorted(out[:, col], target, side="left"))  # the first row at or past the sample
        assert 1 <= r < out.shape[0], (target, r)
        y0, y1, h = out[r - 1, :6], out[r, :6], out[r, 6] - out[r - 1, 6]
        f0, f1 = ref.rhs(list(y0))[0], ref.rhs(list(y1))[0]
        if at == "t":
            th = (target - out[r - 1, 6]) / h
        else:
            lo, hi = 0.0, 1.0
            for _ in range(60):
                th = 0.5 * (lo + hi)
                if _hermite(y0[5], f0[5], y1[5], f1[5], h, th) < target:
                    lo = th
                else:
                    hi = th
            th = 0.5 * (lo + hi)
        got[s, :6] = [_hermite(y0[c], f0[c], y1[c], f1[c], h, th) for c in range(6)]
        got[s, 6] = out[r - 1, 6] + th * h
    return got


def samples_for(name, at, n_lanes=65):
    """Four sample points up to T = 2 shared by the lanes: times, or e-fold counts that the slowest lane's truth reaches by T."""
    if at == "t":
        return SAMPLES_T
    n_min = min(float(tr.sol(T_ADAPTIVE)[5]) for tr in truths(name, n_lanes, T_ADAPTIVE))
    return n_min * np.array([0.25, 0.5, 0.75, 0.97])


def error_against_truth(rows, truth):
    """max over the samples and the six components of |y - truth(t)| at the rows' own t; ``rows`` (S, >= 7): y[0..5], t"""
    return float(np.max(np.abs(rows[:, :6] - truth.sol(rows[:, 6]).T)))


def order_ratios(solve, name, n_lanes=65):
    """(errors at n = 40, ratios of the errors at n = 20 to those at n = 40) of the end point at T = 1 against the truth, per lane;
    ``solve(n)`` returns (n_lanes, 7): every lane's y[0..5] and t after n steps of T / n."""
    truth = truths(name, n_lanes, T_ADAPTIVE)
    errs = np.empty((2, n_lanes))
    for i, n in enumerate((20, 40)):
        end = solve(n)
        for k in range(n_lanes):
            errs[i, k] = np.max(np.abs(end[k, :6] - truth[k].sol(end[k, 6])))
    return errs[1], errs[0] / errs[1]
