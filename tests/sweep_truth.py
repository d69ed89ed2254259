"""An independent 50-digit truth for the sweep (V, v00, v10, v11, |dV|^2 and everything derived) -- TEST INFRASTRUCTURE.

Every other check of the sweep's model values starts from ``inflatox_amd/symbolic.py``: the goldens pin five models to the
reference's symbolic stage, and ``oracle.emit_c_source(model)`` prints the expressions that stage derived.  What is here does not.
``truth_expressions`` writes the covariant Hesse matrix of V as a Lie derivative of the metric along the raised gradient,

    H_ab = (L_X G)_ab / 2 = (X^c d_c G_ab + G_cb d_a X^c + G_ac d_b X^c) / 2,        G X = dV  (LU decomposition),

which forms no Christoffel symbol and no inverse metric and imports nothing from the symbolic stage (tests/test_sweep_truth.py
checks it against d d V - Gamma dV with textbook connections, and against the reference's own derivation as stored with the goldens).
``raw_truth`` evaluates it with mpmath at ``dps`` digits and projects it on the basis (v, w) by the reference's rule -- v = X / sqrt(g),
w the normalised raise of the covector (-v^1, v^0), or the Gram-Schmidt step of a guess -- with the FULL metric in every inner product.
``mp_epilogue`` / ``mp_single_quantities`` restate tests/tolerance.py's ``epilogue`` / ``single_quantities`` in mpmath, in the same
operation order.  The models are the two of tests/background_truth.py with G_01 != 0 and their guess-built variants.
"""

from __future__ import annotations

import functools
from typing import NamedTuple

import mpmath as mp
import numpy as np
import sympy as sp
from sympy.printing.c import C99CodePrinter

import background_truth as bt

DPS = 50
BAR = 1e-10  # the project's parity bar, relative to ``scale``
GRID_CPU = (23, 19)
GRID_GPU = (33, 257)  # one full and one ragged row tile (32 + 1), one full and one ragged column tile (256 + 1)
NAN = mp.nan


# ---- the derivation --------------------------------------------------------------------------------------------------------------
def truth_expressions(fields, metric, potential):
    """{"V", "g", "X": [X^0, X^1], "G": [[..]], "H": [[..]]} as sympy expressions: X solves G X = dV by LU decomposition,
    g = dV . X = |dV|^2, H_ab = (X^c d_c G_ab + G_cb d_a X^c + G_ac d_b X^c) / 2."""
    f = list(fields)
    n = len(f)
    G = sp.Matrix(n, n, lambda a, b: sp.sympify(metric[a][b]))
    V = sp.sympify(potential)
    dV = sp.Matrix([sp.diff(V, q) for q in f])
    X = G.LUsolve(dV)
    g = sum(dV[a] * X[a] for a in range(n))
    H = [[sum(X[c] * sp.diff(G[a, b], f[c]) + G[c, b] * sp.diff(X[c], f[a]) + G[a, c] * sp.diff(X[c], f[b]) for c in range(n)) / 2 for b in range(n)] for a in range(n)]
    return {"V": V, "g": g, "X": [X[a] for a in range(n)], "G": [[G[a, b] for b in range(n)] for a in range(n)], "H": H}


def _triple(model):
    """(fields, metric, potential) of an ``InflationModel`` or of a ``workloads.example_models.ModelSpec``"""
    fields = getattr(model, "coordinates", None)
    return list(fields if fields is not None else model.fields), model.metric, model.potential


_FUNCTIONS = {}


def point_function(model, symbol_dictionary, constants=None):
    """f(x0, x1, p) -> the twelve mpf values (V, g, X^0, X^1, G_00, G_01, G_10, G_11, H_00, H_01, H_10, H_11); a parameter is looked
    up by its printed name in ``symbol_dictionary`` (``"args[k]"``), as ``background_truth.point_function`` does.  ``constants``
    replaces sympy constants (pi, E) before the expressions are lambdified."""
    key = (id(model), tuple(sorted(symbol_dictionary.items())), None if constants is None else tuple(sorted((str(k), str(v)) for k, v in constants.items())))
    if key in _FUNCTIONS:
        return _FUNCTIONS[key][0]
    fields, metric, potential = _triple(model)
    ex = truth_expressions(fields, metric, potential)
    flat = [ex["V"], ex["g"], *ex["X"], *ex["G"][0], *ex["G"][1], *ex["H"][0], *ex["H"][1]]
    if constants:
        flat = [sp.sympify(e).xreplace(constants) for e in flat]
    plain = C99CodePrinter()._print_Symbol
    free = sorted(set().union(*[sp.sympify(e).free_symbols for e in flat]) - set(fields), key=str)
    slots = [int(symbol_dictionary[plain(s)][5:-1]) for s in free]
    fn = sp.lambdify([*fields, *free], flat, modules="mpmath", cse=True)

    def f(a, b, p):
        return fn(mp.mpf(float(a)), mp.mpf(float(b)), *[mp.mpf(float(p[k])) for k in slots])

    _FUNCTIONS[key] = (f, model)  # (the model is kept alive: its id is the key)
    return f


def _project(vals, guess, drop_g01, flip_w):
    V, g, X0, X1, G00, G01, G10, G11, H00, H01, H10, H11 = vals
    if drop_g01:  # the defect the tests are for: inner products and the raising without the off-diagonal component
        G01 = G10 = mp.mpf(0)

    def ip(s, t):
        return G00 * s[0] * t[0] + G01 * s[0] * t[1] + G10 * s[1] * t[0] + G11 * s[1] * t[1]

    n = mp.sqrt(g)
    v = (X0 / n, X1 / n)
    if guess is None:  # the reference's rule: raise the covector (-v^1, v^0) and normalise
        det = G00 * G11 - G01 * G10
        wc = (-v[1], v[0])
        w = ((G11 * wc[0] - G01 * wc[1]) / det, (-G10 * wc[0] + G00 * wc[1]) / det)
    else:  # one Gram-Schmidt step
        gv = (mp.mpf(guess[0]), mp.mpf(guess[1]))
        o = ip(v, gv)
        w = (gv[0] - o * v[0], gv[1] - o * v[1])
        if ip(w, w) <= mp.mpf(10) ** (-(3 * mp.mp.dps) // 2) * ip(gv, gv):
            raise ZeroDivisionError  # the guess is parallel to v to three quarters of the working digits: 0 / 0, what is left is rounding
    wn = mp.sqrt(ip(w, w))
    w = (w[0] / wn, w[1] / wn)
    if flip_w:
        w = (-w[0], -w[1])
    H = ((H00, H01), (H10, H11))

    def pr(s, t):
        return sum(H[i][j] * s[i] * t[j] for i in range(2) for j in range(2))

    return [V, pr(v, v), pr(w, v), pr(w, w), g], [ip(v, v), ip(v, w), ip(w, w), v[0], v[1], w[0], w[1]]


def raw_truth(model, symbol_dictionary, p, pts, guess=None, dps=DPS, drop_g01=False, flip_w=False, constants=None):
    """(rows, basis): per point the mpf values (V, H(v,v), H(w,v), H(w,w), g) and (v.v, v.w, w.w, v^0, v^1, w^0, w^1) -- the
    device's orders.  A point where mpmath divides by zero gives NaN throughout.  ``drop_g01`` / ``flip_w``: deliberately wrong
    variants, for the tests that show what the comparison can see."""
    with mp.workdps(dps):
        fn = point_function(model, symbol_dictionary, constants)
        rows, basis = [], []
        for a, b in np.asarray(pts, dtype=np.float64).reshape(-1, 2):
            try:
                r, e = _project(fn(a, b, p), guess, drop_g01, flip_w)
                r, e = [+c for c in r], [+c for c in e]
                if any(mp.im(c) != 0 for c in r + e):
                    raise ZeroDivisionError
            except ZeroDivisionError:
                r, e = [NAN] * 5, [NAN] * 7
            rows.append(r)
            basis.append(e)
    return rows, basis


def to_float(rows):
    return np.array([[float(c) for c in r] for r in rows], dtype=np.float64).reshape(len(rows), -1)


# ---- tests/tolerance.py's epilogue in mpmath, same operation order ---------------------------------------------------------------
def mp_epilogue(rows, dps=DPS):
    """(six, radicand): per point (consistency, eps_V, eps_H, eta, delta, omega) of ``tolerance.epilogue`` and
    (omega's radicand, |V_tt / V| * 3 -- the size it is judged against).  omega and eta are NaN where the radicand is negative."""
    six, rad = [], []
    with mp.workdps(dps):
        for v, a, b, c, g in rows:
            try:
                lhs = c / v
                rhs = 3 + 3 * (a / b) ** 2 + (a / v) * (b / a) ** 2
                cons = abs(lhs - rhs) / (abs(lhs) + abs(rhs))
                eps_v = g / v**2
                vtt = (a * b**2 + c * a**2 - 2 * a * b**2) / (a**2 + b**2)
                vt2 = eps_v * (1 / (1 + (a / b) ** 2))
                eps_h = 3 * (eps_v - vt2) * (1 / (eps_v + abs(vtt) / v - vt2))
                delta = mp.atan(abs(b / a))
                radicand = (vtt / v) * (3 - eps_h)
                omega = mp.sqrt(radicand) if radicand >= 0 else NAN
                eta = omega * mp.tan(delta) - 3
                six.append([cons, eps_v, eps_h, eta, delta, omega])
                rad.append([radicand, abs(vtt / v) * 3])
            except ZeroDivisionError:
                six.append([NAN] * 6)
                rad.append([NAN] * 2)
    return six, rad


def mp_single_quantities(rows, dps=DPS):
    """{"consistency", "rapidturn", "epsilon_v"}: ``tolerance.single_quantities`` in mpmath, same operation order."""
    out = {"consistency": [], "rapidturn": [], "epsilon_v": []}
    with mp.workdps(dps):
        for v, a, b, c, g in rows:
            try:
                lhs = c / v - 3
                rhs = 3 * (a / b) ** 2 + (a / v) * (b / a) ** 2
                cons = abs(abs(lhs) - abs(rhs)) / (abs(lhs) + abs(rhs))
                lhs2 = c / v
                rhs2 = 3 * (b / a) ** 2
                rapid = abs(abs(lhs2) - abs(rhs2)) / (abs(lhs2) + abs(rhs2))
                eps_v = g / v**2 / 2
            except ZeroDivisionError:
                cons = rapid = eps_v = NAN
            out["consistency"].append(cons)
            out["rapidturn"].append(rapid)
            out["epsilon_v"].append(eps_v)
    return out


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def scale(truth):
    """max(|truth|, 1e-3 x the column's largest finite |truth|): the scale of tests/test_special_gpu.py.  ``truth``: (n,) or (n, k)."""
    t = np.abs(np.asarray(truth, dtype=np.float64))
    top = np.max(np.where(np.isfinite(t), t, 0.0), axis=0, keepdims=True)
    return np.maximum(np.where(np.isfinite(t), t, 0.0), 1e-3 * top)


def worst(got, truth, sc=None):
    """The largest |got - truth| / scale over the values whose truth is finite (``sc``: the scale of a larger set of points)."""
    got, truth = np.asarray(got, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    assert got.shape == truth.shape, (got.shape, truth.shape)
    sc = scale(truth) if sc is None else sc
    fin = np.isfinite(truth)
    assert np.isfinite(got[fin]).all(), "not finite where the truth is"
    return float(np.max((np.abs(got - truth) / sc)[fin])) if fin.any() else 0.0


def nan_rule(got6, six, rad, cap=0.005):
    """NaN patterns of the six outputs must be equal, except for omega and eta where omega's radicand is within 1e-9 of zero
    relative to |V_tt / V| * 3; returns the share of all values excused that way, which must not exceed ``cap``."""
    got6, six, rad = np.asarray(got6), np.asarray(six), np.asarray(rad)
    differ = np.isnan(got6) != np.isnan(six)
    with np.errstate(invalid="ignore"):
        near = np.abs(rad[:, 0]) <= 1e-9 * rad[:, 1]
    allowed = np.zeros_like(differ)
    allowed[:, 3] = allowed[:, 5] = near
    assert not (differ & ~allowed).any(), f"NaN pattern differs at {int((differ & ~allowed).sum())} values"
    share = float(differ.sum()) / differ.size
    assert share <= cap, f"{100 * share:.3f} % of the values excused (cap {100 * cap:.2f} %)"
    return share, differ


# ---- models -----------------------------------------------------------------------------------------------------------------------
class SweepModel(NamedTuple):
    name: str
    model: object
    cse: bool
    box: tuple
    guess: tuple | None


GUESS = {"skew_g": (0, 1), "shear_g": (1, 0)}
NONDIAGONAL = ("skew", "shear", "skew_g", "shear_g")
GPU_MODELS = ("skew", "shear", "shear_g")


@functools.lru_cache(maxsize=None)
def sweep_model(name):
    """``skew`` / ``shear`` of tests/background_truth.py (shear with cse=True); ``skew_g`` / ``shear_g``: the same fields, metric and
    potential built with ``guesses=[[0, 1]]`` / ``[[1, 0]]``; ``fuzz<seed>``: the diagonal models of tests/test_model_fuzz.py."""
    if name in GUESS:
        from inflatox_amd import InflationModelBuilder

        base = bt.nondiagonal_model(name[:-2])
        m = base.model
        built = InflationModelBuilder.new(list(m.coordinates), m.metric, m.potential, model_name=name, silent=True, init_sympy_printing=False, simplify=False, assertions=False).build(
            guesses=[list(GUESS[name])]
        )
        return SweepModel(name, built, base.cse, base.box, GUESS[name])
    z = bt.zoo_model(name)
    return SweepModel(name, z.model, z.cse, z.box, None)


@functools.lru_cache(maxsize=None)
def compiler_for(name, **kw):
    """The ``Compiler`` of a model with its header generated (``.header``); nothing is handed to hipcc."""
    from inflatox_amd import Compiler

    z = sweep_model(name)
    comp = Compiler(z.model, silent=True, cse=z.cse, **kw)
    comp.header = comp._generate_hip_header()
    return comp


@functools.lru_cache(maxsize=None)
def device_artifact(name, **kw):
    from inflatox_amd import Compiler

    z = sweep_model(name)
    return Compiler(z.model, silent=True, cse=z.cse, **kw).compile()


def n_parameters(name):
    return sum(1 for v in compiler_for(name).symbol_dict.values() if v.startswith("args["))


@functools.lru_cache(maxsize=None)
def parameter_rows(name, rows=3):
    """``rows`` parameter rows of a model, a seeded uniform draw in [0.5, 1.8] (the range the models are positive definite for);
    a guess-built model takes the rows of the model it is a variant of."""
    base = name[:-2] if name in GUESS else name
    p = np.random.default_rng(4100 + sum(map(ord, base))).uniform(0.5, 1.8, (rows, n_parameters(name)))
    p.setflags(write=False)
    return p


def grid_points(box, n0, n1):
    """the sweep's points: index * spacing + offset, multiply then add, in float64 (csrc/inflx_ops.h inflx_coord)"""
    x0a, x0b, x1a, x1b = (float(v) for v in box)
    x0 = np.arange(n0, dtype=np.float64) * ((x0b - x0a) / n0) + x0a
    x1 = np.arange(n1, dtype=np.float64) * ((x1b - x1a) / n1) + x1a
    return np.stack(np.meshgrid(x0, x1, indexing="ij"), axis=-1).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def gpu_sample(n0=GRID_GPU[0], n1=GRID_GPU[1], count=400, seed=20):
    """Flat indices into the (n0, n1) grid: a seeded sample of ``count`` points first, then the four corners and the points of the
    last two rows and the last two columns (the ragged row and column tiles and their neighbours), without repetition."""
    rng = np.random.default_rng(seed)
    picked = list(rng.choice(n0 * n1, size=count, replace=False))
    edge = [0, n1 - 1, (n0 - 1) * n1, n0 * n1 - 1]
    edge += [i * n1 + j for i in (n0 - 2, n0 - 1) for j in range(n1)]
    edge += [i * n1 + j for i in range(n0) for j in (n1 - 2, n1 - 1)]
    seen = set(picked)
    for k in edge:
        if k not in seen:
            seen.add(k)
            picked.append(k)
    out = np.array(picked, dtype=np.int64)
    out.setflags(write=False)
    return out


class Truth(NamedTuple):
    rows: list  # mpf (n, 5)
    basis: list  # mpf (n, 7)
    raw: np.ndarray  # float64 (n, 5)
    frame: np.ndarray  # float64 (n, 7)
    six: np.ndarray  # float64 (n, 6)
    radicand: np.ndarray  # float64 (n, 2)
    single: dict  # name -> float64 (n,)
    hesse: np.ndarray  # float64 (n, 4): v00, v01 = v10, v10, v11


_TRUTHS = {}


def truth(name, p, pts, **variant):
    """The truth of a model at one parameter row and a set of points, evaluated once per (model, row, points, variant) and shared."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 2)
    key = (name, p.tobytes(), pts.tobytes(), tuple(sorted(variant.items())))
    if key not in _TRUTHS:
        z = sweep_model(name)
        rows, basis = raw_truth(z.model, compiler_for(name).symbol_dict, p, pts, guess=z.guess, **variant)
        six, rad = mp_epilogue(rows)
        single = {k: np.array([float(c) for c in v]) for k, v in mp_single_quantities(rows).items()}
        raw = to_float(rows)
        arrays = [raw, to_float(basis), to_float(six), to_float(rad), raw[:, [1, 2, 2, 3]]]
        for a in arrays + list(single.values()):
            a.setflags(write=False)
        _TRUTHS[key] = Truth(rows, basis, arrays[0], arrays[1], arrays[2], arrays[3], single, arrays[4])
    return _TRUTHS[key]
