"""Entropic masses without a GPU: the generated masses header and csrc/inflx_masses.h, compiled for the host
(tests/masses_twin.cpp), against a 40-digit truth that takes other routes (tests/masses_reference.py) on fuzzed curved field spaces
and on metrics with G_01 != 0; the Laplace-Beltrami trace; known curvatures and Hesse components; coordinate invariance on the flat
plane; the tie to the sweeps' Hesse planes on the doc model; edge values; and the argument checks of ``masses`` and ``mass_map``.
The states and bounds of tests/test_background_masses_gpu.py are those established here."""

import numpy as np
import pytest

import background_truth as bt
import kinematics_reference as kr
import masses_reference as mr
import workloads

LANES = 65


@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_host_twin_against_truth(name):
    """The first 65 states of the kinematics' zoo states, a parameter row per state, no state left out: every quantity within the
    allowance of tests/masses_reference.py (1e-10 of the sum of the absolute values of the terms it is built from) of the 40-digit
    truth.  Measured worst ratios to the allowance: profiles/background_masses.json."""
    states, pars = (a[:LANES] for a in kr.zoo_states(name))
    truth = mr.zoo_truth(name, 257)[:LANES]
    assert np.isfinite(truth).all() and np.all(truth[:, mr.SIGMA_DOT] > 0)
    got = mr.MassesTwin(bt.host_artifact(name)).masses(pars, states)
    ratios = mr.worst_ratios(got, truth, states[:, 4])
    print(f"{name}: worst |got - truth| / allowance {ratios}")
    assert np.isfinite(got).all()
    assert max(ratios.values()) <= 1.0, (name, ratios)
    assert np.array_equal(np.sign(got[5]), np.sign(truth[:, 5]))
    # eps_H and omega are the kinematics twin's, bit for bit (both twins are built without contraction)
    kin = kr.KinematicsTwin(bt.host_artifact(name)).kinematics(pars, states)
    assert np.array_equal(got[4], kin[0]) and np.array_equal(got[5], kin[2])


def test_the_zoo_is_curved_and_the_normal_matters():
    """What the comparison above can see: fields spaces of either sign of R, and V_TN of either sign."""
    truth = np.concatenate([mr.zoo_truth(name, 257)[:LANES] for name in bt.GPU_MODELS])
    assert (truth[:, 3] > 1e-3).sum() > 20 and (truth[:, 3] < -1e-3).sum() > 20
    assert (truth[:, 1] > 0).sum() > 50 and (truth[:, 1] < 0).sum() > 50


@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_trace_is_the_laplace_beltrami_operator(name):
    """V_TT + V_NN = G^ab V_;ab = (1 / sqrt g) d_a (sqrt g G^ab d_b V), within the allowances of the two summands."""
    states, pars = (a[:LANES] for a in kr.zoo_states(name))
    truth = mr.zoo_truth(name, 257)[:LANES]
    got = mr.MassesTwin(bt.host_artifact(name)).masses(pars, states)
    allow = mr.allowance(truth, states[:, 4])
    ratio = np.abs(got[0] + got[2] - truth[:, mr.TRACE]) / (allow[0] + allow[2])
    print(f"{name}: worst |V_TT + V_NN - Laplace-Beltrami| / allowance {ratio.max():.3e}")
    assert ratio.max() <= 1.0, ratio.max()


def _random_states(rng, n, lo, hi):
    """(n, 5): points in the box (lo, hi) of the chart, velocities in [-0.4, 0.4] and H in [0.5, 1]"""
    return np.concatenate([rng.uniform(lo, hi, (n, 2)), rng.uniform(-0.4, 0.4, (n, 2)), rng.uniform(0.5, 1.0, (n, 1))], axis=1)


def _checked(model, art, pars, states):
    """the twin's (8, n) at the states, checked against the model's own 40-digit truth; returns (got, truth, allowance)"""
    truth = mr.truth_table(mr.model_truth_function(model, art), states, pars)
    got = mr.MassesTwin(art).masses(pars, states)
    ratios = mr.worst_ratios(got, truth, states[:, 4])
    assert max(ratios.values()) <= 1.0, (model.model_name, ratios)
    return got, truth, mr.allowance(truth, states[:, 4])


@pytest.mark.parametrize("L", [0.5, 1.0, 3.0])
def test_ricci_of_the_hyperbolic_model(L):
    """diag(1, L^2 sinh^2(phi / L)): R = -2 / L^2."""
    _spec, art = workloads.artifact_for("hyperbolic")
    model = workloads.model_for("hyperbolic")
    pars = mr.parameter_row(art, **{"m": 0.7, "φ0": 0.4, "L": L})
    states = _random_states(np.random.default_rng(11), 17, (0.5, -2.0), (3.0, 2.0))
    got, _truth, allow = _checked(model, art, pars, states)
    assert np.all(np.abs(got[3] + 2.0 / L**2) <= allow[3]), (got[3], allow[3])
    assert np.all(got[3] < 0)


def test_ricci_of_a_sphere():
    """diag(r^2, r^2 sin^2 x0): R = +2 / r^2."""
    model = mr.sphere_model()
    art = kr.host_artifact_of(model)
    states = _random_states(np.random.default_rng(12), 17, (0.4, -3.0), (2.7, 3.0))
    for r in (0.6, 1.0, 2.5):
        got, _truth, allow = _checked(model, art, mr.parameter_row(art, a=1.1, r=r), states)
        assert np.all(np.abs(got[3] - 2.0 / r**2) <= allow[3]), (r, got[3])


def test_ricci_of_the_flat_plane():
    """R = 0 in polar coordinates within the allowance of its terms, and exactly 0 in Cartesian ones, where every term is zero."""
    polar_model, cart_model = kr.plane_models()
    polar, cart, a, b = kr.plane_states(LANES)
    arts = [kr.host_artifact_of(m) for m in (polar_model, cart_model)]
    got_polar, _truth, allow = _checked(polar_model, arts[0], mr.parameter_row(arts[0], a=a, b=b), polar)
    assert np.all(np.abs(got_polar[3]) <= allow[3]) and np.all(allow[3] > 0)
    got_cart, truth_cart, _allow = _checked(cart_model, arts[1], mr.parameter_row(arts[1], a=a, b=b), cart)
    assert np.all(got_cart[3] == 0.0) and np.all(truth_cart[:, mr.S_R] == 0.0)


def test_radial_motion_on_the_hyperbolic_model():
    """chi along phi alone: V_TT = V_;phi phi = m^2 and V_NN = V_;theta theta / G_theta theta = m^2 (phi - phi0) / (L tanh(phi / L))."""
    _spec, art = workloads.artifact_for("hyperbolic")
    model = workloads.model_for("hyperbolic")
    m, phi0, L = 0.7, 0.4, 1.5
    pars = mr.parameter_row(art, **{"m": m, "φ0": phi0, "L": L})
    states = _random_states(np.random.default_rng(13), 17, (0.5, -2.0), (3.0, 2.0))
    states[:, 3] = 0.0
    states[:, 2] = np.where(np.arange(17) % 2, 1.0, -1.0) * (0.05 + np.abs(states[:, 2]))
    got, _truth, allow = _checked(model, art, pars, states)
    phi = states[:, 0]
    assert np.all(np.abs(got[0] - m**2) <= allow[0])
    assert np.all(np.abs(got[2] - m**2 * (phi - phi0) / (L * np.tanh(phi / L))) <= allow[2])
    assert np.all(np.abs(got[1]) <= allow[1])


def test_coordinate_invariance_on_the_flat_plane():
    """The flat plane as polar and as Cartesian coordinates, the same potential, 65 corresponding states with r in [0.5, 3]: V_TT,
    V_TN, V_NN, M_eff2 and mu_s2 are scalars of charts of the same orientation, so the two agree within the allowance."""
    polar_model, cart_model = kr.plane_models()
    polar, cart, a, b = kr.plane_states(LANES)
    arts = [kr.host_artifact_of(m) for m in (polar_model, cart_model)]
    got_polar, _truth, allow = _checked(polar_model, arts[0], mr.parameter_row(arts[0], a=a, b=b), polar)
    got_cart = mr.MassesTwin(arts[1]).masses(mr.parameter_row(arts[1], a=a, b=b), cart)
    ratio = np.abs(got_polar - got_cart) / np.where(allow > 0, allow, np.inf)
    print(f"polar against Cartesian: worst difference / allowance {dict(zip(mr.NAMES, ratio.max(axis=1)))}")
    assert np.isfinite(got_polar).all() and np.isfinite(got_cart).all()
    for q in (0, 1, 2, 6, 7):
        assert ratio[q].max() <= 1.0, (mr.NAMES[q], ratio[q].max())
    # in Cartesian coordinates the Hesse matrix is diag(a, b): V_TT + V_NN = a + b, and V_TN is of either sign
    assert np.all(np.abs(got_cart[0] + got_cart[2] - (a + b)) <= allow[0] + allow[2])
    assert (got_cart[1] > 0).any() and (got_cart[1] < 0).any() and np.array_equal(np.sign(got_polar[1]), np.sign(got_cart[1]))


def test_doc_model_along_the_gradient_is_the_sweeps_hesse_matrix():
    """The doc model at 16 points with chi = -G^ab d_b V: T = -v, the first vector of the sweeps' gradient basis, so V_TT = v00,
    V_NN = v11 and V_TN = v10 up to the sign convention of w -- here against the 40-digit covariant Hesse matrix projected on the
    normalised gradient and its normal, formed in this test."""
    import mpmath
    import sympy as sp
    from workloads import example_models

    spec, art = workloads.artifact_for("doc")
    model = workloads.model_for("doc")
    states, pts = mr.doc_gradient_states()
    assert states.shape == (16, 5) and np.isfinite(states).all() and np.all(states[:, 4] > 0)
    got, _truth, allow = _checked(model, art, spec.args, states)
    r, th = example_models.get("doc").fields
    V = sp.sympify(spec.potential).subs({s: 1 for s in sp.sympify(spec.potential).free_symbols - {r, th}})
    G = sp.Matrix(spec.metric)
    Ginv, x = G.inv(), [r, th]
    gamma = [[[sum(Ginv[c, d] * (sp.diff(G[d, a], x[b]) + sp.diff(G[d, b], x[a]) - sp.diff(G[a, b], x[d])) for d in range(2)) / 2 for b in range(2)] for a in range(2)] for c in range(2)]
    hesse = sp.Matrix(2, 2, lambda a, b: sp.diff(V, x[a], x[b]) - sum(gamma[c][a][b] * sp.diff(V, x[c]) for c in range(2)))
    grad = Ginv * sp.Matrix([sp.diff(V, r), sp.diff(V, th)])
    v = grad / sp.sqrt((grad.T * G * grad)[0])
    v_low = G * v
    w = sp.Matrix([v_low[1], -v_low[0]]) / sp.sqrt(G.det())
    fn = sp.lambdify([r, th], [(v.T * hesse * v)[0], (v.T * hesse * w)[0], (w.T * hesse * w)[0], (w.T * G * w)[0], (v.T * G * w)[0]], modules="mpmath")
    with mpmath.workdps(mr.DPS):
        want = np.array([[float(q) for q in fn(mpmath.mpf(float(a)), mpmath.mpf(float(b)))] for a, b in pts])
    assert np.allclose(want[:, 3], 1.0, atol=1e-30, rtol=1e-15) and np.all(np.abs(want[:, 4]) < 1e-30)
    assert np.all(np.abs(got[0] - want[:, 0]) <= allow[0])
    assert np.all(np.abs(got[2] - want[:, 2]) <= allow[2])
    assert np.all(np.abs(np.abs(got[1]) - np.abs(want[:, 1])) <= allow[1])
    assert np.all(np.abs(want[:, 1]) > 100 * allow[1])  # (v10 is there to be seen)


def _nonfinite_cases(base):
    """(states (1 + 15, 5), the finite base first): each component of ``base`` in turn replaced by NaN, +inf and -inf"""
    rows = [np.array(base, dtype=np.float64)]
    for c in range(5):
        for bad in (np.nan, np.inf, -np.inf):
            rows.append(rows[0].copy())
            rows[-1][c] = bad
    return np.array(rows)


def test_a_component_that_is_not_finite_gives_eight_nans():
    """hyperbolic (theta is cyclic) and the Cartesian plane (no coordinate is read at all, and R is the constant 0): NaN or +-inf in
    ANY of the five components gives eight NaNs -- ricci included, which reads neither a velocity nor H -- and the finite state next
    to them eight finite numbers."""
    spec, hyper = workloads.artifact_for("hyperbolic")
    _polar, cart_model = kr.plane_models()
    cart = kr.host_artifact_of(cart_model)
    for art, pars, base in ((hyper, spec.args, (2.0, 0.3, 0.1, 0.2, 0.7)), (cart, np.array([1.3, 0.6]), (1.5, -0.5, 0.1, 0.2, 0.7))):
        got = mr.MassesTwin(art).masses(pars, _nonfinite_cases(base))
        assert np.isfinite(got[:, 0]).all(), got[:, 0]
        assert np.isnan(got[:, 1:]).all(), np.argwhere(~np.isnan(got[:, 1:]))


def test_a_state_at_rest():
    """kin = 0: eps_H = 0, a finite ricci and NaN in the other six; the moving state next to it is finite."""
    name = "skew"
    states, pars = (a[:2].copy() for a in kr.zoo_states(name))
    states[1, 2:4] = 0.0
    got = mr.MassesTwin(bt.host_artifact(name)).masses(pars, states)
    assert np.isfinite(got[:, 0]).all()
    assert got[4, 1] == 0.0 and np.isfinite(got[3, 1]) and got[3, 1] != 0.0 and np.isnan(got[[0, 1, 2, 5, 6, 7], 1]).all()


def test_strided_states_and_parameter_rows_of_the_twin():
    """ld = 6 with a sixth column of NaN and one parameter row per three states: bit for bit the flat call."""
    name = "fuzz0"
    states, pars = (a[:12] for a in kr.zoo_states(name))
    twin = mr.MassesTwin(bt.host_artifact(name))
    flat = twin.masses(np.repeat(pars[:4], 3, axis=0), states)
    wide = np.concatenate([states, np.full((12, 1), np.nan)], axis=1)
    assert np.array_equal(twin.masses(pars[:4], wide, traj_len=3), flat)
    assert not np.array_equal(twin.masses(pars[0], states), flat)  # (the rows matter)


def test_mass_point_is_not_yet_divided_by_kin():
    """inflx_mass_point's o[0..2] are V_;ab chi^a chi^b, V_;ab chi^a n^b, V_;ab n^a n^b: kin times V_TT, V_TN, V_NN; o[3] is R."""
    name = "shear"
    states, pars = (a[:9] for a in kr.zoo_states(name))
    truth = mr.zoo_truth(name, 257)[:9]
    twin = mr.MassesTwin(bt.host_artifact(name))
    allow = mr.allowance(truth, states[:, 4])
    kin = truth[:, mr.SIGMA_DOT] ** 2
    for k in range(9):
        o = twin.mass_point(pars[k], states[k : k + 1, :4])[0]
        assert np.all(np.abs(o[:3] - kin[k] * truth[k, :3]) <= kin[k] * allow[:3, k]) and abs(o[3] - truth[k, 3]) <= allow[3, k]


def test_public_names_and_the_generated_header():
    import ctypes
    import os
    import struct

    from conftest import ROOT
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import _BACKGROUND_SOURCES, _KINEMATICS_SOURCES, _MASSES_SOURCES
    from test_background_rows import _elf_symbols

    assert {"masses", "mass_map", "Masses"} <= set(background.__all__)
    assert background.Masses._fields == mr.NAMES
    assert not set(_MASSES_SOURCES) & (set(_BACKGROUND_SOURCES) | set(_KINEMATICS_SOURCES))
    _native.build_library()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "inflx_masses") and hasattr(lib, "inflx_masses_device")
    assert _native.SIGNATURES["inflx_masses"] == _native.SIGNATURES["inflx_kinematics"]
    assert _native.SIGNATURES["inflx_masses_device"] == _native.SIGNATURES["inflx_kinematics_device"]
    abi = open(os.path.join(ROOT, "inflatox_amd", "csrc", "inflx_masses_abi.h")).read()
    assert "#define INFLX_MASS_ABI_VERSION 1" in abi and "#define INFLX_MASS_PLANES 8" in abi and "sizeof(InflxMassArgs) == 64" in abi
    _, art = workloads.artifact_for("hyperbolic")
    text = art.masses_header_text()
    assert "INFLX_FN void inflx_mass_point([[maybe_unused]] const double x0, [[maybe_unused]] const double x1, [[maybe_unused]] const double xd0, " in text
    assert "o[3] = ricci;" in text and "inflx_kin_point" not in text and "inflx_eom_point" not in text
    # a file of its own: the other generated headers are what they were
    assert "inflx_mass_point" not in art.kinematics_header_text() + art.eom_header_text() + art._build[0]
    path = art.ensure_masses()
    assert path == art.shared_object_path + ".masses" and os.path.getsize(path) > 0
    data, sections, symbols = _elf_symbols(path)
    for sym in ("inflx_mass_states", "inflx_mass_states.kd", "INFLX_MASS_ABI", "MODEL_TAG", "VERSION"):
        assert sym in symbols, sym
    value, size, shndx = symbols["INFLX_MASS_ABI"]
    assert size == 4 and struct.unpack_from("<I", data, sections[shndx][4] + value - sections[shndx][3])[0] == 1
    assert "INFLX_BG_ABI" not in symbols and "INFLX_KIN_ABI" not in symbols and not any(s.startswith(("inflx_bg_", "inflx_kin_states")) for s in symbols)
    assert len({path, art.ensure_background(), art.ensure_kinematics()}) == 3


def test_bad_arguments_raise_before_the_device(monkeypatch):
    """Every bad-argument case of ``masses`` and ``mass_map``, with the handle made to fail."""
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    shape, value = _native.InflatoxShapeError, ValueError
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    ok = np.ones((4, 5))
    cases = [
        (shape, three, p, ok),  # not a two-field model
        (shape, art, p, np.ones(4)),  # not five components
        (shape, art, p, np.ones((4, 6))),
        (shape, art, p, np.ones((2, 3, 4))),
        (shape, art, p, np.ones((2, 2, 2, 5))),  # too many axes
        (shape, art, p, np.float64(1.0)),
        (value, art, p, np.array([["a"] * 5])),  # not numbers
        (shape, art, p[:2], ok),  # parameters
        (shape, art, np.zeros((3, p.size)), ok),  # one row per state: 4
        (shape, art, np.zeros((4, p.size)), np.ones((2, 4, 5))),  # one row per trajectory: 2
        (shape, art, np.zeros((2, p.size)), np.ones(5)),  # one state: one row
        (shape, art, np.zeros((1, 1, p.size)), ok),
    ]
    for exc, a, pars, states in cases:
        with pytest.raises(exc) as err:
            background.masses(a, pars, states)
        assert err.type is exc, (states.shape, err.type)
    # good arguments get as far as the device
    for pars, states in ((p, ok), (np.tile(p, (4, 1)), ok), (np.tile(p, (2, 1)), np.ones((2, 3, 5))), (p, np.ones(5)), (np.tile(p, (1, 1)), np.ones(5))):
        with pytest.raises(AssertionError, match="a device call was made"):
            background.masses(art, pars, states)
    # no state: nothing to do, and nothing is done
    empty = background.masses(art, p, np.empty((0, 5)))
    assert len(empty) == 8 and all(q.shape == (0,) for q in empty) and background.masses(art, p, np.empty((3, 0, 5))).mu_s2.shape == (3, 0)
    ss = [[2.0, 5.0], [-1.0, 1.0]]
    grid_cases = [
        (shape, dict(a=three)),
        (shape, dict(ss=[1.0, 2.0, 3.0])),
        (value, dict(N0=0)),
        (value, dict(N1=-1)),
        (shape, dict(p=p[:2])),
        (shape, dict(p=np.tile(p, (2, 1)))),  # one parameter row
        (shape, dict(kw=dict(derivatives_init=(0.0, 0.0, 0.0)))),
        (value, dict(kw=dict(N_star=-1.0))),
        (value, dict(kw=dict(N_star=float("nan")))),
        (value, dict(kw=dict(max_steps=0))),
        (value, dict(kw=dict(max_err=0.0))),
        (value, dict(kw=dict(solver="euler"))),
    ]
    for exc, c in grid_cases:
        with pytest.raises(exc) as err:
            background.mass_map(c.get("a", art), c.get("p", p), c.get("ss", ss), c.get("N0", 4), c.get("N1", 4), **c.get("kw", {}))
        assert err.type is exc, (c, err.type)
    with pytest.raises(AssertionError, match="a device call was made"):
        background.mass_map(art, p, ss, 4, 4)
