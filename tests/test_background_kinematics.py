"""Trajectory kinematics without a GPU: the generated kinematics header and csrc/inflx_kinematics.h, compiled for the host
(tests/kinematics_twin.cpp), against a 40-digit truth that takes another route (tests/kinematics_reference.py) on fuzzed curved
field spaces and on metrics with G_01 != 0; epsilon_H against the integrator's; the Pythagorean identity against the host oracle;
coordinate invariance on the flat plane; and the argument checks of ``kinematics`` and ``turn_rate_map``.  The states and bounds of
tests/test_background_kinematics_gpu.py are those established here."""

import numpy as np
import pytest

import background_truth as bt
import kinematics_reference as kr
import workloads

LANES = 65


@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_host_twin_against_truth(name):
    """The first 65 lanes of the model's batch, H from the Friedmann constraint, a parameter row per lane, no state left out: every
    quantity within the allowance of tests/kinematics_reference.py (1e-10 of the size of the terms it is built from) of the
    40-digit truth.  Measured worst ratios to the allowance: profiles/background_kinematics.json."""
    states, pars = (a[:LANES] for a in kr.zoo_states(name))
    truth = kr.zoo_truth(name, 257)[:LANES]
    assert np.isfinite(truth).all() and np.all(truth[:, 3] > 0)
    got = kr.KinematicsTwin(bt.host_artifact(name)).kinematics(pars, states)
    ratios = kr.worst_ratios(got, truth, states[:, 4])
    print(f"{name}: worst |got - truth| / allowance {ratios}")
    assert np.isfinite(got).all()
    assert max(ratios.values()) <= 1.0, (name, ratios)
    # omega is signed, and both signs occur
    assert np.array_equal(np.sign(got[2]), np.sign(truth[:, 2]))


def test_both_signs_of_omega_occur():
    signs = np.concatenate([np.sign(kr.zoo_truth(name, 257)[:LANES, 2]) for name in bt.GPU_MODELS])
    assert (signs > 0).sum() > 50 and (signs < 0).sum() > 50


@pytest.mark.parametrize("name", ["fuzz1", "shear"])
def test_epsilon_h_is_the_integrators(name):
    """Bit-equal to the integrator's own epsilon_H: the sampled stepper's host twin emits a sample at 0 -- the initial state with H
    from the Friedmann constraint and ``inflx_bg_epsilon`` there -- and the kinematics twin at that very state returns the same
    bits.  Both twins are built without contraction, like every integrator twin."""
    from background_sampled_reference import SampledTwin

    art = bt.host_artifact(name)
    init, pars = (a[:LANES] for a in bt.batch(name))
    sampled, twin = SampledTwin(art), kr.KinematicsTwin(art)
    states, eps = np.empty((LANES, 5)), np.empty(LANES)
    for k in range(LANES):
        out, _meta = sampled.solve(pars[k], init[k], [0.0], 0, "rkf", stop_at_end=False)
        states[k], eps[k] = out[0, :5], out[0, 7]
    got = twin.kinematics(pars, states)
    assert np.isfinite(eps).all() and np.all(eps > 0)
    assert np.array_equal(got[0], eps)


@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_slopes_square_to_the_gradient_norm(name):
    """V_sigma^2 + V_N^2 = |dV|^2_G.  complete_analysis's epsilon_V is g / V^2 (csrc/inflx_ops.h, no factor 1/2), so |dV|^2 =
    epsilon_V V^2 from the host oracle -- the reference's generated C, which knows nothing of velocities -- at the same points, within
    1e-10 S^2 (the parity bar on the size of the term)."""
    import oracle

    z = bt.zoo_model(name)
    src, symdict = oracle.emit_c_source(z.model, cse=z.cse)
    assert symdict == bt.host_artifact(name).symbol_dictionary
    om = oracle.OracleModel(oracle.compile_c_model(src))
    states, pars = (a[:LANES] for a in kr.zoo_states(name))
    truth = kr.zoo_truth(name, 257)[:LANES]
    got = kr.KinematicsTwin(bt.host_artifact(name)).kinematics(pars, states)
    want = np.array([om.trajectory_sweep(oracle.OP.COMPLETE, pars[k], states[k : k + 1, :2])[0, 1] * om.potential(states[k, :2], pars[k]) ** 2 for k in range(LANES)])
    err = np.abs(got[4] ** 2 + got[5] ** 2 - want) / truth[:, 6]
    print(f"{name}: |V_sigma^2 + V_N^2 - epsilon_V V^2| / S^2 {err.max():.3e}; oracle against the 40-digit S^2 {np.max(np.abs(want - truth[:, 6]) / truth[:, 6]):.3e}")
    assert err.max() <= kr.RTOL, err.max()


def test_coordinate_invariance_on_the_flat_plane():
    """The flat plane as polar and as Cartesian coordinates, the same potential, 65 corresponding states with r in [0.5, 3]: the six
    quantities are scalars, so the two charts agree within the allowance -- omega with its sign, which both signs of occur."""
    polar_model, cart_model = kr.plane_models()
    polar, cart, a, b = kr.plane_states(LANES)
    arts = [kr.host_artifact_of(m) for m in (polar_model, cart_model)]
    pars = []
    for art in arts:
        p = np.zeros(art.n_parameters)
        p[int(art.symbol_dictionary["a"][5:-1])] = a
        p[int(art.symbol_dictionary["b"][5:-1])] = b
        pars.append(p)
    got_polar = kr.KinematicsTwin(arts[0]).kinematics(pars[0], polar)
    got_cart = kr.KinematicsTwin(arts[1]).kinematics(pars[1], cart)
    f = kr.truth_function(polar_model.coordinates, polar_model.metric, polar_model.potential, polar_model.coordinate_tangents, arts[0].symbol_dictionary)
    truth = kr.truth_table(f, polar, pars[0])
    allow = kr.allowance(truth, polar[:, 4])
    ratio = np.abs(got_polar - got_cart) / allow
    print(f"polar against Cartesian: worst difference / allowance {ratio.max(axis=1)}; polar against truth {kr.worst_ratios(got_polar, truth, polar[:, 4])}")
    assert np.isfinite(got_polar).all() and np.isfinite(got_cart).all()
    assert ratio.max() <= 1.0, ratio.max(axis=1)
    assert np.array_equal(np.sign(got_polar[2]), np.sign(got_cart[2])) and (got_polar[2] > 0).any() and (got_polar[2] < 0).any()
    assert max(kr.worst_ratios(got_polar, truth, polar[:, 4]).values()) <= 1.0


def test_edge_values_of_the_device_function():
    """A NaN component gives six NaNs; a state at rest gives eps_H = 0, sigma_dot = 0 and NaN in the other four."""
    name = "skew"
    states, pars = (a[:6].copy() for a in kr.zoo_states(name))
    for c in range(5):
        states[c, c] = np.nan
    states[5, 2:4] = 0.0
    got = kr.KinematicsTwin(bt.host_artifact(name)).kinematics(pars, states)
    assert np.isnan(got[:, :5]).all()
    assert got[0, 5] == 0.0 and got[3, 5] == 0.0 and np.isnan(got[[1, 2, 4, 5], 5]).all()


def _nonfinite_cases(base):
    """(states (1 + 15, 5), the finite base first): each component of ``base`` in turn replaced by NaN, +inf and -inf"""
    rows = [np.array(base, dtype=np.float64)]
    for c in range(5):
        for bad in (np.nan, np.inf, -np.inf):
            rows.append(rows[0].copy())
            rows[-1][c] = bad
    return np.array(rows)


def test_a_component_that_is_not_finite_gives_six_nans_on_cyclic_coordinates():
    """Models that never read one of the coordinates: hyperbolic (G and V depend on phi alone, theta is cyclic) and the Cartesian
    plane (a flat metric).  NaN or +-inf in ANY of the five components -- the cyclic coordinate, H, which three of the quantities do
    not divide by -- gives six NaNs, and the finite state next to them six finite numbers."""
    spec, hyper = workloads.artifact_for("hyperbolic")
    _polar, cart_model = kr.plane_models()
    cart = kr.host_artifact_of(cart_model)
    for art, pars, base in ((hyper, spec.args, (2.0, 0.3, 0.1, 0.2, 0.7)), (cart, np.array([1.3, 0.6]), (1.5, -0.5, 0.1, 0.2, 0.7))):
        states = _nonfinite_cases(base)
        got = kr.KinematicsTwin(art).kinematics(pars, states)
        assert np.isfinite(got[:, 0]).all(), got[:, 0]
        assert np.isnan(got[:, 1:]).all(), np.argwhere(~np.isnan(got[:, 1:]))
        # the taint is a zero: the finite state's values are those of the plain formulas
        kin = 2.0 * got[0, 0] * base[4] ** 2
        assert abs(got[3, 0] - np.sqrt(kin)) <= 1e-14 * got[3, 0] and got[0, 0] > 0


def test_strided_states_and_parameter_rows_of_the_twin():
    """ld = 6 with a sixth column of NaN and one parameter row per three states: bit for bit the flat call."""
    name = "fuzz0"
    states, pars = (a[:12] for a in kr.zoo_states(name))
    twin = kr.KinematicsTwin(bt.host_artifact(name))
    rows = np.repeat(pars[:4], 3, axis=0)
    flat = twin.kinematics(rows, states)
    wide = np.concatenate([states, np.full((12, 1), np.nan)], axis=1)
    assert np.array_equal(twin.kinematics(pars[:4], wide, traj_len=3), flat)


def test_state_stride():
    from inflatox_amd.background import _state_stride

    assert _state_stride((5,), (1,)) == 5
    assert _state_stride((7, 5), (5, 1)) == 5 and _state_stride((7, 5), (6, 1)) == 6 and _state_stride((1, 5), (99, 1)) == 5
    assert _state_stride((3, 4, 5), (24, 6, 1)) == 6 and _state_stride((3, 4, 5), (20, 5, 1)) == 5
    assert _state_stride((3, 1, 5), (6, 6, 1)) == 6 and _state_stride((1, 4, 5), (0, 7, 1)) == 7
    for shape, strides in (((7, 5), (5, 2)), ((7, 5), (-5, 1)), ((7, 5), (4, 1)), ((3, 4, 5), (30, 6, 1)), ((3, 4, 5), (24, 5, 1)), ((4, 3, 5), (5, 20, 1)), ((7, 5), (0, 1))):
        assert _state_stride(shape, strides) is None, (shape, strides)


def test_public_names_and_the_generated_header():
    import ctypes
    import os

    from conftest import ROOT
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import _BACKGROUND_SOURCES, _KINEMATICS_SOURCES

    assert {"kinematics", "turn_rate_map", "Kinematics"} <= set(background.__all__)
    assert background.Kinematics._fields == ("eps_H", "eta_par", "omega", "sigma_dot", "V_sigma", "V_N")
    assert not set(_KINEMATICS_SOURCES) & set(_BACKGROUND_SOURCES)
    _native.build_library()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "inflx_kinematics") and hasattr(lib, "inflx_kinematics_device")
    assert len(_native.SIGNATURES["inflx_kinematics"][1]) == 9 and len(_native.SIGNATURES["inflx_kinematics_device"][1]) == 12
    abi = open(os.path.join(ROOT, "inflatox_amd", "csrc", "inflx_kinematics_abi.h")).read()
    assert "#define INFLX_KIN_ABI_VERSION 1" in abi
    _, art = workloads.artifact_for("hyperbolic")
    text = art.kinematics_header_text()
    assert "INFLX_FN void inflx_kin_point(" in text and "o[1] = (dv0 * xl1 - dv1 * xl0) / sqrt(det);" in text
    path = art.ensure_kinematics()
    assert path == art.shared_object_path + ".kinematics" and os.path.getsize(path) > 0
    # the object's exports: the kernel, its layout word, the model tag -- and the background object is another file
    from test_background_rows import _elf_symbols
    import struct

    data, sections, symbols = _elf_symbols(path)
    for sym in ("inflx_kin_states", "inflx_kin_states.kd", "INFLX_KIN_ABI", "MODEL_TAG", "VERSION"):
        assert sym in symbols, sym
    value, size, shndx = symbols["INFLX_KIN_ABI"]
    assert size == 4 and struct.unpack_from("<I", data, sections[shndx][4] + value - sections[shndx][3])[0] == 1
    assert "INFLX_BG_ABI" not in symbols and not any(s.startswith("inflx_bg_") for s in symbols)
    assert art.ensure_background() != path


def test_bad_arguments_raise_before_the_device(monkeypatch):
    """Every bad-argument case of ``kinematics`` and ``turn_rate_map``, with the handle made to fail."""
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
            background.kinematics(a, pars, states)
        assert err.type is exc, (states.shape, err.type)
    # good arguments get as far as the device
    for pars, states in ((p, ok), (np.tile(p, (4, 1)), ok), (np.tile(p, (2, 1)), np.ones((2, 3, 5))), (p, np.ones(5)), (np.tile(p, (1, 1)), np.ones(5))):
        with pytest.raises(AssertionError, match="a device call was made"):
            background.kinematics(art, pars, states)
    # no state: nothing to do, and nothing is done
    empty = background.kinematics(art, p, np.empty((0, 5)))
    assert all(q.shape == (0,) for q in empty) and background.kinematics(art, p, np.empty((3, 0, 5))).omega.shape == (3, 0)
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
            background.turn_rate_map(c.get("a", art), c.get("p", p), c.get("ss", ss), c.get("N0", 4), c.get("N1", 4), **c.get("kw", {}))
        assert err.type is exc, (c, err.type)
    with pytest.raises(AssertionError, match="a device call was made"):
        background.turn_rate_map(art, p, ss, 4, 4)
