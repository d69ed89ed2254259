"""Entropic masses on the GPU (inflatox_amd.background.masses, mass_map): the kernel against the 40-digit truth of
tests/masses_reference.py on fuzzed curved field spaces and metrics with G_01 != 0, eps_H and omega against ``kinematics``' bit for
bit, the shapes and strides of the states, the device-resident path, the chunks of a large host call, ``mass_map`` against its two
halves, the tie to ``calc_H`` on the doc model, and the refusal of a masses object of another layout.  States, truth and bounds are
those tests/test_background_masses.py establishes on the host build."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import background_truth as bt
import kinematics_reference as kr
import masses_reference as mr
import workloads
from test_background_gpu import _hyper_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


def _same(a, b):
    """two Masses of numpy arrays: the same shapes and the same values, NaN where NaN"""
    return len(a) == len(b) == 8 and all(u.shape == w.shape and np.array_equal(u, w, equal_nan=True) for u, w in zip(a, b))


def _hyperbolic_ricci_allowance(phi):
    """1e-10 of the terms of R = -2 / L^2 on the hyperbolic model at L = 1 as the code adds them up: d_0 d_0 G_11 / det G =
    2 (sinh^2 + cosh^2) / sinh^2 and the product of first-kind symbols 2 cosh^2 / sinh^2"""
    return mr.RTOL * (2.0 + 4.0 / np.tanh(phi) ** 2)


def _host(mass):
    return type(mass)(*(q.cpu().numpy() for q in mass))


@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_kernel_against_truth(bg, name):
    """257 states (four wavefronts and one lane), one parameter row each (traj_len = 1, ld = 5): every quantity within the allowance
    of the 40-digit truth; the difference to the host twin is printed.  eps_H and omega are ``kinematics``' at the same states, bit
    for bit.  Measured: profiles/background_masses.json."""
    art = bt.device_artifact(name)
    states, pars = kr.zoo_states(name)
    truth = mr.zoo_truth(name, 257)
    mass = bg.masses(art, pars, states)
    assert isinstance(mass, bg.Masses) and all(q.shape == (257,) and q.dtype == np.float64 for q in mass)
    got = np.stack(mass)
    ratios = mr.worst_ratios(got, truth, states[:, 4])
    twin = mr.MassesTwin(bt.host_artifact(name)).masses(pars, states)
    allow = mr.allowance(truth, states[:, 4])
    with np.errstate(divide="ignore", invalid="ignore"):
        to_twin = np.where(got == twin, 0.0, np.abs(got - twin) / allow)
    print(f"{name}: worst |GPU - truth| / allowance {ratios}; worst |GPU - host twin| / allowance {dict(zip(mr.NAMES, to_twin.max(axis=1)))}")
    assert np.isfinite(got).all()
    assert max(ratios.values()) <= 1.0, (name, ratios)
    assert np.array_equal(np.sign(got[5]), np.sign(truth[:, 5]))
    # all eight are views of one (8, 257) array
    assert all(q.base is mass.V_TT.base for q in mass) and mass.V_TT.base.shape == (8, 257)
    kin = bg.kinematics(art, pars, states)
    assert np.array_equal(mass.eps_H, kin.eps_H) and np.array_equal(mass.omega, kin.omega)


def test_shapes_strides_and_parameter_rows(bg):
    """(5,), (65, 5) and (3, 22, 5) with three parameter rows; ld = 6 and ld = 8 host views read in place; a view without a uniform
    stride, made contiguous.  On ``skew``: three parameters, G_01 != 0."""
    name = "skew"
    art = bt.device_artifact(name)
    states, pars = kr.zoo_states(name)
    full = bg.masses(art, pars, states)
    part = bg.masses(art, pars[:65], states[:65])
    assert all(q.shape == (65,) for q in part) and _same(part, type(full)(*(q[:65] for q in full)))
    one = bg.masses(art, pars[7], states[7])
    assert all(q.shape == () for q in one) and all(float(u) == w[7] for u, w in zip(one, full))
    # (B, S) = (3, 22): trajectory b uses parameter row b
    traj = states[:66].reshape(3, 22, 5)
    got = bg.masses(art, pars[:3], traj)
    flat = bg.masses(art, np.repeat(pars[:3], 22, axis=0), states[:66])
    assert all(q.shape == (3, 22) for q in got) and _same(type(got)(*(q.reshape(66) for q in got)), flat)
    assert not np.array_equal(got.V_NN.reshape(66), full.V_NN[:66])  # (the rows matter: state k's own row gives something else)
    shared = bg.masses(art, pars[0], traj)  # one row for all
    assert np.array_equal(shared.V_NN[0], got.V_NN[0]) and not np.array_equal(shared.V_NN[1:], got.V_NN[1:])
    # ld = 6 and ld = 8: the gaps hold NaN and are not read
    for ld in (6, 8):
        wide = np.full((3, 22, ld), np.nan)
        wide[:, :, :5] = traj
        view = wide[:, :, :5]
        assert bg._state_stride(view.shape, tuple(s // 8 for s in view.strides)) == ld <= bg._HOST_MAX_LD
        assert _same(bg.masses(art, pars[:3], view), got)
    # no uniform stride at all (column-major), and a uniform one above the host path's bound: made contiguous first
    column_major = np.asfortranarray(states)
    assert bg._state_stride(column_major.shape, (1, 257)) is None
    assert _same(bg.masses(art, pars, column_major), full)
    assert _same(bg.masses(art, pars[::2], states[::2]), type(full)(*(q[::2] for q in full)))
    # a state at rest, and a component that is not finite
    edge = states[:3].copy()
    edge[1, 2:4] = 0.0
    edge[2, 1] = np.inf
    at = np.stack(bg.masses(art, pars[:3], edge))
    assert np.isfinite(at[:, 0]).all() and np.isnan(at[:, 2]).all()
    assert at[4, 1] == 0.0 and np.isfinite(at[3, 1]) and np.isnan(at[[0, 1, 2, 5, 6, 7], 1]).all()


def test_a_component_that_is_not_finite_gives_eight_nans_on_a_cyclic_coordinate(bg):
    """hyperbolic never reads theta: NaN or +-inf in any of the five components gives eight NaNs all the
    same, on the host path and on the device path; the finite state next to them gives finite numbers."""
    import torch

    from test_background_masses import _nonfinite_cases

    spec, art = workloads.artifact_for("hyperbolic")
    states = _nonfinite_cases((2.0, 0.3, 0.1, 0.2, 0.7))
    for got in (np.stack(bg.masses(art, spec.args, states)), torch.stack(tuple(bg.masses(art, spec.args, torch.from_numpy(states).cuda()))).cpu().numpy()):
        assert got.shape == (8, 16) and np.isfinite(got[:, 0]).all() and np.isnan(got[:, 1:]).all(), got
        assert abs(got[3, 0] + 2.0) <= _hyperbolic_ricci_allowance(2.0)  # L = 1


def test_device_path(bg):
    """``solve_eom_batch_device`` on the hyperbolic model, B = 65, 8 steps, the first eight lanes past the end of inflation at the
    start so that they stop at once: ``masses(sol.states)`` reads the (B, steps, 6) rows in place and returns GPU tensors equal to the
    host call on the copied rows bit for bit; the NaN rows after a stopped lane are NaN in all eight planes; the input is unchanged."""
    import torch

    spec, art = workloads.artifact_for("hyperbolic")
    x, v = _hyper_batch(65, seed=5)
    x[:8, 0], v[:8] = 1.05, 0.15  # near the minimum of V, where the velocity dominates: epsilon_H >= 1 at the start
    x[8:16, 0], v[8:16] = 3.5, 0.01  # far up the potential and slow: these run through all rows
    sol = bg.solve_eom_batch_device(art, spec.args, 8, x, v, substeps=4, stop_at_end=True)
    assert sol.states.shape == (65, 8, 5) and sol.states.stride() == (48, 6, 1)
    assert bg._state_stride(tuple(sol.states.shape), tuple(sol.states.stride())) == 6
    before = sol.states.clone()
    mass = bg.masses(art, spec.args, sol.states)
    assert isinstance(mass, bg.Masses)
    for q in mass:
        assert isinstance(q, torch.Tensor) and q.is_cuda and q.dtype == torch.float64 and q.shape == (65, 8)
    assert len({q.untyped_storage().data_ptr() for q in mass}) == 1  # views of one (8, 65, 8) tensor
    rows = sol.states.cpu().numpy()
    want = bg.masses(art, spec.args, rows)
    assert _same(_host(mass), want)
    stopped = np.arange(8)[None, :] > sol.last_row[:, None]
    assert np.array_equal(np.isnan(rows).all(axis=2), stopped) and np.array_equal(np.isnan(rows).any(axis=2), stopped)
    assert stopped[:8, 1:].all() and not stopped[:, 0].any() and (~stopped).all(axis=1).any()
    for q in want:
        assert np.array_equal(np.isnan(q), stopped)
    # per-trajectory parameter rows on the device path: B rows, each the shared one
    assert _same(_host(bg.masses(art, np.tile(spec.args, (65, 1)), sol.states)), want)
    # a tensor that is not a uniform view is made contiguous first
    assert _same(_host(bg.masses(art, spec.args, sol.states[:, ::2])), type(want)(*(q[:, ::2] for q in want)))
    torch.cuda.synchronize()
    assert torch.equal(sol.states.nan_to_num(nan=-7.0), before.nan_to_num(nan=-7.0))
    empty = bg.masses(art, spec.args, sol.states[:0])
    assert len(empty) == 8 and all(q.shape == (0, 8) and q.is_cuda for q in empty)
    with pytest.raises(ValueError):
        bg.masses(art, spec.args, sol.states.float())
    # the library checks the bytes the tensor's storage really holds
    from inflatox_amd import _native

    lib, flat = bg._dylib(art, background=False), before.reshape(-1, 5)
    out = torch.empty((8, flat.shape[0]), dtype=torch.float64, device=flat.device)
    with pytest.raises(_native.InflatoxShapeError, match="state buffer"):
        lib.masses_device(spec.args, flat.data_ptr(), flat.numel() * 8 - 8, flat.shape[0], 5, 1, out.data_ptr(), out.numel() * 8)
    with pytest.raises(_native.InflatoxShapeError, match="output buffer"):
        lib.masses_device(spec.args, flat.data_ptr(), flat.numel() * 8, flat.shape[0], 5, 1, out.data_ptr(), out.numel() * 8 - 8)


def test_chunks_of_a_large_host_call(bg):
    """n = 2^20 + 65 hyperbolic states in one host call (two chunks: 2^20 and 65) with a parameter row per state equals two calls on
    the halves bit for bit: the second chunk finds its states, its parameter rows (``first``) and its place in the planes."""
    spec, art = workloads.artifact_for("hyperbolic")
    n = (1 << 20) + 65
    rng = np.random.default_rng(21)
    big = np.concatenate([rng.uniform(1.5, 4.0, (n, 1)), rng.uniform(-1.0, 1.0, (n, 1)), rng.uniform(-0.2, 0.2, (n, 2)), rng.uniform(0.5, 1.5, (n, 1))], axis=1)
    pars = spec.args[None, :] * rng.uniform(0.9, 1.1, (n, spec.args.size))
    whole = bg.masses(art, pars, big)
    half = n // 2
    first, second = bg.masses(art, pars[:half], big[:half]), bg.masses(art, pars[half:], big[half:])
    assert _same(whole, type(whole)(*(np.concatenate([a, b]) for a, b in zip(first, second))))
    assert np.isfinite(np.stack(whole)).all() and len(np.unique(whole.M_eff2[-65:])) == 65
    # the states of the second chunk against a small call of their own
    assert _same(type(whole)(*(q[-65:] for q in whole)), bg.masses(art, pars[-65:], big[-65:]))


def test_mass_map(bg):
    """An 8 x 8 hyperbolic grid with N_star = 1: ``mass_map`` is ``horizon_exit_map`` followed by ``masses``, NaN exactly where the
    exit state is."""
    spec, art = workloads.artifact_for("hyperbolic")
    ss = np.array([[1.0, 5.0], [-1.0, 1.0]])
    kw = dict(N_star=1.0, max_steps=20_000, max_err=1e-9)
    mass, state, n_end, status = bg.mass_map(art, spec.args, ss, 8, 8, return_status=True, **kw)
    want_state, want_end, want_status = bg.horizon_exit_map(art, spec.args, ss, 8, 8, return_status=True, **kw)
    assert np.array_equal(state, want_state, equal_nan=True) and np.array_equal(n_end, want_end, equal_nan=True) and np.array_equal(status, want_status)
    assert _same(mass, bg.masses(art, spec.args, want_state))
    missing = np.isnan(state).any(axis=2)
    assert missing.any() and (~missing).any()
    for q in mass:
        assert q.shape == (8, 8) and np.array_equal(np.isnan(q), missing)
    triple = bg.mass_map(art, spec.args, ss, 8, 8, **kw)
    assert len(triple) == 3 and _same(triple[0], mass)
    assert np.all(np.abs(mass.ricci[~missing] + 2.0) <= _hyperbolic_ricci_allowance(state[~missing][:, 0]))  # L = 1


def test_doc_model_along_the_gradient_is_calc_H(bg):
    """The doc model at the 16 gradient-aligned states of tests/masses_reference.py: V_TT = v00, V_NN = v11 and |V_TN| = |v10| of
    ``GeneralisedAL.calc_H`` at the same points, within what tests/tolerance.py grants the doc model's Hesse planes (1e-10 of the
    value plus KAPPA times the reference's own measured rounding error there)."""
    import tolerance as tol
    from inflatox_amd.consistency_conditions import GeneralisedAL

    spec, art = workloads.artifact_for("doc")
    states, pts = mr.doc_gradient_states()
    mass = bg.masses(art, spec.args, states)
    al = GeneralisedAL(art)
    hesse = np.array([al.calc_H(pt, spec.args) for pt in pts])  # (16, 2, 2)
    env, _flaky = tol.reference_error("doc", spec.args, pts)
    want = np.stack([np.zeros(16), hesse[:, 0, 0], hesse[:, 1, 0], hesse[:, 1, 1], np.zeros(16)], axis=1)
    allowed = tol.allowance_raw(want, env, "doc")
    assert np.isfinite(allowed[:, 1:4]).all() and np.isfinite(hesse).all()
    err = np.stack([np.abs(mass.V_TT - want[:, 1]), np.abs(np.abs(mass.V_TN) - np.abs(want[:, 2])), np.abs(mass.V_NN - want[:, 3])], axis=1)
    print(f"doc: worst |masses - calc_H| / allowance {(err / allowed[:, 1:4]).max(axis=0)}")
    assert np.all(err <= allowed[:, 1:4]), (err / allowed[:, 1:4]).max(axis=0)
    assert np.all(np.abs(want[:, 2]) > 1e-3)  # (v10 is there to be seen)


def test_masses_object_of_another_layout_is_refused(bg):
    """An object built with -DINFLX_MASS_ABI_VERSION=2 is refused with INFLX_ERR_VERSION, a missing one is INFLX_ERR_SYMBOL with the
    way to build it; the kinematics object of the same artefact is untouched by all this."""
    from background_reference import power_law_artifact, power_law_init
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".masses"
    headers = {stale + ".model.h": header_text, stale + ".eom.h": art.eom_header_text(), stale + ".kin.h": art.kinematics_header_text(),
               stale + ".mass.h": art.masses_header_text()}  # fmt: skip
    state = np.array([[*power_law_init(), 8.0]])
    p = np.ascontiguousarray(p, dtype=np.float64)
    out = np.empty((8, 1))
    dp = C.POINTER(C.c_double)

    def raw(lib):  # the C entry point's own return code
        return lib._lib.inflx_masses(lib._h, p.ctypes.data_as(dp), 1, lib.n_parameters, state.ctypes.data_as(dp), 1, 5, 1, out.ctypes.data_as(dp))

    try:
        if os.path.exists(stale):
            os.remove(stale)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        assert raw(lib) == _native.ERR_SYMBOL
        with pytest.raises(SystemError, match=r"ensure_masses\(\)") as err:
            lib.masses(p, state, 1, 5)
        assert ".masses exists" in str(err.value)
        for path, text in headers.items():
            with open(path, "w") as fh:
                fh.write(text)
        hdr, eom_hdr, kin_hdr, mass_hdr = headers
        cmd = [hipcc_path(), *options, "-DINFLX_MASS_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_KIN_HEADER="{kin_hdr}"', f'-DINFLX_MASS_HEADER="{mass_hdr}"',
               os.path.join(_CSRC, "inflx_masses_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        assert raw(lib) == _native.ERR_VERSION
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.masses(p, state, 1, 5)
        assert "INFLX_MASS_ABI 2, expected 1" in str(err.value)
        # the kinematics object is another file with another layout word: it loads and works on the same handle
        art.ensure_kinematics()
        assert np.isfinite(lib.kinematics(p, state, 1, 5)).all()
        # ... and the artefact's own build replaces the refused file and works on the same handle
        os.remove(stale)
        art.ensure_masses()
        got = lib.masses(p, state, 1, 5)
        assert got.shape == (8, 1) and np.isfinite(got).all()
        lib.close()
    finally:
        for path in (stale, art.shared_object_path + ".kinematics", *headers):
            if os.path.exists(path):
                os.remove(path)
