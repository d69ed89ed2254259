"""Trajectory kinematics on the GPU (inflatox_amd.background.kinematics, turn_rate_map): the kernel against the 40-digit truth of
tests/kinematics_reference.py on fuzzed curved field spaces and metrics with G_01 != 0, the shapes and strides of the states, the
device-resident path and its stream ordering, epsilon_H against the sampled solver's own, the chunks of a large host call,
``turn_rate_map`` against its two halves, and the refusal of a kinematics object of another layout.  States, truth and bounds are
those tests/test_background_kinematics.py establishes on the host build."""

import os
import struct
import subprocess

import numpy as np
import pytest

import background_truth as bt
import kinematics_reference as kr
import workloads
from test_background_gpu import _hyper_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper_states(bg):
    """(artefact, parameter row, states (257, 5)) of the hyperbolic model: initial states with H from the solver's own row 0"""
    spec, art = workloads.artifact_for("hyperbolic")
    x, v = _hyper_batch(257, seed=3)
    sol = bg.solve_eom_batch(art, spec.args, 1, x, v)
    states = np.ascontiguousarray(sol.states[:, 0])
    assert np.isfinite(states).all()
    return art, spec.args, states


def _same(a, b):
    """two Kinematics of numpy arrays: the same shapes and the same values, NaN where NaN"""
    return all(u.shape == w.shape and np.array_equal(u, w, equal_nan=True) for u, w in zip(a, b))


def _host(kin):
    return type(kin)(*(q.cpu().numpy() for q in kin))


@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_kernel_against_truth(bg, name):
    """257 states (a 256-lane workgroup and one lane), one parameter row each (traj_len = 1, ld = 5): every quantity within the
    allowance of the 40-digit truth; the difference to the host twin is recorded.  Measured: profiles/background_kinematics.json."""
    art = bt.device_artifact(name)
    states, pars = kr.zoo_states(name)
    truth = kr.zoo_truth(name, 257)
    kin = bg.kinematics(art, pars, states)
    assert isinstance(kin, bg.Kinematics) and all(q.shape == (257,) and q.dtype == np.float64 for q in kin)
    got = np.stack(kin)
    ratios = kr.worst_ratios(got, truth, states[:, 4])
    twin = kr.KinematicsTwin(bt.host_artifact(name)).kinematics(pars, states)
    to_twin = np.abs(got - twin) / kr.allowance(truth, states[:, 4])
    print(f"{name}: worst |GPU - truth| / allowance {ratios}; worst |GPU - host twin| / allowance {dict(zip(kr.NAMES, to_twin.max(axis=1)))}")
    assert np.isfinite(got).all()
    assert max(ratios.values()) <= 1.0, (name, ratios)
    assert np.array_equal(np.sign(got[2]), np.sign(truth[:, 2]))
    # all six are views of one (6, 257) array
    assert all(q.base is kin.eps_H.base for q in kin) and kin.eps_H.base.shape == (6, 257)


def test_shapes_strides_and_parameter_rows(bg):
    """n in {0, 1, 255, 256, 257}; ld = 6 with a sixth column of NaN; (B, S) = (3, 5) with three parameter rows against the flat call
    with each row repeated five times; one state (5,); NaN tail rows give NaN exactly there.  On ``skew``: three parameters, G_01 != 0."""
    name = "skew"
    art = bt.device_artifact(name)
    states, pars = kr.zoo_states(name)
    full = bg.kinematics(art, pars, states)
    for n in (0, 1, 255, 256, 257):
        part = bg.kinematics(art, pars[:n], states[:n])
        assert _same(part, type(full)(*(q[:n] for q in full))), n
        shared = bg.kinematics(art, pars[0], states[:n])  # one row for all
        assert all(q.shape == (n,) for q in shared)
        if n:
            assert shared.omega[0] == full.omega[0]
        if n > 1:  # (the rows matter: another state's row gives something else)
            assert not np.array_equal(shared.omega[1:], full.omega[1:n])
    wide = np.concatenate([states, np.full((257, 1), np.nan)], axis=1)
    view = wide[:, :5]
    assert bg._state_stride(view.shape, tuple(s // 8 for s in view.strides)) == 6  # read in place, 48 bytes between states
    assert _same(bg.kinematics(art, pars, view), full)
    assert np.isnan(wide[:, 5]).all() and np.array_equal(wide[:, :5], states)
    # (B, S) = (3, 5): trajectory b uses parameter row b
    traj = states[:15].reshape(3, 5, 5)
    got = bg.kinematics(art, pars[:3], traj)
    flat = bg.kinematics(art, np.repeat(pars[:3], 5, axis=0), states[:15])
    assert all(q.shape == (3, 5) for q in got) and _same(type(got)(*(q.reshape(15) for q in got)), flat)
    assert not np.array_equal(got.omega.reshape(15), full.omega[:15])  # (the rows matter: lane k's own row gives something else)
    # ... also as a strided view of (3, 5, 6) rows, the solver's layout
    rows6 = np.full((3, 5, 6), np.nan)
    rows6[:, :, :5] = traj
    assert _same(bg.kinematics(art, pars[:3], rows6[:, :, :5]), got)
    # what the host path does not read in place is made contiguous first: every second state (a uniform stride of 10 doubles, above
    # the host path's bound: the gaps would be uploaded) and a column-major array (no uniform stride at all: the last stride is 257)
    assert bg._state_stride(states[::2].shape, tuple(s // 8 for s in states[::2].strides)) == 10 > bg._HOST_MAX_LD
    assert _same(bg.kinematics(art, pars[::2], states[::2]), type(full)(*(q[::2] for q in full)))
    column_major = np.asfortranarray(states)
    assert column_major.strides == (8, 257 * 8) and bg._state_stride(column_major.shape, (1, 257)) is None
    assert _same(bg.kinematics(art, pars, column_major), full)
    first_rows = np.full((257, 40, 6), np.nan)  # sol.states[:, 0] of (B, steps, 6) rows: 240 doubles between states
    first_rows[:, 0, :5] = states
    assert _same(bg.kinematics(art, pars, first_rows[:, 0, :5]), full)
    one = bg.kinematics(art, pars[7], states[7])
    assert all(q.shape == () for q in one) and all(float(u) == w[7] for u, w in zip(one, full))
    # a trajectory whose tail rows are NaN: NaN exactly there
    tail = traj.copy()
    tail[1, 3:] = np.nan
    tail[2, 4, 4] = np.nan  # H alone
    got_tail = bg.kinematics(art, pars[:3], tail)
    want_nan = np.zeros((3, 5), dtype=bool)
    want_nan[1, 3:] = True
    want_nan[2, 4] = True
    for q, ref in zip(got_tail, got):
        assert np.array_equal(np.isnan(q), want_nan) and np.array_equal(q[~want_nan], ref[~want_nan])
    # a state at rest
    rest = states[:2].copy()
    rest[1, 2:4] = 0.0
    at_rest = bg.kinematics(art, pars[:2], rest)
    assert at_rest.eps_H[1] == 0.0 and at_rest.sigma_dot[1] == 0.0 and all(np.isnan(q[1]) for q in (at_rest.eta_par, at_rest.omega, at_rest.V_sigma, at_rest.V_N))
    assert all(np.isfinite(q[0]) for q in at_rest)


def test_a_component_that_is_not_finite_gives_six_nans_on_a_cyclic_coordinate(bg):
    """hyperbolic never reads theta, and three of the quantities do not divide by H: NaN or +-inf in any of the five components gives
    six NaNs all the same, on the host path and on the device path; the finite state next to them gives finite numbers."""
    import torch

    from test_background_kinematics import _nonfinite_cases

    spec, art = workloads.artifact_for("hyperbolic")
    states = _nonfinite_cases((2.0, 0.3, 0.1, 0.2, 0.7))
    for got in (np.stack(bg.kinematics(art, spec.args, states)), torch.stack(tuple(bg.kinematics(art, spec.args, torch.from_numpy(states).cuda()))).cpu().numpy()):
        assert got.shape == (6, 16) and np.isfinite(got[:, 0]).all() and np.isnan(got[:, 1:]).all(), got
    # the same state with another theta: the same bits (the coordinate is cyclic)
    other = states[:1].copy()
    other[0, 1] = -1.7
    assert _same(bg.kinematics(art, spec.args, other), bg.kinematics(art, spec.args, states[:1]))


def test_device_path(bg):
    """``solve_eom_batch_device`` on the hyperbolic model, B = 130, steps = 9, substeps = 4: ``kinematics(sol.states)`` reads the
    (B, steps, 6) rows in place and returns GPU tensors equal to the host path on ``sol.states.cpu()`` bit for bit -- also under a
    non-default current stream, with a reduction enqueued right behind the call and no synchronise --; the input is unchanged."""
    import torch

    spec, art = workloads.artifact_for("hyperbolic")
    x, v = _hyper_batch(130, seed=5)
    sol = bg.solve_eom_batch_device(art, spec.args, 9, x, v, substeps=4)
    assert sol.states.shape == (130, 9, 5) and sol.states.stride() == (54, 6, 1)
    assert bg._state_stride(tuple(sol.states.shape), tuple(sol.states.stride())) == 6
    before = sol.states.clone()
    rows_before = sol.N.clone()
    kin = bg.kinematics(art, spec.args, sol.states)
    assert isinstance(kin, bg.Kinematics)
    for q in kin:
        assert isinstance(q, torch.Tensor) and q.is_cuda and q.dtype == torch.float64 and q.shape == (130, 9)
    assert len({q.untyped_storage().data_ptr() for q in kin}) == 1  # views of one (6, 130, 9) tensor
    want = bg.kinematics(art, spec.args, sol.states.cpu().numpy())
    assert _same(_host(kin), want)
    assert np.isfinite(want.eps_H).all() and (want.eps_H > 0).all()
    # per-trajectory parameter rows on the device path: B rows, each the shared one
    assert _same(_host(bg.kinematics(art, np.tile(spec.args, (130, 1)), sol.states)), want)
    # a non-default current stream: the call is ordered after what that stream has enqueued, and the stream after the call
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        shifted = sol.states * 1.0  # produced on `stream`, consumed by the call
        kin2 = bg.kinematics(art, spec.args, shifted)
        total = torch.nansum(kin2.omega) + torch.nansum(kin2.eta_par)
    stream.synchronize()
    assert _same(_host(kin2), want)
    assert total.item() == (torch.nansum(kin.omega) + torch.nansum(kin.eta_par)).item()
    # a tensor that is not a uniform view is made contiguous first; the result is the same states' result
    odd = bg.kinematics(art, spec.args, sol.states[:, ::2])
    assert _same(_host(odd), type(want)(*(q[:, ::2] for q in want)))
    torch.cuda.synchronize()
    assert torch.equal(sol.states, before) and torch.equal(sol.N, rows_before)
    empty = bg.kinematics(art, spec.args, sol.states[:0])
    assert all(q.shape == (0, 9) and q.is_cuda for q in empty)
    with pytest.raises(ValueError):
        bg.kinematics(art, spec.args, sol.states.float())
    # the library checks the bytes the tensor's storage really holds
    from inflatox_amd import _native

    lib, flat = bg._dylib(art, background=False), before.reshape(-1, 5)
    out = torch.empty((6, flat.shape[0]), dtype=torch.float64, device=flat.device)
    with pytest.raises(_native.InflatoxShapeError, match="state buffer"):
        lib.kinematics_device(spec.args, flat.data_ptr(), flat.numel() * 8 - 8, flat.shape[0], 5, 1, out.data_ptr(), out.numel() * 8)
    with pytest.raises(_native.InflatoxShapeError, match="output buffer"):
        lib.kinematics_device(spec.args, flat.data_ptr(), flat.numel() * 8, flat.shape[0], 5, 1, out.data_ptr(), out.numel() * 8 - 8)


def test_epsilon_h_equals_the_sampled_solvers(bg):
    """``solve_eom_sampled``, B = 65, samples = linspace(0, 2, 9): epsilon_H of ``kinematics`` at the emitted states is the solver's
    own epsilon_H bit for bit, and NaN exactly where that is (the samples a trajectory did not reach)."""
    spec, art = workloads.artifact_for("hyperbolic")
    x, v = _hyper_batch(65, seed=9)
    x[:8, 0] = 1.05  # near the minimum of V, where the velocity dominates: these are past the end of inflation at the start
    x[8:16, 0], v[8:16] = 5.5, 0.01  # far up the potential and slow: these reach N = 2
    at = bg.solve_eom_sampled(art, spec.args, np.linspace(0.0, 2.0, 9), x, v)
    kin = bg.kinematics(art, spec.args, at.states)
    assert kin.eps_H.shape == (65, 9)
    emitted = np.arange(9)[None, :] < at.n_stored[:, None]
    assert np.array_equal(np.isnan(at.eps_H), ~emitted) and emitted.any() and (~emitted).any() and emitted.all(axis=1).any()
    assert np.array_equal(np.isnan(kin.eps_H), ~emitted)
    assert np.array_equal(kin.eps_H[emitted], at.eps_H[emitted])
    for q in kin:
        assert np.array_equal(np.isnan(q), ~emitted)


def test_chunks_of_a_large_host_call(bg, hyper_states):
    """n = 2^20 + 257 states in one host call (two chunks: 2^20 and 257) with a parameter row per state equals two calls on the
    halves bit for bit: the second chunk finds its states, its parameter rows and its place in the planes."""
    art, p, states = hyper_states
    n = (1 << 20) + 257
    rng = np.random.default_rng(21)
    big = states[rng.integers(0, 257, n)] * rng.uniform(0.9, 1.1, (n, 5))
    pars = p[None, :] * rng.uniform(0.9, 1.1, (n, p.size))
    whole = bg.kinematics(art, pars, big)
    half = n // 2
    first, second = bg.kinematics(art, pars[:half], big[:half]), bg.kinematics(art, pars[half:], big[half:])
    assert _same(whole, type(whole)(*(np.concatenate([a, b]) for a, b in zip(first, second))))
    assert np.isfinite(whole.omega).all() and len(np.unique(whole.omega[-300:])) == 300
    # the last states against a small call of their own
    assert _same(type(whole)(*(q[-257:] for q in whole)), bg.kinematics(art, pars[-257:], big[-257:]))


def test_turn_rate_map(bg):
    """An 8 x 8 hyperbolic grid with N_star = 1: ``turn_rate_map`` is ``horizon_exit_map`` followed by ``kinematics``, NaN exactly
    where the exit state is."""
    spec, art = workloads.artifact_for("hyperbolic")
    ss = np.array([[1.0, 5.0], [-1.0, 1.0]])
    kw = dict(N_star=1.0, max_steps=20_000, max_err=1e-9)
    kin, state, n_end, status = bg.turn_rate_map(art, spec.args, ss, 8, 8, return_status=True, **kw)
    want_state, want_end, want_status = bg.horizon_exit_map(art, spec.args, ss, 8, 8, return_status=True, **kw)
    assert np.array_equal(state, want_state, equal_nan=True) and np.array_equal(n_end, want_end, equal_nan=True) and np.array_equal(status, want_status)
    assert _same(kin, bg.kinematics(art, spec.args, want_state))
    missing = np.isnan(state).any(axis=2)
    assert missing.any() and (~missing).any() and np.array_equal(missing, status != bg.TARGET)
    for q in kin:
        assert q.shape == (8, 8) and np.array_equal(np.isnan(q), missing)
    triple = bg.turn_rate_map(art, spec.args, ss, 8, 8, **kw)
    assert len(triple) == 3 and _same(triple[0], kin)
    # one e-fold before the end of inflation the field rolls: 0 < eps_H < 1
    assert np.all((kin.eps_H[~missing] > 0) & (kin.eps_H[~missing] < 1))


def test_kinematics_object_of_another_layout_is_refused(bg):
    """An object built with -DINFLX_KIN_ABI_VERSION=0 is refused (INFLX_ERR_VERSION), a missing one is INFLX_ERR_SYMBOL with the way
    to build it; the background object of the same artefact still loads and reports layout 5."""
    from background_reference import power_law_artifact, power_law_init
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path
    from test_background_rows import _elf_symbols

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".kinematics"
    headers = {stale + ".model.h": header_text, stale + ".eom.h": art.eom_header_text(), stale + ".kin.h": art.kinematics_header_text()}
    state = np.array([[*power_law_init(), 8.0]])
    try:
        lib = _native.InflatoxDevLib(art.shared_object_path)
        assert not os.path.exists(stale)
        with pytest.raises(SystemError, match=r"ensure_kinematics\(\)") as err:
            lib.kinematics(p, state, 1, 5)
        assert ".kinematics exists" in str(err.value)
        for path, text in headers.items():
            with open(path, "w") as fh:
                fh.write(text)
        hdr, eom_hdr, kin_hdr = headers
        cmd = [hipcc_path(), *options, "-DINFLX_KIN_ABI_VERSION=0", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', f'-DINFLX_KIN_HEADER="{kin_hdr}"', os.path.join(_CSRC, "inflx_kinematics_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.kinematics(p, state, 1, 5)
        assert "INFLX_KIN_ABI 0, expected 1" in str(err.value)
        # the background object is untouched by all this
        data, sections, symbols = _elf_symbols(art.ensure_background())
        value, _size, shndx = symbols["INFLX_BG_ABI"]
        assert struct.unpack_from("<I", data, sections[shndx][4] + value - sections[shndx][3])[0] == 5
        out = lib.solve_eom(p, state[:, :4], 3, 1, _native.EOM_RKF, 1e-6, 0.0, 0)
        assert np.isfinite(out[0]).all()
        # ... and the artefact's own build replaces the refused file and works on the same handle
        os.remove(stale)
        art.ensure_kinematics()
        got = lib.kinematics(p, state, 1, 5)
        assert got.shape == (6, 1) and np.isfinite(got).all()
        lib.close()
    finally:
        for path in (stale, *headers):
            if os.path.exists(path):
                os.remove(path)
