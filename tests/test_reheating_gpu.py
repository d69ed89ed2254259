"""Reheating on the GPU (inflatox_amd.reheating): lanes that stop in different launches against the host build of the same code, adaptive
runs against the independent truth with the host build's bound, fourth order without the event, lane independence and lane chunks, the
maps against their halves, the heavy-register models and the refusal of an object of another layout."""

import os
import subprocess

import numpy as np
import pytest

import background_truth as bt
import reheating_reference as rr
import workloads
from background_reference import COMPLETE, ENDED, power_law_artifact, power_law_init
from background_sampled_reference import EGNO_SEEDS
from reheating_reference import REHEATED, ReheatingTwin
from test_background import initial_state
from test_background_gpu import RESTATEMENT_TOL, _hyper_batch
from test_reheating import LOCATED_BOUND, METHODS, ORDER_MODELS, RETURNED_COMPONENTS, order_conditions, order_gammas

pytestmark = pytest.mark.gpu

FIELDS = ("state", "rho_r", "N_reh", "t_reh", "H_start", "w_reh", "A_shift", "omega_r", "status")


@pytest.fixture(scope="module")
def rh():
    from inflatox_amd import reheating

    return reheating


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper():
    art, p, _rhs = rr.hyper_case()
    return p, art


def _planes(reh):
    """(B, 8): y[0..4], N, rho_r, t -- the twin's layout; N is the twin's for a REHEATED lane only (every other lane returns NaN there)"""
    return np.concatenate([reh.state, reh.N_reh[:, None], reh.rho_r[:, None], reh.t_reh[:, None]], axis=1)


def _same(a, b, rows=slice(None)):
    return all(np.array_equal(getattr(a, f)[rows], getattr(b, f), equal_nan=True) for f in FIELDS)


def _against_the_twin(reh, twin, p, init, gamma, max_steps, **kw):
    """Every lane against the host build of the same code: the same status, H_start and every value of the returned state relative to
    its scale (its magnitude with a floor of 1e-3).  Returns every lane's worst figure and the twin's accepted steps."""
    got = _planes(reh)
    worst, accepted = [], []
    for k in range(init.shape[0]):
        want, meta = twin.solve(p if np.ndim(p) == 1 else p[k], init[k], gamma[k], max_steps, **kw)
        assert reh.status[k] == meta["status"], (k, reh.status[k], meta)
        cols = slice(None) if meta["status"] == REHEATED else [0, 1, 2, 3, 4, 6, 7]
        assert np.isfinite(got[k, cols]).all() and (meta["status"] == REHEATED or np.isnan(got[k, 5]))
        worst.append(max(float(np.max(np.abs(got[k, cols] - want[cols]) / np.maximum(np.abs(want[cols]), 1e-3))), abs(reh.H_start[k] / meta["H0"] - 1.0)))
        accepted.append(meta["accepted"])
    return np.array(worst), np.array(accepted)


def test_launch_boundaries(rh, hyper):
    """B = 96 (a wavefront and a half) from the hyperbolic end states, Gamma = 0.2 and 1.0 alternating, dt = 0.01: between 353 and
    3055 accepted steps, so the lanes stop in different launches of 256 steps.  Against the host build (contraction off), which
    differs by FMA contraction only: the same status per lane, values within RESTATEMENT_TOL["hyperbolic"] = 1e-12 of their scale.
    The reheating object is built without FMA contraction (csrc/inflx_reheating_kernels.hip) for this: measured on the MI355X 6.0e-16
    with rk4 and 5.1e-14 with rkf.  Built with the core object's -ffp-contract=on it was 4.8e-12 and 1.25e-11, the figure of one lane
    (Gamma = 0.2, 2481 steps) whose located chi^phi = 0.0024 lies next to a zero of the oscillating velocity; the host build with and
    without contraction differs by 3.4e-12 and 1.1e-11 on that same lane."""
    p, art = hyper
    twin = ReheatingTwin(art)
    ends = rr.hyper_end_states(96)
    gamma = np.where(np.arange(96) % 2 == 0, *rr.HYPER_GAMMAS)
    tol = RESTATEMENT_TOL["hyperbolic"]
    figures = {}
    for solver in METHODS:
        reh = rh.reheating(art, p, gamma, ends[:, :2], ends[:, 2:], max_steps=20_000, solver=solver, dt=0.01)
        assert reh.state.shape == (96, 5) and all(getattr(reh, f).shape == (96,) for f in FIELDS[1:]) and reh.status.dtype == np.int8
        worst, accepted = _against_the_twin(reh, twin, p, ends, gamma, 20_000, method=solver, dt=0.01)
        print(f"{solver}: GPU vs host build at dt = 0.01, max relative difference {worst.max():.3e} (lane {worst.argmax()}, {accepted[worst.argmax()]} steps; "
              f"{(worst > tol).sum()} of 96 lanes above {tol:.0e}); accepted steps {accepted.min()} .. {accepted.max()}")
        assert np.all(reh.status == REHEATED) and len(set(accepted // 256)) >= 4
        figures[solver] = float(worst.max())
    assert max(figures.values()) <= tol, figures


@pytest.mark.parametrize("solver", METHODS)
def test_adaptive_runs_against_the_truth(rh, hyper, solver):
    """The lanes of the CPU test (a), adaptive at max_err = 1e-9: every lane REHEATED, and N_reh, ln H_reh and the state within the bound
    the host build set (tests/test_reheating.py LOCATED_BOUND, twice its own worst error)."""
    p, art = hyper
    ends = rr.hyper_end_states()
    worst = 0.0
    for gamma in rr.HYPER_GAMMAS:
        reh = rh.reheating(art, p, gamma, ends[:, :2], ends[:, 2:], omega_r=rr.HYPER_OMEGA, max_err=1e-9, solver=solver)
        assert np.all(reh.status == REHEATED), np.bincount(reh.status)
        got = _planes(reh)
        worst = max(worst, max(rr.located_error(got[k], tr) for k, tr in enumerate(rr.hyper_truths(gamma))))
    print(f"hyperbolic {solver}: located states against the truth, worst {worst:.3e} (bound {LOCATED_BOUND['hyperbolic', solver]:.1e})")
    assert worst <= LOCATED_BOUND["hyperbolic", solver]
    init, pars = (a[: rr.LANES] for a in bt.batch(rr.FUZZ_NAME))
    reh = rh.reheating(bt.device_artifact(rr.FUZZ_NAME), pars, rr.FUZZ_GAMMA, init[:, :2], init[:, 2:], omega_r=rr.FUZZ_OMEGA, max_err=1e-9, solver=solver)
    assert np.all(reh.status == REHEATED), np.bincount(reh.status)
    got = _planes(reh)
    worst = max(rr.located_error(got[k], tr) for k, tr in enumerate(rr.fuzz_truths()))
    print(f"fuzz4 {solver}: located states against the truth, worst {worst:.3e} (bound {LOCATED_BOUND['fuzz4', solver]:.1e})")
    assert worst <= LOCATED_BOUND["fuzz4", solver]
    assert np.max(np.abs(reh.omega_r - rr.FUZZ_OMEGA)) <= 1e-12 and np.all(reh.N_reh > 0.0)


@pytest.mark.parametrize("name", ORDER_MODELS)
def test_fourth_order_without_the_event(rh, name):
    """The CPU test (b) on the device: fixed dt to T = 1 with a decay rate per lane, every lane COMPLETE, and the three conditions of
    ``background_truth.BATCH_DRAW`` lane by lane."""
    art = bt.device_artifact(name)
    init, pars = (a[: rr.LANES] for a in bt.batch(name))
    gam = order_gammas(name)
    for solver in METHODS:

        def solve(n):
            reh = rh.reheating(art, pars, gam, init[:, :2], init[:, 2:], max_steps=n, solver=solver, dt=bt.T_ORDER / n)
            assert np.all(reh.status == COMPLETE) and np.isnan(reh.N_reh).all() and np.allclose(reh.t_reh, bt.T_ORDER, rtol=1e-13)
            return reh

        # (a COMPLETE lane does not return its N: the conditions are taken over the fields, the velocities, H and rho_r, on which the
        # host test asserts them as well)
        err, ratio, h_min = order_conditions(lambda n: _planes(solve(n)), name, cols=RETURNED_COMPONENTS)
        print(f"{name} {solver}: error at n = 40 in [{err.min():.3e}, {err.max():.3e}], ratio in [{ratio.min():.2f}, {ratio.max():.2f}], H >= {h_min:.3f}")
        assert err.min() > 1.2e-10 and ratio.min() >= 14.5 and h_min > 0.05


def test_lane_independence_and_lane_chunks(rh, hyper):
    """B = 257: lane k equals the lane run alone, bit for bit, adaptive and with Gamma per lane.  A mixed batch -- Gamma = 0 lanes that
    run out of steps, lanes whose radiation dominates at the start, ordinary lanes -- leaves every lane with its own status and the
    values it has alone.  B = 2^20 + 5 takes two passes (the carry of a pass holds 2^20 lanes at most): the second pass's five lanes, and
    lanes on both sides of the seam, equal calls of their own."""
    p, art = hyper
    x, v = _hyper_batch(257, seed=4)
    gamma = np.random.default_rng(9).uniform(0.2, 1.0, 257)
    big = rh.reheating(art, p, gamma, x, v, max_steps=60, omega_r=0.3)
    assert (big.status == REHEATED).sum() > 64 and (big.status == COMPLETE).sum() > 64, np.bincount(big.status)  # (the lanes reheat after 26 .. 123 steps)
    for k in (0, 63, 64, 200, 255, 256):
        alone = rh.reheating(art, p, gamma[k : k + 1], x[k : k + 1], v[k : k + 1], max_steps=60, omega_r=0.3)
        assert _same(big, alone, slice(k, k + 1)), k
    kind = np.arange(257) % 3
    gamma3 = np.where(kind == 0, 0.0, gamma)
    rho3 = np.where(kind == 1, 50.0, 0.0)
    mixed = rh.reheating(art, p, gamma3, x, v, rho_r_init=rho3, max_steps=60, omega_r=0.3)
    assert np.all(mixed.status[kind == 0] == COMPLETE) and np.all(mixed.status[kind == 1] == REHEATED) and np.all(mixed.N_reh[kind == 1] == 0.0)
    assert np.isnan(mixed.w_reh[kind != 2]).all() and np.all(mixed.A_shift[kind == 1] == 0.0) and np.all(mixed.rho_r[kind == 0] == 0.0)
    assert (mixed.status[kind == 2] == REHEATED).sum() > 16 and np.isfinite(mixed.state).all()
    for k in range(0, 257, 16):
        alone = rh.reheating(art, p, gamma3[k : k + 1], x[k : k + 1], v[k : k + 1], rho_r_init=rho3[k : k + 1], max_steps=60, omega_r=0.3)
        assert _same(mixed, alone, slice(k, k + 1)), k
    B = (1 << 20) + 5
    xb, vb = _hyper_batch(B, seed=8)
    gb = np.random.default_rng(10).uniform(0.0, 1.0, B)
    kw = dict(max_steps=3, solver="rkf", dt=1e-2, rho_r_init=np.where(np.arange(B) % 7 == 0, 100.0, 0.0), omega_r=0.5)
    whole = rh.reheating(art, p, gb, xb, vb, **kw)
    assert np.array_equal(whole.status == REHEATED, np.arange(B) % 7 == 0) and np.all(whole.status[np.arange(B) % 7 != 0] == COMPLETE)
    for sl in (slice(0, 5), slice((1 << 20) - 2, (1 << 20) + 2), slice(B - 5, None)):
        part = rh.reheating(art, p, gb[sl], xb[sl], vb[sl], **{**kw, "rho_r_init": kw["rho_r_init"][sl]})
        assert _same(whole, part, sl), sl


def test_maps_are_their_halves(rh, bg, hyper):
    """The 6 x 5 hyperbolic grid from rest with Gamma = 0.2.  reheating_map equals inflation_end followed by reheating from the located
    end states, bit for bit.  pivot_observables_map_reheated equals pivot_observables_map with the A assembled by hand from the
    reheating map, bit for bit, and is NaN exactly where its halves are."""
    p, art = hyper
    ss, N0, N1 = [[14.0, 19.0], [-1.0, 1.0]], 6, 5
    reh, n_end, status = rh.reheating_map(art, p, 0.2, ss, N0, N1)
    x0, x1 = bg.grid_points(ss, N0, N1)
    x = np.stack([np.repeat(x0, N1), np.tile(x1, N0)], axis=1)
    end = bg.inflation_end(art, p, x, np.zeros_like(x))
    assert np.all(end.status == ENDED) and np.array_equal(end.N_end.reshape(N0, N1), n_end)
    half = rh.reheating(art, p, 0.2, end.state[:, :2], end.state[:, 2:4])
    assert np.all(half.status == REHEATED) and np.array_equal(status, half.status.reshape(N0, N1)) and np.array_equal(reh.status, status)
    for f in FIELDS:
        assert np.array_equal(getattr(reh, f).reshape(N0 * N1, -1), getattr(half, f).reshape(N0 * N1, -1)), f
    varied = rh.reheating_map(art, p, np.linspace(0.1, 1.0, 30).reshape(N0, N1), ss, N0, N1)[0]
    assert np.all(varied.status == REHEATED) and np.all(np.diff(varied.t_reh.reshape(-1)[::N1]) != 0.0)
    with np.printoptions(precision=4, linewidth=200):
        print(f"N_reh:\n{reh.N_reh}\nw_reh:\n{reh.w_reh}\nA_shift:\n{reh.A_shift}")

    obs, state, n_star, n_end2, reh2, status2 = rh.pivot_observables_map_reheated(art, p, 0.2, ss, N0, N1, return_status=True)
    short = rh.pivot_observables_map_reheated(art, p, 0.2, ss, N0, N1)
    assert len(short) == 5 and _same(reh2, reh) and _same(short[4], reh) and np.array_equal(n_end2, n_end)
    A = rh.offset_from_reheating(reh).reshape(N0, N1)
    assert np.isfinite(A).all() and np.array_equal(A, bg.reheating_offset() + reh.A_shift)
    want_obs, want_state, want_n_star, want_n_end, want_status = bg.pivot_observables_map(art, p, ss, N0, N1, A, return_status=True)
    for got, want in ((state, want_state), (n_star, want_n_star), (n_end2, want_n_end), (status2, want_status), *zip(obs, want_obs), *zip(short[0], want_obs)):
        assert np.array_equal(got, want, equal_nan=True)
    found = np.isfinite(want_n_star)
    assert 0 < found.sum() < 30 and all(np.array_equal(np.isfinite(member), found) for member in obs[:-1])
    with np.printoptions(precision=5, linewidth=200):
        print(f"n_s:\n{obs.n_s}\nr:\n{obs.r}\nN_star:\n{n_star}")


@pytest.mark.parametrize("name", ["egno", "d5"])
def test_heavy_models(rh, name):
    """The kernels with the most registers against the host build at RESTATEMENT_TOL of the model: 50 fixed steps, Gamma = 0.5,
    omega_r = 0.05.  EGNO (dt = 1e-3, the initial states of background_sampled_reference.EGNO_SEEDS) is kinetic-dominated, so that
    Omega_r grows as 2 Gamma t: most lanes reheat in their last steps and the others run out of steps.  D5 (dt = 0.1, velocities of the
    potential's energy) reheats within ten steps on every lane."""
    spec, art = workloads.artifact_for(name)
    p = np.asarray(spec.args, dtype=np.float64)
    twin = ReheatingTwin(art)
    # 65 lanes: EGNO_SEEDS and the next seed at which the host build with and without contraction agrees within 5e-14 here
    init = np.array([initial_state(name, seed=s) for s in ((*EGNO_SEEDS, 160) if name == "egno" else range(65))])
    if name == "d5":  # V ~ 1e-6: velocities of the same energy
        init[:, 2:] *= 1e-3
    dt = 1e-3 if name == "egno" else 0.1
    gamma = np.full(init.shape[0], 0.5)
    for solver in METHODS:
        reh = rh.reheating(art, p, gamma, init[:, :2], init[:, 2:], omega_r=0.05, max_steps=50, solver=solver, dt=dt)
        worst, accepted = _against_the_twin(reh, twin, p, init, gamma, 50, omega_r=0.05, method=solver, dt=dt)
        worst = float(worst.max())
        print(f"{name} {solver}: GPU vs host build, max relative difference {worst:.3e}; status {np.bincount(reh.status)}; accepted {accepted.min()} .. {accepted.max()}")
        assert worst <= RESTATEMENT_TOL[name], worst
        assert (reh.status == REHEATED).sum() >= 32 and ((reh.status == COMPLETE).sum() >= 8 if name == "egno" else np.all(reh.status == REHEATED))


def test_reheating_object_of_another_layout_is_refused():
    """Without ``<artefact>.reheating`` the call names the way to build it; an object built with INFLX_RH_ABI = 2 is refused; the
    artefact's own build then works on the same handle."""
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p = power_law_artifact()
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".reheating"
    hdr, eom_hdr = stale + ".model.h", stale + ".eom.h"
    init = np.array([power_law_init()])
    args = (init, np.array([0.5]), np.zeros(1), 0.01, 10_000, _native.EOM_RKF, 1e-6, 0.0)  # (on the attractor Omega_r grows as Gamma (1 + t) / 256: 0.01 at t = 4)
    try:
        if os.path.exists(stale):
            os.remove(stale)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        with pytest.raises(SystemError, match=r"ensure_reheating\(\)") as err:
            lib.reheating(p, *args)
        assert ".reheating exists" in str(err.value)
        for path, text in ((hdr, header_text), (eom_hdr, art.eom_header_text())):
            with open(path, "w") as fh:
                fh.write(text)
        cmd = [hipcc_path(), *options, "-DINFLX_RH_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', os.path.join(_CSRC, "inflx_reheating_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.reheating(p, *args)
        assert "INFLX_RH_ABI 2, expected 1" in str(err.value)
        os.remove(stale)
        art.ensure_reheating()
        states, t, h_start, status = lib.reheating(p, *args)
        assert states.shape == (1, 7) and status[0] == REHEATED and abs(states[0, 6] / (3.0 * states[0, 4] ** 2) - 0.01) <= 1e-14 and h_start[0] == 8.0 and t[0] > 0.0
        for bad, words in ((args[:1] + (np.array([-1.0]),) + args[2:], "decay rate"), (args[:2] + (np.array([np.inf]),) + args[3:], "radiation density"),
                           (args[:3] + (1.0,) + args[4:], "omega_r")):  # fmt: skip
            with pytest.raises(Exception, match=words):
                lib.reheating(p, *bad)
        lib.close()
    finally:
        for path in (stale, hdr, eom_hdr):
            if os.path.exists(path):
                os.remove(path)
        art._companion_paths.pop("reheating", None)
