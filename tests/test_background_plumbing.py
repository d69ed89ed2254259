"""What ``inflatox_amd.background`` hands the native layer and what it does with the answer, on a stub artefact and the fake library
of background_fake.py -- no device, no compiler.  The fake checks dtype, shape and C-contiguity of every array it is given; the tests
check the rows of the grid maps, the lanes a second stage runs again, where their results land, and the shapes and dtypes of what
comes back.  Every expectation is computed here from the lane indices and the fake's rules (``value``, ``N_END0``, ``CYCLES``)."""

import math

import numpy as np
import pytest

from background_fake import COMPLETE, CYCLES, ENDED, ENDED_SHORT, LOCATED, N_END0, TARGET, FakeLib, stub_artifact, value
from inflatox_amd import _native
from inflatox_amd import background as bg

P = np.array([0.5, 1.5, 2.5])
D = (0.25, -0.75)
#: (start_stop, N0, N1) and the grid's fields, written out: x = i * ((stop - start) / N) + start
GRIDS = {
    "3x2": (([[0.0, 3.0], [10.0, 12.0]], 3, 2), [(0.0, 10.0), (0.0, 11.0), (1.0, 10.0), (1.0, 11.0), (2.0, 10.0), (2.0, 11.0)]),
    "1x1": (([[0.5, 1.5], [2.0, 4.0]], 1, 1), [(0.5, 2.0)]),
}
N_STAR = 60.5  # lane 0 ends after N_END0 = 60 e-folds: too short


@pytest.fixture
def fake(monkeypatch):
    lib, art = FakeLib(), stub_artifact()

    def dylib(artifact, background=True):
        assert artifact is art
        if background:
            artifact.ensure_background()
        return lib

    monkeypatch.setattr(bg, "_dylib", dylib)
    return lib, art


def grid_rows(name):
    return np.array([[x0, x1, *D] for x0, x1 in GRIDS[name][1]])


def cycle(name, n):
    return np.array([CYCLES[name][i % len(CYCLES[name])] for i in range(n)])


def exit_expectation(n, n_star):
    """``horizon_exit_map`` over n grid points on the fake: (the lanes of the second pass, state (n, 5), N_end (n,), status (n,))"""
    first = cycle("solve_eom", n)
    n_end = np.where(first == ENDED, N_END0 + np.arange(n), np.nan)
    run = [k for k in range(n) if first[k] == ENDED and N_END0 + k >= n_star]
    second = cycle("solve_eom_to_efolds", len(run))
    status = np.where(first == ENDED, ENDED_SHORT, first)
    state = np.full((n, 5), np.nan)
    for c, k in enumerate(run):
        status[k] = second[c]
        if second[c] == TARGET:
            state[k] = [value(c, col) for col in range(5)]
    return run, state, n_end, status


def check_exit(got_state, got_n_end, got_status, shape, n_star):
    n = shape[0] * shape[1]
    _, state, n_end, status = exit_expectation(n, n_star)
    assert got_state.shape == (*shape, 5) and got_state.dtype == np.float64 and np.array_equal(got_state.reshape(n, 5), state, equal_nan=True)
    assert got_n_end.shape == shape and np.array_equal(got_n_end.reshape(n), n_end, equal_nan=True)
    assert np.array_equal(got_status.reshape(n), status)
    return [k for k in range(n) if status[k] == TARGET], state, status


# ---- the rows of the grid -----------------------------------------------------------------------------------------------------------
GRID_MAPS = {
    "efolds_map": (lambda art, ss, N0, N1: bg.efolds_map(art, P, ss, N0, N1, D), "solve_eom"),
    "horizon_exit_map": (lambda art, ss, N0, N1: bg.horizon_exit_map(art, P, ss, N0, N1, N_STAR, D), "solve_eom"),
    "turn_rate_map": (lambda art, ss, N0, N1: bg.turn_rate_map(art, P, ss, N0, N1, N_STAR, D), "solve_eom"),
    "mass_map": (lambda art, ss, N0, N1: bg.mass_map(art, P, ss, N0, N1, N_STAR, D), "solve_eom"),
    "transfer_map": (lambda art, ss, N0, N1: bg.transfer_map(art, P, ss, N0, N1, N_STAR, D), "solve_eom"),
    "spectrum_map": (lambda art, ss, N0, N1: bg.spectrum_map(art, P, ss, N0, N1, N_STAR - 5.0, 5.0, D), "solve_eom"),
    "evolution_map": (lambda art, ss, N0, N1: bg.evolution_map(art, P, ss, N0, N1, [0.0], N_STAR - 5.0, 5.0, D), "solve_eom"),
    "observables_map": (lambda art, ss, N0, N1: bg.observables_map(art, P, ss, N0, N1, N_STAR - 5.5, 0.5, 5.0, D), "solve_eom"),
    "fnl_map": (lambda art, ss, N0, N1: bg.fnl_map(art, P, ss, N0, N1, N_STAR, 1e-2, "fixed", D), "solve_eom"),
    "stochastic_map": (lambda art, ss, N0, N1: bg.stochastic_map(art, P, ss, N0, N1, 4, derivatives_init=D), "stochastic_efolds"),
    "stochastic_distribution_map": (lambda art, ss, N0, N1: bg.stochastic_distribution_map(art, P, ss, N0, N1, 4, 8, (-1.0, 1.0), derivatives_init=D), "stochastic_efolds"),
    "pivot_exit_map": (lambda art, ss, N0, N1: bg.pivot_exit_map(art, P, ss, N0, N1, -61.0, D), "inflation_end"),
    "pivot_observables_map": (lambda art, ss, N0, N1: bg.pivot_observables_map(art, P, ss, N0, N1, -61.0, 0.5, 5.0, D), "inflation_end"),
}


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", GRID_MAPS)
def test_grid_maps_pass_the_grid_rows(fake, name, grid):
    """The first native call of every grid map gets the rows [x0[i], x1[j], d0, d1] in row-major order and the one parameter row."""
    lib, art = fake
    call, first = GRID_MAPS[name]
    call(art, *GRIDS[grid][0])
    method, args = lib.calls[0]
    assert method == first
    assert np.array_equal(args["init"], grid_rows(grid)) and np.array_equal(args["p"], P) and args["p"].shape == (3,)
    if first == "solve_eom":
        assert (args["rows"], args["substeps"], args["flags"], args["dt"]) == (100_001 if name != "fnl_map" else 1_000_001, 1, _native.EOM_STOP_AT_END | _native.EOM_FINAL_ONLY, 0.0)


@pytest.mark.parametrize("grid", GRIDS)
def test_efolds_map(fake, grid):
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n_end, status = bg.efolds_map(art, P, ss, N0, N1, D, return_status=True)
    first = cycle("solve_eom", N0 * N1)
    assert n_end.shape == status.shape == (N0, N1) and status.dtype == np.int8
    assert np.array_equal(status.reshape(-1), first) and np.array_equal(n_end.reshape(-1), np.where(first == ENDED, N_END0 + np.arange(N0 * N1), np.nan), equal_nan=True)
    assert [m for m, _ in lib.calls] == ["solve_eom"] and art.ensured == ["background"]
    assert np.array_equal(bg.efolds_map(art, P, ss, N0, N1, D), n_end, equal_nan=True)


@pytest.mark.parametrize("grid", GRIDS)
def test_horizon_exit_map_runs_the_points_that_ended_late_enough(fake, grid):
    """The second pass gets exactly the points that ENDED with N_end >= N_star, their grid rows and the targets N_end - N_star; the
    states land at those points, and ``status`` is TARGET / ENDED_SHORT / the first pass's elsewhere."""
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n_star = N_STAR if grid == "3x2" else 55.0
    state, n_end, status = bg.horizon_exit_map(art, P, ss, N0, N1, n_star, D, return_status=True)
    assert status.dtype == np.int8 and status.shape == (N0, N1)
    check_exit(state, n_end, status, (N0, N1), n_star)
    run = exit_expectation(N0 * N1, n_star)[0]
    assert run == ([1, 3, 4] if grid == "3x2" else [0])
    assert [m for m, _ in lib.calls] == ["solve_eom", "solve_eom_to_efolds"]
    second = lib.calls[1][1]
    assert np.array_equal(second["init"], grid_rows(grid)[run]) and np.array_equal(second["target"], np.array([N_END0 + k - n_star for k in run]))
    assert np.array_equal(second["p"], P) and second["flags"] == _native.EOM_STOP_AT_END and second["max_steps"] == 100_000
    assert len(bg.horizon_exit_map(art, P, ss, N0, N1, n_star, D)) == 2


def test_horizon_exit_map_without_a_second_pass(fake):
    lib, art = fake
    (ss, N0, N1), _ = GRIDS["3x2"]
    state, n_end, status = bg.horizon_exit_map(art, P, ss, N0, N1, 1000.0, D, return_status=True)
    assert [m for m, _ in lib.calls] == ["solve_eom"] and np.isnan(state).all()
    assert np.array_equal(status.reshape(-1), np.where(cycle("solve_eom", 6) == ENDED, ENDED_SHORT, COMPLETE))


# ---- the maps with a second stage ----------------------------------------------------------------------------------------------------
def second_stage(lib, grid, method, n_star=N_STAR):
    """the lanes whose exit state was found, their rows (fields, velocities of the exit state), and the first call of ``method``"""
    n = len(GRIDS[grid][1])
    _, state, _, status = exit_expectation(n, n_star)
    lanes = [k for k in range(n) if status[k] == TARGET]
    calls = lib.named(method)
    return lanes, state[lanes, :4], status, calls[0] if calls else None


@pytest.mark.parametrize("name,method,planes", [("turn_rate_map", "kinematics", 6), ("mass_map", "masses", 8)])
@pytest.mark.parametrize("grid", GRIDS)
def test_pointwise_maps(fake, grid, name, method, planes):
    """``turn_rate_map`` and ``mass_map`` hand every exit state of the grid, found or NaN, to the pointwise pass in one call."""
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n_star = N_STAR if grid == "3x2" else 55.0
    res, state, n_end, status = getattr(bg, name)(art, P, ss, N0, N1, n_star, D, return_status=True)
    check_exit(state, n_end, status, (N0, N1), n_star)
    args = lib.named(method)[0]
    n = N0 * N1
    assert (args["n"], args["ld"], args["traj_len"]) == (n, 5, N1) and np.array_equal(args["states"].reshape(n, 5), state.reshape(n, 5), equal_nan=True)
    assert len(res) == planes and art.ensured == ["background", "background", method]
    for plane, member in enumerate(res):
        assert member.shape == (N0, N1) and np.array_equal(member.reshape(n), value(np.arange(n), plane))


@pytest.mark.parametrize("grid", GRIDS)
def test_transfer_map(fake, grid):
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n_star = N_STAR if grid == "3x2" else 55.0
    n = N0 * N1
    dq = 0.5 * np.arange(n).reshape(N0, N1)
    (t_rs, t_ss), state, n_end, status = bg.transfer_map(art, P, ss, N0, N1, n_star, D, dq_dN=dq, return_status=True)
    check_exit(state, n_end, np.where(np.isnan(state[..., 0]), status, TARGET), (N0, N1), n_star)
    lanes, rows, before, args = second_stage(lib, grid, "transfer_functions", n_star)
    assert np.array_equal(args["init"], rows) and np.array_equal(args["samples"], [0.0]) and np.array_equal(args["dq_dn"], [0.5 * k for k in lanes])
    assert args["flags"] == _native.EOM_STOP_AT_END and art.ensured[-1] == "transfer"
    stage = cycle("transfer_functions", len(lanes))
    want_rs, want_ss, want_status = np.full(n, np.nan), np.full(n, np.nan), before.copy()
    for c, k in enumerate(lanes):
        want_status[k] = stage[c]
        if stage[c] == ENDED:
            want_ss[k], want_rs[k] = value(c, 0), value(c, 1)
    assert t_rs.shape == t_ss.shape == status.shape == (N0, N1) and status.dtype == np.int8
    assert np.array_equal(t_rs.reshape(n), want_rs, equal_nan=True) and np.array_equal(t_ss.reshape(n), want_ss, equal_nan=True)
    assert np.array_equal(status.reshape(n), want_status)
    lib.calls.clear()
    bg.transfer_map(art, P, ss, N0, N1, n_star, D, dq_dN=0.25)
    assert np.array_equal(lib.named("transfer_functions")[0]["dq_dn"], np.full(len(lanes), 0.25))
    lib.calls.clear()
    bg.transfer_map(art, P, ss, N0, N1, n_star, D)
    assert lib.named("transfer_functions")[0]["dq_dn"] is None


@pytest.mark.parametrize("grid", GRIDS)
def test_spectrum_map(fake, grid):
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n_star, n_sub = (N_STAR if grid == "3x2" else 55.0) - 4.0, 4.0
    n = N0 * N1
    spectra, state, n_end, status = bg.spectrum_map(art, P, ss, N0, N1, n_star, n_sub, D, return_status=True)
    check_exit(state, n_end, np.where(np.isnan(state[..., 0]), status, TARGET), (N0, N1), n_star + n_sub)
    lanes, rows, before, args = second_stage(lib, grid, "solve_eom_sampled", n_star + n_sub)
    assert np.array_equal(args["init"], rows) and np.array_equal(args["samples"], [0.0, n_sub])
    mode = lib.named("mode_spectra")[0]
    # the lanes start from the first stage's state at the sample 0 and the H at the sample N_sub (value(lane, plane, sample))
    assert np.array_equal(mode["init"], [[value(c, col, 0) for col in range(4)] for c in range(len(lanes))])
    assert np.array_equal(mode["kappa"], [value(c, 4, 1) * math.exp(n_sub) for c in range(len(lanes))]) and np.isnan(mode["n_target"]).all()
    stage = cycle("mode_spectra", len(lanes))
    want, want_status = np.full((3, n), np.nan), before.copy()
    for c, k in enumerate(lanes):
        want_status[k] = stage[c]
        if stage[c] == ENDED:
            want[:, k] = [value(c, plane) for plane in range(3)]
    assert isinstance(spectra, tuple) and len(spectra) == 3 and all(s.shape == (N0, N1) for s in spectra)
    assert np.array_equal(np.stack(spectra).reshape(3, n), want, equal_nan=True)
    assert status.dtype == np.int8 and np.array_equal(status.reshape(n), want_status)


@pytest.mark.parametrize("grid", GRIDS)
def test_evolution_map(fake, grid):
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n_star, n_sub, samples = (N_STAR if grid == "3x2" else 55.0) - 4.0, 4.0, [-1.0, 0.0, 2.0]
    n = N0 * N1
    spectra, state, n_end, status = bg.evolution_map(art, P, ss, N0, N1, samples, n_star, n_sub, D, return_status=True)
    lanes, rows, before, args = second_stage(lib, grid, "solve_eom_sampled", n_star + n_sub)
    assert np.array_equal(args["init"], rows)
    evo = lib.named("mode_evolution")[0]
    assert np.array_equal(evo["samples"], samples) and np.array_equal(evo["shift"], np.full(len(lanes), -n_sub)) and evo["init"].shape == (len(lanes), 4)
    assert art.ensured[-1] == "evolution" and not lib.named("mode_spectra")
    stage = cycle("mode_evolution", len(lanes))
    want, want_status = np.full((3, n, 3), np.nan), before.copy()
    for c, k in enumerate(lanes):  # the samples of a lane are kept whatever its status
        want_status[k] = stage[c]
        want[:, k, :] = [[value(c, plane, s) for s in range(3)] for plane in range(3)]
    assert len(spectra) == 3 and all(s.shape == (N0, N1, 3) for s in spectra)
    assert np.array_equal(np.stack(spectra).reshape(3, n, 3), want, equal_nan=True)
    assert status.dtype == np.int8 and status.shape == (N0, N1) and np.array_equal(status.reshape(n), want_status)


@pytest.mark.parametrize("grid", GRIDS)
def test_observables_map(fake, grid):
    """Three wavenumbers per point, scalar and tensor: the lanes b 3 + j.  With the cycle below all six lanes of the first point found
    end inflation and one of the second's does not."""
    lib, art = fake
    lib.cycles["mode_spectra"] = (ENDED,) * 5 + (COMPLETE,)
    (ss, N0, N1), _ = GRIDS[grid]
    n_star, dn, n_sub = (N_STAR if grid == "3x2" else 55.0) - 4.5, 0.5, 4.0
    n = N0 * N1
    obs, state, n_end, status = bg.observables_map(art, P, ss, N0, N1, n_star, dn, n_sub, D, return_status=True)
    lanes, rows, before, args = second_stage(lib, grid, "solve_eom_sampled", n_star + n_sub + dn)
    assert np.array_equal(args["init"], rows)
    modes = lib.named("mode_spectra")
    assert [m["flags"] for m in modes] == [_native.EOM_STOP_AT_END, _native.EOM_STOP_AT_END | _native.MODES_TENSOR] and all(m["init"].shape == (3 * len(lanes), 4) for m in modes)
    want_status = before.copy()
    valid = np.zeros(n, dtype=bool)
    for c, k in enumerate(lanes):
        valid[k] = c == 0
        want_status[k] = ENDED if c == 0 else COMPLETE
    assert isinstance(obs, bg.Observables) and all(member.shape == (N0, N1) for member in obs)
    assert obs.status.dtype == np.int8 and np.array_equal(obs.status.reshape(n), want_status) and np.array_equal(status, obs.status)
    for member in obs[:8]:
        assert np.array_equal(np.isfinite(member.reshape(n)), valid)
    for member in (obs.k, obs.N_end):  # not masked by the pivot's status: finite wherever the second stage ran
        assert np.array_equal(np.isfinite(member.reshape(n)), np.isin(np.arange(n), lanes))
    if lanes:  # the pivot's own lane is lane 1 of the second stage, scalar and tensor: planes 0 are P_R and P_T
        k = lanes[0]
        assert (obs.A_s.reshape(n)[k], obs.A_t.reshape(n)[k], obs.r.reshape(n)[k]) == (value(1, 0), value(1, 0), 1.0)


@pytest.mark.parametrize("grid", GRIDS)
def test_fnl_map(fake, grid):
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n_star = N_STAR if grid == "3x2" else 55.0
    n = N0 * N1
    dn, state, n_end, status = bg.fnl_map(art, P, ss, N0, N1, n_star, (1e-2, 2e-2), "slow_roll", D, return_status=True)
    lanes, rows, before, args = second_stage(lib, grid, "delta_n", n_star)
    assert np.array_equal(args["centre"], rows) and args["vel"] is None and args["h_end"] is None
    assert (args["rule"], args["h0"], args["h1"], args["max_steps"]) == (_native.DN_SLOW_ROLL, 1e-2, 2e-2, 1_000_000) and art.ensured[-1] == "deltan"
    stage = cycle("delta_n", len(lanes))
    want_status = before.astype(np.int16)
    want = {"N": (4,), "f_NL": (18,), "P_zeta": (19,), "grad2": (17,), "N_members": range(9), "N_I": (9, 10), "N_IJ": (11, 13, 13, 12), "N_cov": (14, 16, 16, 15)}
    shapes = {"N_members": (3, 3), "N_I": (2,), "N_IJ": (2, 2), "N_cov": (2, 2)}
    for name, planes in want.items():
        member = getattr(dn, name)
        assert member.shape == (N0, N1, *shapes.get(name, ())), name
        expect = np.full((n, len(planes)), np.nan)
        for c, k in enumerate(lanes):
            expect[k] = [value(c, plane) for plane in planes]
        assert np.array_equal(member.reshape(n, -1), expect, equal_nan=True), name
    for c, k in enumerate(lanes):
        want_status[k] = stage[c]
    assert dn.H_end.shape == (N0, N1) and np.array_equal(np.isfinite(dn.H_end.reshape(n)), np.isin(np.arange(n), lanes))
    assert dn.status.dtype == np.int16 and status.dtype == np.int16 and np.array_equal(status.reshape(n), want_status) and np.array_equal(dn.status, status)
    if grid == "3x2":
        assert list(want_status) == [ENDED_SHORT, LOCATED, COMPLETE, COMPLETE + 64, ENDED, COMPLETE]


# ---- the pivot maps -----------------------------------------------------------------------------------------------------------------
def pivot_expectation(n, A, ln_k):
    """``_pivot_crossing`` over n grid points on the fake: (run, N_end (n,), pivot (n,), state (n, 5), N (n,), status (n,))"""
    first = cycle("inflation_end", n)
    n_end = np.where(first == ENDED, value(np.arange(n), 5), np.nan)
    pivot = n_end + 0.5 * np.log(value(np.arange(n), 4)) + A
    run = [k for k in range(n) if first[k] == ENDED]
    crossed, before = cycle("solve_eom_crossings", len(run)), cycle("n_before", len(run))
    status, state, n_at = first.copy(), np.full((n, 5), np.nan), np.full(n, np.nan)
    for c, k in enumerate(run):
        status[k] = ENDED_SHORT if before[c] == 1 else crossed[c]
        state[k], n_at[k] = [value(c, col) for col in range(5)], value(c, 5)
    return run, n_end, pivot, state, n_at, status


@pytest.mark.parametrize("grid", GRIDS)
def test_pivot_exit_map(fake, grid):
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n = N0 * N1
    A = -61.0 + 0.125 * np.arange(n).reshape(N0, N1)
    state, n_star, n_end, status = bg.pivot_exit_map(art, P, ss, N0, N1, A, D, return_status=True)
    run, want_end, pivot, want_state, n_at, want_status = pivot_expectation(n, A.reshape(n), 0.0)
    assert [m for m, _ in lib.calls] == ["inflation_end", "solve_eom_crossings"] and art.ensured == ["crossing", "crossing"]
    crossing = lib.calls[1][1]
    assert np.array_equal(crossing["init"], grid_rows(grid)[run]) and np.array_equal(crossing["offset"], pivot[run]) and np.array_equal(crossing["samples"], [0.0])
    assert state.shape == (N0, N1, 5) and n_star.shape == n_end.shape == status.shape == (N0, N1) and status.dtype == np.int8
    assert np.array_equal(state.reshape(n, 5), want_state, equal_nan=True) and np.array_equal(n_end.reshape(n), want_end, equal_nan=True)
    assert np.array_equal(n_star.reshape(n), want_end - n_at, equal_nan=True) and np.array_equal(status.reshape(n), want_status)
    if grid == "3x2":
        assert run == [0, 1, 3, 4] and list(want_status) == [TARGET, ENDED_SHORT, COMPLETE, COMPLETE, ENDED_SHORT, COMPLETE]


@pytest.mark.parametrize("grid", GRIDS)
def test_pivot_observables_map(fake, grid):
    """The second stage runs from every point whose crossing was located (a finite N), whatever its status: the restart rows and the
    offsets L_star - N of its own crossings call, NaN and the first stage's status everywhere else."""
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n, dlnk, n_sub = N0 * N1, 0.5, 4.0
    obs, state, n_star, n_end, status = bg.pivot_observables_map(art, P, ss, N0, N1, -61.0, dlnk, n_sub, D, return_status=True)
    run, want_end, pivot, want_state, n_at, before = pivot_expectation(n, -61.0, -(dlnk + n_sub))
    crossings = lib.named("solve_eom_crossings")
    assert np.array_equal(crossings[0]["samples"], [-(dlnk + n_sub)]) and np.array_equal(crossings[0]["init"], grid_rows(grid)[run])
    # scalar lanes, then tensor lanes: the same crossings call twice, from the restart states
    assert len(crossings) == 3 and all(np.array_equal(c["init"], want_state[run, :4]) and np.array_equal(c["offset"], (pivot - n_at)[run]) for c in crossings[1:])
    assert all(np.array_equal(c["samples"], [-dlnk, 0.0, dlnk]) for c in crossings[1:])
    assert isinstance(obs, bg.Observables) and all(member.shape == (N0, N1) for member in obs) and obs.status.dtype == np.int8 and np.array_equal(obs.status, status)
    assert state.shape == (N0, N1, 5) and np.array_equal(state.reshape(n, 5), want_state, equal_nan=True) and np.array_equal(n_end.reshape(n), want_end, equal_nan=True)
    outside = ~np.isin(np.arange(n), run)
    for member in obs[:-1]:
        assert np.isnan(member.reshape(n)[outside]).all()
    assert np.array_equal(status.reshape(n)[outside], before[outside]) and np.isfinite(obs.k.reshape(n)[~outside]).all()
    # N_star = N_end - (the restart's N + the pivot's exit since the restart: sample 1 of the second stage's crossings)
    want_star = np.full(n, np.nan)
    for c, k in enumerate(run):
        want_star[k] = want_end[k] - (n_at[k] + value(c, 5, 1))
    assert n_star.shape == (N0, N1) and np.array_equal(n_star.reshape(n), want_star, equal_nan=True)
    assert len(bg.pivot_observables_map(art, P, ss, N0, N1, -61.0, dlnk, n_sub, D)) == 4


# ---- the stochastic maps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", GRIDS)
def test_stochastic_map(fake, grid):
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n = N0 * N1
    res = bg.stochastic_map(art, P, ss, N0, N1, 4, derivatives_init=D, seed=7, noise_scale=0.5, dN_max=0.25, N_stop=3.0, dt=1e-3)
    noisy, classical = lib.named("stochastic_efolds")
    for args in (noisy, classical):
        assert np.array_equal(args["init"], grid_rows(grid)) and args["streams"] is None and (args["seed"], args["dn_max"], args["n_stop"], args["dt"]) == (7, 0.25, 3.0, 1e-3)
    assert (noisy["R"], noisy["noise_scale"], classical["R"], classical["noise_scale"]) == (4, 0.5, 1, 0.0) and art.ensured == ["stochastic"]
    stage = cycle("stochastic_efolds", n)
    assert res.N_mean.shape == (N0, N1) and np.array_equal(res.N_mean.reshape(n), value(np.arange(n), 0)) and np.array_equal(res.N_max.reshape(n), value(np.arange(n), 5))
    assert res.counts.shape == (N0, N1, 6) and res.counts.dtype == np.int64 and np.array_equal(res.counts.reshape(n, 6), 4 * (stage[:, None] == np.arange(6)))
    assert np.array_equal(res.n_ended.reshape(n), 4 * (stage == ENDED)) and res.N is None and res.state is None and res.status is None
    assert np.array_equal(res.N_classical.reshape(n), np.where(stage == ENDED, value(np.arange(n), 0), np.nan), equal_nan=True)


@pytest.mark.parametrize("grid", GRIDS)
def test_stochastic_distribution_map(fake, grid):
    """Centred on the classical e-fold count, only the points whose classical run ended are run: their rows, their streams (the flat
    index) and their shifted ranges; the others have zero counts and NaN edges."""
    lib, art = fake
    (ss, N0, N1), _ = GRIDS[grid]
    n, bins = N0 * N1, 4
    res = bg.stochastic_distribution_map(art, P, ss, N0, N1, 5, bins, (-1.0, 1.0), derivatives_init=D, seed=3, first_realisation=10, lanes_per_point=128)
    stage = cycle("stochastic_efolds", n)
    run = [k for k in range(n) if stage[k] == ENDED]
    classical = lib.named("stochastic_efolds")[0]
    assert np.array_equal(classical["init"], grid_rows(grid)) and np.array_equal(classical["streams"], np.arange(n)) and classical["R"] == 1 and math.isnan(classical["n_stop"])
    args = lib.named("stochastic_distribution")[0]
    assert np.array_equal(args["init"], grid_rows(grid)[run]) and np.array_equal(args["streams"], run) and np.array_equal(args["p"], P)
    assert np.array_equal(args["ranges"], [[-1.0 + value(k, 0), 1.0 + value(k, 0)] for k in run])
    assert (args["R"], args["seed"], args["first"], args["lanes_per_point"], args["bins"]) == (5, 3, 10, 128, bins) and art.ensured == ["stochastic", "distribution"]
    hist, below, above, counts = np.zeros((n, bins), dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros((n, 6), dtype=np.int64)
    edges = np.full((n, bins + 1), np.nan)
    for c, k in enumerate(run):
        hist[k], below[k], above[k] = [c + 1000 * b for b in range(1, bins + 1)], c, c + 1000 * (bins + 1)
        counts[k] = [c + 1000 * s for s in range(6)]
        edges[k] = [-1.0 + value(k, 0) + b * (2.0 / bins) for b in range(bins + 1)]
    assert res.hist.shape == (N0, N1, bins) and res.hist.dtype == np.int64 and np.array_equal(res.hist.reshape(n, bins), hist)
    assert np.array_equal(res.below.reshape(n), below) and np.array_equal(res.above.reshape(n), above) and np.array_equal(res.counts.reshape(n, 6), counts)
    assert res.edges.shape == (N0, N1, bins + 1) and np.array_equal(res.edges.reshape(n, bins + 1), edges, equal_nan=True)
    assert (res.realisations, res.first_realisation, res.seed) == (5, 10, 3) and res.N_classical.shape == (N0, N1)


# ---- batches ------------------------------------------------------------------------------------------------------------------------
BATCH_CALLS = {
    "solve_eom_batch": (lambda art, p, x, v: bg.solve_eom_batch(art, p, 7, x, v), "solve_eom"),
    "state_at_efolds": (lambda art, p, x, v: bg.state_at_efolds(art, p, x, v, 3.0), "solve_eom_to_efolds"),
    "solve_eom_sampled": (lambda art, p, x, v: bg.solve_eom_sampled(art, p, [0.0, 1.0], x, v), "solve_eom_sampled"),
    "transfer_functions": (lambda art, p, x, v: bg.transfer_functions(art, p, [0.0, 1.0], x, v), "transfer_functions"),
    "power_spectra": (lambda art, p, x, v: bg.power_spectra(art, p, [6.0, 7.0], x, v), "solve_eom_sampled"),
    "tensor_spectra": (lambda art, p, x, v: bg.tensor_spectra(art, p, [6.0, 7.0], x, v), "solve_eom_sampled"),
    "spectra_evolution": (lambda art, p, x, v: bg.spectra_evolution(art, p, [6.0, 7.0], [0.0, 1.0], x, v), "solve_eom_sampled"),
    "observables": (lambda art, p, x, v: bg.observables(art, p, [6.0], x, v), "solve_eom_sampled"),
    "delta_N": (lambda art, p, x, v: bg.delta_N(art, p, x, v), "delta_n"),
    "stochastic_efolds": (lambda art, p, x, v: bg.stochastic_efolds(art, p, x, v, 3, return_samples=True), "stochastic_efolds"),
    "stochastic_distribution": (lambda art, p, x, v: bg.stochastic_distribution(art, p, x, v, 3, 4, (50.0, 70.0)), "stochastic_efolds"),
    "horizon_crossings": (lambda art, p, x, v: bg.horizon_crossings(art, p, [-1.0, 0.0], x, v), "solve_eom_crossings"),
    "inflation_end": (lambda art, p, x, v: bg.inflation_end(art, p, x, v), "inflation_end"),
    "power_spectra_at_k": (lambda art, p, x, v: bg.power_spectra_at_k(art, p, [0.0, 1.0], x, v), "solve_eom_crossings"),
    "tensor_spectra_at_k": (lambda art, p, x, v: bg.tensor_spectra_at_k(art, p, [0.0, 1.0], x, v), "solve_eom_crossings"),
    "observables_at_k": (lambda art, p, x, v: bg.observables_at_k(art, p, [0.0], x, v), "solve_eom_crossings"),
}


@pytest.mark.parametrize("B", [3, 0])
@pytest.mark.parametrize("name", BATCH_CALLS)
def test_batches_pass_fields_and_velocities(fake, name, B):
    """Every batch function hands the native layer the rows [x0, x1, v0, v1] of its B trajectories, B = 0 included, and one parameter
    row per trajectory as given; lists that are not C-contiguous float64 arrive as such arrays (the fake asserts it)."""
    lib, art = fake
    x = np.asfortranarray(np.arange(2.0 * B).reshape(B, 2) + 1.0)
    v = [[0.125 * b, -0.25 * b] for b in range(B)] if B else np.empty((0, 2), dtype=np.float32)
    p = np.arange(3.0 * B).reshape(B, 3)
    call, first = BATCH_CALLS[name]
    res = call(art, p, x, v)
    method, args = lib.calls[0]
    key = "centre" if first == "delta_n" else "init"
    assert method == first and args[key].shape == (B, 4)
    assert np.array_equal(args[key], [[1.0 + 2 * b, 2.0 + 2 * b, 0.125 * b, -0.25 * b] for b in range(B)] if B else np.empty((0, 4)))
    assert np.array_equal(args["p"], p)
    lead = res[0] if isinstance(res, tuple) and not hasattr(res, "_fields") else res
    assert lead[0].shape[0] == B


def test_batch_results(fake):
    """Shapes, dtypes and the NaN rules of the plain batch calls."""
    lib, art = fake
    x, v = np.arange(6.0).reshape(3, 2), np.zeros((3, 2))
    sol = bg.solve_eom_batch(art, P, 7, x, v, substeps=2, stop_at_end=True, solver="rk4", dt=0.5, max_err=1e-3)
    args = lib.calls[-1][1]
    assert (args["rows"], args["substeps"], args["method"], args["max_err"], args["dt"], args["flags"]) == (7, 2, _native.EOM_RK4, 1e-3, 0.5, _native.EOM_STOP_AT_END)
    assert sol.states.shape == (3, 7, 5) and sol.t.shape == sol.N.shape == (3, 7) and sol.status.dtype == np.int8 and sol.last_row.dtype == np.int64
    assert np.array_equal(bg.solve_eom(art, P, 7, x[1], v[1]), sol.states[0] * 0 + [[value(0, col, row) for col in range(5)] for row in range(7)])
    got = bg.state_at_efolds(art, P, x, v, [1.0, 2.0, 3.0], stop_at_end=False)
    assert np.array_equal(lib.calls[-1][1]["target"], [1.0, 2.0, 3.0]) and lib.calls[-1][1]["flags"] == 0
    hit = cycle("solve_eom_to_efolds", 3) == TARGET
    assert got.state.shape == (3, 5) and np.array_equal(np.isfinite(got.state).all(axis=1), hit) and np.array_equal(np.isfinite(got.t), hit)
    assert np.array_equal(got.N_end, np.where(~hit, N_END0 + np.arange(3), np.nan), equal_nan=True)
    sam = bg.solve_eom_sampled(art, P, [0.0, 1.0], x, v, at="t")
    assert lib.calls[-1][1]["flags"] == _native.EOM_STOP_AT_END | _native.EOM_SAMPLE_T
    assert sam.states.shape == (3, 2, 5) and sam.t.shape == (3, 2) and sam.n_stored.dtype == np.uint32 and sam.states[2, 1, 4] == value(2, 4, 1)
    end = bg.inflation_end(art, P, x, v)
    ended = cycle("inflation_end", 3) == ENDED
    assert end.state.shape == (3, 5) and np.array_equal(np.isfinite(end.N_end), ended) and end.status.dtype == np.int8
    cr = bg.horizon_crossings(art, P, [-1.0, 0.0], x, v, offset=[0.5, 1.5, 2.5], stop_at_end=False)
    assert np.array_equal(lib.calls[-1][1]["offset"], [0.5, 1.5, 2.5]) and lib.calls[-1][1]["flags"] == 0
    assert cr.states.shape == (3, 2, 5) and np.array_equal(cr.ln_aH, cr.N + np.log(cr.states[..., 4])) and cr.n_before.dtype == np.uint32
    kin = bg.kinematics(art, np.arange(9.0).reshape(3, 3), np.ones((3, 4, 5)))
    assert (lib.calls[-1][1]["n"], lib.calls[-1][1]["traj_len"]) == (12, 4) and kin.eps_H.shape == (3, 4) and art.ensured[-1] == "kinematics"
    assert bg.masses(art, P, np.ones((0, 5))).mu_s2.shape == (0,) and lib.calls[-1][0] == "kinematics"
