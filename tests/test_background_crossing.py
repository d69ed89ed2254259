"""Horizon crossings on the host build (tests/crossing_twin.cpp compiles csrc/inflx_crossing.h for the CPU): the twin against a numpy
restatement of the rule with an independent root search, the residual of N + ln H at every emitted crossing, the analytic power-law
attractor, the located end of inflation, ``reheating_offset`` against the formula restated from its own constants, the front end's
argument checks, the public surface, and the twin under sanitizers."""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import workloads
from background_reference import COMPLETE, ENDED, P_POW, BackgroundTwin, model_functions, power_law_artifact, power_law_exact, power_law_init, solve_ivp_reference
from background_target_reference import TARGET, hermite
from conftest import ROOT
from crossing_reference import CrossingTwin, reheating_offset_restated, restated_crossings

# twin against restatement: the same steps (one host stepper), the same cubic in another basis, theta from two root searches that stop
# at 1e-15 and 1e-16: the states differ by rounding, amplified by the cancellation inside a step of dt = 0.5 (2e-13 measured)
RULE_TOL = 1e-12


def _hyper_batch(B, seed=0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(1.5, 4.0, B), rng.uniform(-1, 1, B)], axis=1), rng.uniform(-0.2, 0.2, (B, 2))


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return art, np.asarray(spec.args, dtype=np.float64), CrossingTwin(art), BackgroundTwin(art)


def _ln_h0(stepper, p, init):
    return math.log(stepper.solve(p, init, 1)[0][0, 4])  # (libm's logarithm, the twin's: a target AT ln H_0 hangs on its last bit)


def _compare(hyper, init, samples, max_steps, **kw):
    """the twin and the restatement of one trajectory: equal status, counts, NaN pattern and emitting steps, values within RULE_TOL"""
    _art, p, twin, stepper = hyper
    got, meta = twin.solve(p, init, samples, max_steps, **kw)
    want, ref = restated_crossings(stepper, p, init, samples, max_steps, **kw)
    assert (meta["status"], meta["n_stored"], meta["n_before"]) == (ref["status"], ref["n_stored"], ref["n_before"]), (meta, ref)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(meta["step_of"], ref["step_of"], equal_nan=True)
    lo, n = meta["n_before"], meta["n_stored"]
    emitted = np.zeros(len(samples), dtype=bool)
    emitted[lo : lo + n] = True
    assert np.array_equal(emitted, np.isfinite(got).all(axis=1)) and np.array_equal(emitted, ~np.isnan(got).any(axis=1))
    if meta["status"] == ENDED:
        assert meta["N_end"] == ref["N_end"]
    worst = float(np.max(np.abs(got[emitted] - want[emitted]) / np.maximum(np.abs(want[emitted]), 1e-3))) if n else 0.0
    assert worst <= RULE_TOL, worst
    tau = kw.get("offset", 0.0) + np.asarray(samples, dtype=np.float64)[emitted]
    residual = np.abs(got[emitted, 5] + np.log(got[emitted, 4]) - tau) / np.maximum(1.0, np.abs(tau))
    return got, meta, float(residual.max()) if n else 0.0


def test_twin_against_the_restated_rule(hyper):
    """Eight hyperbolic trajectories (one starts past the end of inflation), targets relative to each one's own ln H_0: adaptive rkf with
    a target before the start and one at it; fixed dt = 1e-3 with crossings more than 256 accepted steps apart and a max_steps that runs
    out; dt = 0.5 with three crossings inside the first step.  Residual: |N + ln H - tau| <= 1e-12 max(1, |tau|) on every emitted sample."""
    _art, p, _twin, stepper = hyper
    x, v = _hyper_batch(8, seed=3)
    seen = dict(before=0, at_start=0, past_end=0, far_apart=0, ran_out=0, one_step=0, target=0, ended=0)
    worst = 0.0
    for k in range(8):
        init = np.concatenate([x[k], v[k]])
        l0 = _ln_h0(stepper, p, init)
        got, meta, res = _compare(hyper, init, [-1.0, 0.0, 0.02, 0.1, 0.5, 1.0, 3.0], 100_000, offset=l0, method="rkf", stop_at_end=True)
        worst = max(worst, res)
        assert meta["n_before"] == 1 and meta["step_of"][1] == 0 and got[1, 5] == 0.0 and got[1, 6] == 0.0  # tau = L_0: the initial state
        seen["before"] += 1
        seen["at_start"] += 1
        seen["past_end"] += meta["status"] == ENDED and meta["accepted"] == 0 and meta["N_end"] == 0.0
        seen["ended"] += meta["status"] == ENDED and meta["accepted"] > 0
        _, meta, res = _compare(hyper, init, [0.02, 0.15, 0.4, 50.0], 1000, offset=l0, method="rk4", dt=1e-3, stop_at_end=True)
        worst = max(worst, res)
        steps = meta["step_of"][: meta["n_stored"]]
        seen["far_apart"] += steps.size >= 2 and np.diff(steps).max() > 256
        seen["ran_out"] += meta["status"] == COMPLETE and meta["accepted"] == 1000 and meta["n_stored"] < 4
        _, meta, res = _compare(hyper, init, [1e-3, 2e-3, 3e-3], 10, offset=l0, method="rkf", dt=0.5, stop_at_end=True)
        worst = max(worst, res)
        seen["one_step"] += meta["n_stored"] == 3 and bool((meta["step_of"] == 1).all())
        seen["target"] += meta["status"] == TARGET
    print(f"cases seen {seen}; worst residual |N + ln H - tau| / max(1, |tau|) = {worst:.3e}")
    assert all(count > 0 for count in seen.values()), seen
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_the_step_that_ends_inflation(hyper, method):
    """Nine targets inside the step that ends inflation (fixed dt = 0.05) and one above its end state's ln(a H).  The rule emits a
    crossing of that step only if its located N is <= N_end.  ln(a H) has its maximum where epsilon_H = 1, so every crossing inside
    the step lies before the true end of inflation; N_end's linear rule is later than all nine here, and the run with stop_at_end emits
    them bit for bit as the run without it does, then ends with the tenth target left.  (On no trajectory tried -- eight hyperbolic
    ones, dt from 0.05 to 0.5 -- does a crossing of the ending step fall behind the linear N_end: the cut-off is the sampled kernels'
    rule kept for the case, and the restatement applies it too.)"""
    _art, p, twin, stepper = hyper
    x, v = _hyper_batch(8, seed=3)
    init = np.concatenate([x[3], v[3]])
    rows, meta = stepper.solve(p, init, 2000, method=method, dt=0.05, stop_at_end=True)
    last = meta["last_row"]
    assert meta["status"] == ENDED and last > 10
    L = rows[: last + 1, 5] + np.log(rows[: last + 1, 4])
    assert L[last] > L[last - 1]
    samples = np.concatenate([L[last - 1] + (L[last] - L[last - 1]) * np.linspace(0.1, 0.9, 9), [L[last] + 1e-6]])
    free, fm = twin.solve(p, init, samples[:9], 2000, method=method, dt=0.05, stop_at_end=False)
    assert fm["status"] == TARGET and fm["n_stored"] == 9 and (fm["step_of"] == last).all()
    assert np.all(free[:, 5] <= meta["N_end"]) and np.all(free[:, 5] > rows[last - 1, 5]) and np.all(np.diff(free[:, 5]) > 0)
    cut, cm, _ = _compare(hyper, init, samples, 2000, method=method, dt=0.05, stop_at_end=True)
    assert cm["status"] == ENDED and cm["n_stored"] == 9 and cm["N_end"] == meta["N_end"] and cm["accepted"] == last
    assert np.array_equal(cut[:9], free) and np.isnan(cut[9]).all()


def test_locate_inside_a_bracket(hyper):
    """inflx_hx_locate alone, on steps given by their ends: a smooth step, and one whose H bends so strongly that Newton's first
    iterates leave the bracket.  The root has |g| at rounding, and theta stays inside [0, 1]."""
    _art, _p, twin, _stepper = hyper
    for ends, h in (([0.0, 0.9, 0.85, 0.8, 0.9, -0.05, 0.85, -0.06], 1.0), ([0.0, 1.0, 0.2, 0.1, 1.0, -3.0, 0.9, 2.5], 1.0), ([2.0, 3.0, 2.7, 0.5, 3.0, 0.0, 2.0, -8.0], 0.5)):
        l0, l1 = ends[0] + math.log(ends[4]), ends[2] + math.log(ends[6])
        assert l1 > l0
        for frac in (1e-9, 0.03, 0.5, 0.97, 1.0):
            tau = l0 + frac * (l1 - l0)
            th = twin.locate(ends, h, tau)
            assert 0.0 <= th <= 1.0
            H = hermite(ends[4], ends[5], ends[6], ends[7], h, th)
            g = hermite(ends[0], ends[1], ends[2], ends[3], h, th) + math.log(H) - tau
            assert abs(g) <= 1e-13, (ends, frac, th, g)


@pytest.mark.parametrize("method", ["rk4", "rkf"])
def test_crossings_on_the_power_law(method):
    """The attractor of V0 exp(-lam phi) with p = 8 from H_0 = 8: H = p / (1 + t), N = p ln(1 + t), so L = N (1 - 1 / p) + ln p and the
    crossing of tau lies at N = (tau - ln p) p / (p - 1) exactly.  Located N and states within 1e-8 at max_err = 1e-10, the bound of
    test_time_samples_on_the_power_law; epsilon_H = 1 / p."""
    art, p = power_law_artifact()
    twin = CrossingTwin(art)
    x0 = power_law_init()
    n_exact = np.array([0.0, 0.37, 2.0, 8.0])
    samples = n_exact * (1.0 - 1.0 / P_POW)
    out, meta = twin.solve(p, x0, np.concatenate([[-0.5], samples]), 100_000, offset=math.log(P_POW), method=method, max_err=1e-10, stop_at_end=True)
    assert meta["status"] == TARGET and meta["n_stored"] == 4 and meta["n_before"] == 1 and np.isnan(out[0]).all()
    got = out[1:]
    exact = power_law_exact(np.expm1(n_exact / P_POW))
    errs = np.max(np.abs(got[:, :6] - exact) / np.maximum(np.abs(exact), 1.0), axis=1)
    n_err = np.abs(got[:, 5] - n_exact)
    print(f"{method}: state errors {errs}, N errors {n_err}")
    assert errs.max() <= 1e-8 and n_err.max() <= 1e-8, (errs, n_err)
    assert np.max(np.abs(got[:, 6] - np.expm1(n_exact / P_POW))) <= 1e-8 and np.max(np.abs(got[:, 7] - 1.0 / P_POW)) <= 1e-8


def test_located_end_of_inflation(hyper):
    """inflx_hx_step_end on the twin: epsilon_H = 1 at the located state to the iteration's bracket (1e-15 in theta), the state against
    DOP853 with an exact event at max_err = 1e-10, and N_end within the dense output's order of inflx_bg_step_taken's linear rule."""
    art, p, twin, stepper = hyper
    eom = model_functions(workloads.model_for("hyperbolic"), art.symbol_dictionary)
    x, v = _hyper_batch(8, seed=3)
    for k in (1, 3, 5):
        init = np.concatenate([x[k], v[k]])
        for method in ("rk4", "rkf"):
            out, meta = twin.end(p, init, 100_000, method=method, max_err=1e-10)
            assert meta["status"] == ENDED and abs(out[7] - 1.0) <= 1e-12
            kin = stepper.eom(p, out[None, :4])[0, 3]
            assert out[7] == 0.5 * kin / out[4] ** 2
            sol = solve_ivp_reference(eom, p, init, 50.0, end_event=True)
            truth = np.concatenate([sol.y_events[0][0], sol.t_events[0]])
            err = np.max(np.abs(out[:7] - truth) / np.maximum(np.abs(truth), 1.0))
            _, linear = stepper.solve(p, init, 100_001, method=method, max_err=1e-10, stop_at_end=True)
            print(f"trajectory {k} {method}: located end against DOP853 {err:.2e}; N_end located {out[5]:.9f}, linear {linear['N_end']:.9f}")
            assert err <= 1e-7, err  # (the steppers' own error at max_err = 1e-10 over ~40 steps; the linear rule is off by 1e-5 .. 1e-4)
            assert meta["accepted"] == linear["accepted"] and abs(out[5] - linear["N_end"]) <= 1e-3
    past = np.array([3.0, 0.0, 5.0, 0.0])  # starts past the end
    out, meta = twin.end(p, past, 100)
    assert meta == dict(status=ENDED, accepted=0) and out[5] == 0.0 and out[6] == 0.0 and out[7] >= 1.0 and np.array_equal(out[:4], past)
    out, meta = twin.end(p, np.concatenate([x[3], v[3]]), 5)  # max_steps run out
    assert meta == dict(status=COMPLETE, accepted=5) and np.isnan(out).all()


def test_reheating_offset():
    from inflatox_amd.background import reheating_offset

    # both sides take CODATA's hbar c and k_B and the IAU's parsec in full: they differ by the order of their sums alone
    cases = [dict(), dict(k_mpc=0.002), dict(w_reh=0.0, N_reh=7.5), dict(w_reh=1.0, N_reh=3.0, g_reh=10.75, gs_reh=10.75), dict(k_mpc=1.0, w_reh=-0.3, N_reh=20.0, g_reh=200.0, gs_reh=90.0)]
    for kw in cases:
        assert abs(reheating_offset(**kw) - reheating_offset_restated(**kw)) <= 1e-12, kw
    assert abs(reheating_offset() - (-61.37)) <= 5e-3 and reheating_offset(0.05) == reheating_offset()
    assert reheating_offset(w_reh=1.0 / 3.0, N_reh=9.0) == reheating_offset()  # radiation-like reheating changes nothing
    for kw in (dict(k_mpc=0.0), dict(k_mpc=-1.0), dict(k_mpc=math.inf), dict(k_mpc=math.nan), dict(N_reh=-1e-9), dict(N_reh=math.inf), dict(w_reh=-1.0 / 3.0),
               dict(w_reh=1.0 + 1e-9), dict(w_reh=math.nan), dict(g_reh=0.0), dict(gs_reh=-3.0), dict(g_reh=math.inf), dict(k_mpc="x")):  # fmt: skip
        with pytest.raises(ValueError):
            reheating_offset(**kw)


def test_argument_checks_before_the_device(monkeypatch):
    """Every new function refuses bad arguments before the library is loaded or a code object built."""
    from inflatox_amd import background
    from inflatox_amd._native import InflatoxShapeError as shape

    spec, art = workloads.artifact_for("hyperbolic")
    p = np.asarray(spec.args, dtype=np.float64)

    def untouched(*_a, **_k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(background, "_dylib", untouched)
    monkeypatch.setattr(background, "_crossing_dylib", untouched)
    x, v = np.array([[3.0, 0.5], [3.0, 0.1]]), np.zeros((2, 2))
    value = ValueError
    for fn in (background.horizon_crossings, background.power_spectra_at_k, background.tensor_spectra_at_k, background.observables_at_k):
        for ln_k, err in (([], value), ([[0.0]], shape), ([0.0, math.nan], value), ([1.0, 1.0], value), ([2.0, 1.0], value), ("k", value)):
            with pytest.raises(err):
                fn(art, p, ln_k, x, v)
        for kw, err in ((dict(offset=[0.0]), shape), (dict(offset=math.inf), value), (dict(offset=np.zeros((2, 1))), shape), (dict(max_steps=0), value),
                        (dict(max_err=0.0), value), (dict(solver="euler"), value), (dict(dt=-1.0), value)):  # fmt: skip
            with pytest.raises(err):
                fn(art, p, [0.0], x, v, **kw)
        for args, err in (((p, [0.0], x[0], v[0]), shape), ((p, [0.0], x, v[:1]), shape), ((p[:-1], [0.0], x, v), shape), ((np.zeros((3, p.size)), [0.0], x, v), shape)):
            with pytest.raises(err):
                fn(art, *args)
    for fn in (background.power_spectra_at_k, background.tensor_spectra_at_k, background.observables_at_k):
        for kw in (dict(N_sub=0.0), dict(N_sub=math.nan), dict(N_eval=math.inf), dict(N_eval=5.0), dict(N_eval="x"), dict(stop_at_end=False)):
            with pytest.raises(value):
                fn(art, p, [0.0], x, v, **kw)
    for dlnk in (0.0, -0.5, math.nan, "x"):
        with pytest.raises(value):
            background.observables_at_k(art, p, [0.0], x, v, dlnk=dlnk)
    for kw, err in ((dict(max_steps=0), value), (dict(max_err=math.inf), value), (dict(solver="x"), value), (dict(dt=0.0), value)):
        with pytest.raises(err):
            background.inflation_end(art, p, x, v, **kw)
    for args in ((p, x[0], v[0]), (p, x, v[:1]), (p[:-1], x, v)):
        with pytest.raises(shape):
            background.inflation_end(art, *args)
    grid = ([[14.0, 19.0], [-1.0, 1.0]], 3, 2)
    for fn in (background.pivot_exit_map, background.pivot_observables_map):
        for args, kw, err in (((p, *grid, math.nan), {}, value), ((p, *grid, np.zeros((2, 3))), {}, shape), ((p, *grid, "A"), {}, value), ((p, grid[0], 0, 2, -60.0), {}, value),
                              ((p, [1.0, 2.0], 3, 2, -60.0), {}, shape), ((np.zeros((6, p.size)), *grid, -60.0), {}, shape), ((p, *grid, -60.0), dict(derivatives_init=(0.0,)), shape),
                              ((p, *grid, -60.0), dict(max_err=-1.0), value), ((p, *grid, -60.0), dict(solver="x"), value)):  # fmt: skip
            with pytest.raises(err):
                fn(art, *args, **kw)
    for kw in (dict(dlnk=0.0), dict(N_sub=-1.0)):
        with pytest.raises(value):
            background.pivot_observables_map(art, p, *grid, -60.0, **kw)


def test_public_names_and_unchanged_surface():
    import ctypes
    import inspect
    import re

    from inflatox_amd import _native, background
    from inflatox_amd.compiler import _BACKGROUND_SOURCES, _CROSSING_SOURCES, _DELTAN_SOURCES, KERNEL_GROUPS, CompilationArtifact

    names = {"horizon_crossings", "inflation_end", "power_spectra_at_k", "tensor_spectra_at_k", "observables_at_k", "reheating_offset", "pivot_exit_map",
             "pivot_observables_map", "CrossingSolution", "InflationEnd", "ExitPoints", "OUTSIDE_AT_START"}  # fmt: skip
    assert names <= set(background.__all__) and all(name in background.__doc__ for name in names - {"CrossingSolution", "InflationEnd", "ExitPoints", "OUTSIDE_AT_START"})
    assert background.CrossingSolution._fields == ("states", "N", "t", "eps_H", "ln_aH", "n_stored", "n_before", "N_end", "status")
    assert background.InflationEnd._fields == ("state", "N_end", "t_end", "eps_H", "status")
    assert background.OUTSIDE_AT_START == 9 and 9 in background.STATUS and 9 not in (background.LOCATED, background.PAST_SURFACE, background.ENDED_SHORT)
    sig = inspect.signature(background.horizon_crossings)
    assert list(sig.parameters) == ["artifact", "pars", "ln_k", "fields_init", "derivatives_init", "offset", "max_steps", "max_err", "solver", "dt", "stop_at_end"]
    assert sig.parameters["offset"].default is None and sig.parameters["stop_at_end"].default is True and sig.parameters["offset"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(background.power_spectra_at_k)
    assert list(sig.parameters)[:5] == ["artifact", "pars", "ln_k", "fields_init", "derivatives_init"] and sig.parameters["N_sub"].default == 5.0
    assert list(inspect.signature(background.tensor_spectra_at_k).parameters) == list(sig.parameters)
    assert inspect.signature(background.observables_at_k).parameters["dlnk"].default == 0.5
    sig = inspect.signature(background.reheating_offset)
    assert [q.default for q in sig.parameters.values()] == [0.05, 1.0 / 3.0, 0.0, 106.75, 106.75]
    assert list(inspect.signature(background.pivot_exit_map).parameters)[:7] == ["artifact", "pars", "start_stop", "N0", "N1", "A", "derivatives_init"]
    assert list(inspect.signature(background.pivot_observables_map).parameters)[5:8] == ["A", "dlnk", "N_sub"]
    assert callable(CompilationArtifact.ensure_crossing) and "crossing" not in KERNEL_GROUPS
    new = ("inflx_crossing_kernels.hip", "inflx_crossing.h", "inflx_crossing_abi.h")
    assert _CROSSING_SOURCES[:3] == new and set(_CROSSING_SOURCES[3:]) == {"inflx_deltan.h", "inflx_background.h", "inflx_background_abi.h"}
    csrc = os.path.join(ROOT, "inflatox_amd", "csrc")
    assert all(os.path.exists(os.path.join(csrc, f)) for f in _CROSSING_SOURCES)
    # no other object is built from the new files, so every existing object keeps its hash
    import inflatox_amd.compiler as compiler

    for name, sources in vars(compiler).items():
        if name.endswith("_SOURCES") and name != "_CROSSING_SOURCES":
            assert not set(sources) & set(new), name
    assert "inflx_deltan.h" in _DELTAN_SOURCES and "inflx_background.h" in _BACKGROUND_SOURCES
    assert list(_native.CROSSING_SIGNATURES) == ["inflx_solve_eom_crossings", "inflx_inflation_end"]
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inflx_hip_crossing.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(inflx_[a-z_0-9]+)\s*\(", text))) == ["inflx_inflation_end", "inflx_solve_eom_crossings"]
    assert '#include "inflx_hip_crossing.h"' in open(os.path.join(ROOT, "include", "inflx_hip.h")).read()
    assert len(_native.CROSSING_SIGNATURES["inflx_solve_eom_crossings"][1]) == 19 and len(_native.CROSSING_SIGNATURES["inflx_inflation_end"][1]) == 14
    others = set(_native.SIGNATURES) | set(_native.DELTAN_SIGNATURES) | set(_native.EVOLUTION_SIGNATURES) | set(_native.STOCHASTIC_SIGNATURES) | set(_native.DISTRIBUTION_SIGNATURES)
    assert not set(_native.CROSSING_SIGNATURES) & others
    _native.build_library()
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert hasattr(lib, "inflx_solve_eom_crossings") and hasattr(lib, "inflx_inflation_end")
    assert callable(_native.InflatoxDevLib.solve_eom_crossings) and callable(_native.InflatoxDevLib.inflation_end)
    assert re.search(r"#define INFLX_HX_ABI_VERSION 1\b", open(os.path.join(csrc, "inflx_crossing_abi.h")).read())
    assert re.search(r"#define INFLX_BG_ABI_VERSION 5\b", open(os.path.join(csrc, "inflx_background_abi.h")).read())
    assert re.search(r"#define INFLX_DN_ABI_VERSION 1\b", open(os.path.join(csrc, "inflx_deltan_abi.h")).read())


def test_twin_program_under_address_and_ub_sanitizers(tmp_path, hyper):
    """tests/crossing_twin.cpp as a stand-alone program (CROSSING_TWIN_MAIN) under ASan + UBSan on the CPU: two trajectories (one past
    the end of inflation at its start), seven targets with two before the start and one at it, both steppers, adaptive with stop_at_end
    and at a fixed dt with 300 steps, and the located end of inflation."""
    gxx = shutil.which("g++")
    assert gxx is not None
    _art, p, twin, _stepper = hyper
    exe = str(tmp_path / "crossing_twin")
    cmd = [gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DCROSSING_TWIN_MAIN",
           *CrossingTwin.compile_options(*twin.headers), CrossingTwin.SOURCES[-1], "-o", exe]  # fmt: skip
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe, *map(repr, p.tolist())], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    lines = run.stdout.strip().splitlines()
    assert len(lines) == 8 and all("before 2," in ln for ln in lines), run.stdout[-3000:]
    first, second = lines[:4], lines[4:]
    assert all("fixed 0: status 1," in ln and "end status 1," in ln for ln in first[0::2]) and all("fixed 1: status 0," in ln and "accepted 300;" in ln for ln in first[1::2])
    assert all("status 1, stored 1, before 2, accepted 0; end status 1, N_end 0.000000" in ln for ln in second[0::2])
    assert all("fixed 1: status" in ln and "end status 1, N_end 0.000000" in ln for ln in second[1::2])  # (no stop_at_end: the crossings run on)
