"""Super-horizon transfer functions on the host build (tests/transfer_twin.cpp compiles csrc/inflx_transfer.h for the CPU): two
independent truths, the properties the equations imply, the documented default and edge cases, and the front-end's argument checks.
The bounds against the truths are 1e-10 plus twice the twin's own recorded step-control error (profiles/background_transfer.json,
written by ``python tests/transfer_reference.py``): a margin for other libm and contraction choices, not for defects."""

import math

import numpy as np
import pytest

import background_truth as bt
import kinematics_reference as kr
import transfer_reference as tr
import workloads
from transfer_reference import COMPLETE, ENDED, NONFINITE, TARGET


@pytest.fixture(scope="module")
def hyper():
    spec, art = workloads.artifact_for("hyperbolic")
    return spec.args, tr.TransferTwin(art)


def _hyper_states(B, seed=0):
    """inflating states of the hyperbolic model (epsilon_H < 0.1) that roll towards phi0 = 1 and turn: 0.7 to 2.5 e-folds to the end"""
    return tr.hyper_states(B, seed)


@pytest.mark.parametrize("max_err", tr.MAX_ERRS)
@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_twin_against_the_field_basis_system(solver, max_err):
    """Truth (a): 17 states of the Cartesian plane, T_SS and T_RS at N = 0.05, 0.2, 0.5 against the k = 0 field-basis system, which
    knows neither omega nor mu_s2 nor the adiabatic-entropic split.  This is what fixes the signs and the orientation."""
    _pa, ca, _pp, cp, _ps, cs, a, b = tr.plane_case()
    sol = tr.TransferTwin(ca).solve(cp, tr.PLANE_SAMPLES, cs[:, :2], cs[:, 2:4], max_err=max_err, solver=solver, dq_dN=tr.PLANE_DQ, stop_at_end=False)
    assert np.all(sol.status == TARGET) and np.all(sol.n_stored == 4)
    assert np.all(sol.T_SS[:, 0] == 1.0) and np.all(sol.T_RS[:, 0] == 0.0)
    err, bound = tr.plane_error(sol, cs, a, b), tr.plane_bound(solver, max_err)
    print(f"plane {solver} max_err {max_err:g}: worst |twin - truth (a)| {err:.3e}, bound {bound:.3e}; |T_RS| up to {np.abs(sol.T_RS).max():.2f}")
    assert err <= bound
    assert np.abs(sol.T_RS).max() > 0.3  # (the source term is there to be seen: the opposite sign would miss by order one)


def test_the_opposite_source_sign_misses_truth_a_by_order_one():
    """-T_RS of the twin is nowhere near truth (a): the check above can tell the sign of the source term."""
    _pa, ca, _pp, cp, _ps, cs, a, b = tr.plane_case()
    sol = tr.TransferTwin(ca).solve(cp, tr.PLANE_SAMPLES, cs[:, :2], cs[:, 2:4], max_err=1e-10, dq_dN=tr.PLANE_DQ, stop_at_end=False)
    flipped = sol._replace(T_RS=-sol.T_RS)
    assert tr.plane_error(flipped, cs, a, b) > 0.5


@pytest.mark.parametrize("max_err", tr.MAX_ERRS)
@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", bt.GPU_MODELS)
def test_twin_against_truth_on_the_curved_zoo(name, solver, max_err):
    """Truth (b): 65 lanes, a parameter row per lane, the four e-fold samples of ``background_truth.samples_for``; no lane and no
    sample is left out, every status is TARGET and the truth is finite."""
    init, pars = (v[: tr.LANES] for v in bt.batch(name))
    samples, truth = tr.zoo_truth(name)
    assert truth.shape == (tr.LANES, 4, 4) and np.isfinite(truth).all()
    sol = tr.zoo_twin(name).solve(pars, samples, init[:, :2], init[:, 2:], max_err=max_err, solver=solver, stop_at_end=False)
    assert np.all(sol.status == TARGET) and np.all(sol.n_stored == 4)
    assert np.isfinite(sol.T_SS).all() and np.isfinite(sol.T_RS).all()
    err, bound = tr.zoo_error(sol, truth), tr.bound(name, solver, max_err)
    print(f"{name} {solver} max_err {max_err:g}: worst |twin - truth (b)| {err:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_entropic_mode_of_a_radial_trajectory_is_the_field_itself(solver):
    """Cartesian plane with a = b, a start on the X axis moving along it: the entropic direction is Y, whose equation is X's own,
    so with dq_dN = Xd0 / (H0 X0) q = X / X0: T_SS sqrt(eps / eps_star) = X(N) / X(0) against the same run's states, and no turn:
    T_RS = 0 exactly."""
    import masses_reference as mr

    _polar, cart = kr.plane_models()
    art = kr.host_artifact_of(cart)
    p = mr.parameter_row(art, a=0.8, b=0.8)
    x = np.array([[2.0, 0.0], [1.2, 0.0], [-2.5, 0.0]])
    v = np.array([[-0.3, 0.0], [0.25, 0.0], [0.1, 0.0]])
    H0 = np.sqrt((0.8 * x[:, 0] ** 2 / 2 + v[:, 0] ** 2 / 2) / 3)
    samples = np.array([0.0, 0.1, 0.3, 0.6])
    max_err = 1e-10
    sol = tr.TransferTwin(art).solve(p, samples, x, v, max_err=max_err, solver=solver, dq_dN=v[:, 0] / (H0 * x[:, 0]), stop_at_end=False)
    assert np.all(sol.status == TARGET)
    eps_star = sol.eps_H[:, :1]
    got = sol.T_SS * np.sqrt(sol.eps_H / eps_star)
    want = sol.states[:, :, 0] / x[:, :1]
    err = np.abs(got - want).max()
    print(f"{solver}: worst |T_SS sqrt(eps / eps_star) - X / X0| {err:.3e}")
    assert err <= tr.plane_bound(solver, max_err)
    assert np.all(sol.T_RS == 0.0) and np.abs(1 - want[:, -1]).min() > 0.05


def test_geodesic_has_no_transfer(hyper):
    """Hyperbolic model with theta' = 0: V does not depend on theta, the trajectory is a geodesic, cross is +-0 at every stage, so
    T_RS is +-0 at every sample and at the end of inflation."""
    p, twin = hyper
    x, v = _hyper_states(9)
    v[:, 1] = 0.0
    sol = twin.solve(p, [0.0, 0.05, 0.2, 50.0], x, v, stop_at_end=True)
    assert np.all(sol.status == ENDED) and np.all(sol.n_stored >= 2)
    reached = np.arange(4)[None, :] < sol.n_stored[:, None]
    assert np.all(sol.T_RS[reached] == 0.0) and np.all(np.isnan(sol.T_RS[~reached]))
    assert np.all(sol.T_RS_end == 0.0) and np.all(np.isfinite(sol.T_SS_end)) and np.all(sol.N_end > 0.2)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_polar_and_cartesian_charts_agree(solver):
    """One geometry, one potential, two charts of the same orientation (``kinematics_reference.plane_states``): T_SS and T_RS are
    scalars and agree within the truth bound."""
    pa, ca, pp, cp, ps, cs, _a, _b = tr.plane_case()
    max_err = 1e-10
    kw = dict(max_err=max_err, solver=solver, dq_dN=tr.PLANE_DQ, stop_at_end=False)
    polar = tr.TransferTwin(pa).solve(pp, tr.PLANE_SAMPLES, ps[:, :2], ps[:, 2:4], **kw)
    cart = tr.TransferTwin(ca).solve(cp, tr.PLANE_SAMPLES, cs[:, :2], cs[:, 2:4], **kw)
    assert np.all(polar.status == TARGET) and np.all(cart.status == TARGET)
    err = max(np.abs(polar.T_SS - cart.T_SS).max(), np.abs(polar.T_RS - cart.T_RS).max())
    print(f"{solver}: worst |polar - cartesian| {err:.3e}")
    assert err <= tr.plane_bound(solver, max_err)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_affine_in_dq_dN(hyper, solver):
    """The perturbation equations are linear in (q, u, r) and a fixed dt takes the same steps whatever they hold: the results for
    three values of dq_dN at one dt are affine in it to 1e-12."""
    p, twin = hyper
    x, v = _hyper_states(17)
    samples = [0.0, 0.02, 0.05, 0.1]
    d = (-0.7, 0.1, 1.3)
    a, b, c = (twin.solve(p, samples, x, v, max_steps=2000, solver=solver, dq_dN=dq, dt=2e-3, stop_at_end=False) for dq in d)
    assert all(np.all(s.status == TARGET) for s in (a, b, c))
    w = (d[1] - d[0]) / (d[2] - d[0])
    for name in ("T_SS", "T_RS"):
        fa, fb, fc = (getattr(s, name) for s in (a, b, c))
        assert np.abs(fb - (fa + w * (fc - fa))).max() <= 1e-12, name
    assert np.abs(c.T_SS - a.T_SS).max() > 1e-3 and np.abs(c.T_RS - a.T_RS).max() > 1e-5
    assert np.array_equal(a.states, c.states) and np.array_equal(a.t, c.t)


def _end_errors(twin, p, x, v, want, solver, T, n):
    sol = twin.solve(p, [1e3], x, v, max_steps=n, solver=solver, dt=T / n, stop_at_end=False)
    assert np.all(sol.status == COMPLETE) and np.all(sol.accepted == n)
    return np.abs(sol.final[:, 6:9] - want).max(axis=1)


# The coarser of the two step counts per stepper, chosen the way ``background_truth.BATCH_DRAW`` chooses its draws: the first of 20,
# 40, 80 at which every one of the 17 lanes of ``hyper_states`` (seed 0) has a ratio >= 14.5 to T = 1.  rkf: 20, the step counts of
# ``background_truth.order_ratios`` itself (ratios 30 .. 124).  rk4: 40 (14.6 .. 18.4); at 20 its fifth-order term is not yet small
# on 14 of the lanes (12.1 .. 22.2).
ORDER_N = {"rk4": 40, "rkf": 20}


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_fixed_step_is_fourth_order_in_the_perturbations(hyper, solver):
    """As ``background_truth.order_ratios`` does for the background: a fixed dt = T / n to T = 1 on 17 inflating lanes of the
    hyperbolic model, the end state's (q, u, r) against the three equations integrated by DOP853 at rtol 1e-13, and halving dt cuts
    every lane's error by >= 14.5; the error at the finer step is above 1e-10, far above the truth's own.

    What the ratios are: the Fehlberg stepper advances with its fourth-order weights, whose h^4 coefficient is small.  At dt = 1/20
    its error is led by the h^5 term and falls by 30 to 124 per halving, faster than fourth order; further down the two terms have
    comparable size and opposite sign on most of these lanes, the ratio dips (2 .. 26 at n = 40, 10 .. 17.5 at n = 80 to T = 0.5)
    and then climbs towards 16 from below, reaching 14 where the error has fallen to 1e-13 and rounding takes over.  RK4's ratio
    is 14.6 .. 18.4 at n = 40 and 15.6 .. 16.7 at n = 80.  (The zoo of tests/background_truth.py does not serve here: its lanes do
    not inflate, their velocity passes near zero, where omega and mu_s2 are singular, and neither stepper is in a regular regime
    at these step counts.)"""
    p, twin = hyper
    x, v = _hyper_states(17)
    g = tr.workload_rhs("hyperbolic")
    want = np.array([tr.truth_final(g, [*x[k], *v[k]], p, bt.T_ORDER) for k in range(17)])
    n = ORDER_N[solver]
    coarse, fine = (_end_errors(twin, p, x, v, want, solver, bt.T_ORDER, m) for m in (n, 2 * n))
    ratios = coarse / fine
    print(f"{solver}: error at n = {2 * n} {fine.min():.2e} .. {fine.max():.2e}, ratios {ratios.min():.2f} .. {ratios.max():.2f}")
    assert fine.min() > 1e-10 and ratios.min() >= 14.5, (ratios.min(), int(np.argmin(ratios)))


def test_default_dq_dN_is_the_documented_root():
    """u(0) / H0 of a run without dq_dN is the slowly decaying root, from mu_s2 and eps_H of the masses twin at the initial state;
    on the plane with a steep potential across the velocity the discriminant is negative and the real part is taken."""
    import masses_reference as mr

    for name in ("fuzz1", "shear"):
        init, pars = (v[:17] for v in bt.batch(name))
        sol = tr.zoo_twin(name).solve(pars, [1e3], init[:, :2], init[:, 2:], max_steps=0, stop_at_end=False)
        H0 = sol.final[:, 4]
        mass = mr.MassesTwin(bt.host_artifact(name)).masses(pars, np.concatenate([init, H0[:, None]], axis=1))
        want = np.array([tr.default_dq_dN(e, m) for e, m in zip(mass[4], mass[7])])
        assert np.allclose(sol.final[:, 7] / H0, want, rtol=1e-12, atol=1e-14), name
        assert np.all(sol.final[:, 6] == 1.0) and np.all(sol.final[:, 8] == 0.0)
    _polar, cart = kr.plane_models()
    art = kr.host_artifact_of(cart)
    p = mr.parameter_row(art, a=0.1, b=400.0)  # V_NN / H^2 ~ 400 * 3 / (0.1 * 4 / 2): far above 9 / 4
    x, v = np.array([[2.0, 0.0]]), np.array([[-0.05, 0.0]])
    sol = tr.TransferTwin(art).solve(p, [1e3], x, v, max_steps=0, stop_at_end=False)
    H0 = sol.final[0, 4]
    eps = 0.05**2 / 2 / H0**2
    assert (3 - eps) ** 2 - 4 * 400.0 / H0**2 < 0
    assert sol.final[0, 7] / H0 == pytest.approx(-(3 - eps) / 2, rel=1e-13)
    assert tr.default_dq_dN(0.01, 0.02) == pytest.approx(0.5 * (-(2.99) + math.sqrt(2.99**2 - 0.08)))


def test_a_lane_at_rest_is_nonfinite_with_nans(hyper):
    """kin = 0: a point has no direction.  The lane stops in init, emits nothing -- not even the sample at 0 -- and its neighbours
    are untouched."""
    p, twin = hyper
    x, v = _hyper_states(3)
    v[1] = 0.0
    sol = twin.solve(p, [0.0, 0.05], x, v, stop_at_end=True)
    assert sol.status[1] == NONFINITE and sol.n_stored[1] == 0
    for member in (sol.T_SS, sol.T_RS, sol.t, sol.N, sol.eps_H, sol.states):
        assert np.isnan(member[1]).all() and np.isfinite(member[[0, 2]]).all()
    assert np.isnan([sol.N_end[1], sol.T_SS_end[1], sol.T_RS_end[1]]).all()
    assert np.all(sol.status[[0, 2]] == TARGET)


def test_a_lone_sample_at_zero_runs_to_the_end(hyper):
    """``samples=[0.0]`` asks for the end values alone (``transfer_map``): the sample is emitted in init and the lane runs on to
    epsilon_H = 1; its end values are those of a run with further samples that it does not reach."""
    p, twin = hyper
    x, v = _hyper_states(5)
    lone = twin.solve(p, [0.0], x, v, stop_at_end=True)
    more = twin.solve(p, [0.0, 500.0], x, v, stop_at_end=True)
    assert np.all(lone.status == ENDED) and np.all(lone.n_stored == 1) and np.all(more.n_stored == 1)
    for name in ("N_end", "T_SS_end", "T_RS_end"):
        assert np.array_equal(getattr(lone, name), getattr(more, name)) and np.isfinite(getattr(lone, name)).all()
    assert np.all(lone.T_SS[:, 0] == 1.0) and np.all(lone.T_RS[:, 0] == 0.0)
    short = twin.solve(p, [0.0], x, v, max_steps=7, stop_at_end=True)
    assert np.all(short.status == COMPLETE) and np.isnan(short.T_RS_end).all()


def test_recorded_errors_are_anchored():
    """The bounds come from profiles/background_transfer.json, which tests/transfer_reference.py writes from the host build.  Two
    anchors keep a re-recording from widening them unseen: the file carries the hash of the stepper's code it was measured with,
    which must be the present code's, and every recorded value is at most 100 max_err^(4/5) -- step-control error scales as the
    accepted steps' local error, max_err, times their number, ~ max_err^(-1/5); the largest value recorded is 69 max_err^(4/5)
    (fuzz3, rkf), and a value past 100 is a regression of the stepper, not a new bound."""
    rec = tr.recorded()
    assert rec["stepper_code"] == tr.stepper_code_hash()
    values = {f"zoo/{k}": v for k, v in rec["zoo"].items()} | {f"plane/{k}": v for k, v in rec["plane"].items()} | {f"hyperbolic/{k}": v for k, v in rec["hyperbolic"].items()}
    assert len(values) == 32 + 4 + 2
    for key, value in values.items():
        max_err = float(key.rsplit("/", 1)[1])
        assert 0.0 < value <= 100.0 * max_err**0.8, (key, value)


def test_public_names():
    from inflatox_amd import _native, background

    assert {"transfer_functions", "transfer_map", "TransferSolution"} <= set(background.__all__)
    assert background.TransferSolution._fields == tr.TwinSolution._fields[:11]
    assert callable(_native.InflatoxDevLib.transfer_functions) and "inflx_transfer_functions" in _native.SIGNATURES


def test_bad_arguments_raise_before_the_device(monkeypatch):
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    monkeypatch.setattr(CompilationArtifact, "ensure_transfer", no_device)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = np.zeros((3, 2)) + 2.0, np.zeros((3, 2)) + 0.1
    good = [0.0, 0.5, 1.0]
    shape, value = _native.InflatoxShapeError, ValueError
    tf = background.transfer_functions
    for bad in ([0.5, 0.2, 1.0], [0.5, 0.5], [-0.1, 0.5], [0.1, float("nan")], [0.1, float("inf")], [], "abc"):
        with pytest.raises(value):
            tf(art, p, bad, x, v)
    with pytest.raises(shape):
        tf(art, p, [[0.1, 0.2]], x, v)
    for args in ((p[:2], good, x, v), (np.zeros((2, p.size)), good, x, v), (p, good, x, v[:2]), (p, good, np.zeros((3, 3)), np.zeros((3, 3)))):
        with pytest.raises(shape):
            tf(art, *args)
    for kw in (dict(max_steps=0), dict(max_steps=-1), dict(max_steps=2.5), dict(max_err=0.0), dict(max_err=-1e-6), dict(max_err=float("nan")), dict(solver="euler"),
               dict(dt=0.0), dict(dt=float("inf")), dict(dq_dN=float("nan")), dict(dq_dN=[0.1, float("inf"), 0.2]), dict(dq_dN="abc")):  # fmt: skip
        with pytest.raises(value):
            tf(art, p, good, x, v, **kw)
    for dq in ([0.1, 0.2], np.zeros((3, 1)), np.zeros(4)):
        with pytest.raises(shape):
            tf(art, p, good, x, v, dq_dN=dq)
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    with pytest.raises(shape):
        tf(three, np.zeros(3), good, x, v)
    tm = background.transfer_map
    with pytest.raises(value):
        tm(art, p, [[1.5, 4.0], [-1.0, 1.0]], 3, 3, dq_dN=float("inf"))
    for dq in ([0.1, 0.2], np.zeros((3, 4)), np.zeros((3, 3, 1))):
        with pytest.raises(shape):
            tm(art, p, [[1.5, 4.0], [-1.0, 1.0]], 3, 3, dq_dN=dq)
    with pytest.raises(value):
        tm(art, p, [[1.5, 4.0], [-1.0, 1.0]], 3, 3, dq_dN=np.full((3, 3), np.nan))
    with pytest.raises(value):
        tm(art, p, [[1.5, 4.0], [-1.0, 1.0]], 3, 3, N_star=-1.0)
