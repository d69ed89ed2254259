"""The delta-N stencils on the host build (tests/deltan_twin.cpp compiles csrc/inflx_deltan.h for the CPU): the twin against a second
spelling of the algorithm, against an independent truth with events, the exact power-law and Killing-direction cases, the formulas
of the reduction against sympy, the statuses, and the front end's argument checks.  The bounds against the truth are b = 1e-10 plus
twice the twin's own recorded error on N_members (profiles/background_deltan.json, written by ``python tests/deltan_reference.py``);
the derivatives' bounds are the propagated ones, b / h for N_,I and 4 b / h^2 for N_,IJ."""

import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import sympy as sp

import deltan_reference as dr
import workloads
from conftest import ROOT
from deltan_reference import COMPLETE, LOCATED, NONFINITE, PAST_SURFACE

H = dr.H_DEFAULT


@pytest.fixture(scope="module")
def hyper():
    c = dr.case("hyperbolic")
    return c, dr.case_twin("hyperbolic")


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_twin_is_the_restatement(hyper, solver):
    """One hyperbolic stencil at max_err = 1e-8, the twin against ``DeltaNRestatement`` on the host-compiled model function: the same
    number of accepted steps in phase A and for every member, H_c, N_c and N_members to 1e-12."""
    c, twin = hyper
    got = twin.delta_n(c.p, c.x[:1], c.v[:1], max_err=1e-8, solver=solver)
    assert got.dn.status[0] == LOCATED
    ref = dr.DeltaNRestatement(dr.host_eom(c.artifact), c.p)
    _g, geom = dr.case_functions("hyperbolic")
    states = dr.member_states(geom, c.p, c.x[0], c.v[0], (H, H), dr.FIXED)
    st, h_c, n_c, accepted = ref.end(states[4], solver, 1e-8)
    assert st == LOCATED and accepted == got.centre_accepted[0]
    assert abs(h_c - got.dn.H_end[0]) <= 1e-12 and abs(n_c - got.N_c[0]) <= 1e-12
    for m in range(9):
        st, n, accepted = ref.surface(states[m], got.dn.H_end[0], solver, 1e-8)
        assert st == LOCATED and accepted == got.accepted[0, m], (m, accepted, got.accepted[0, m])
        assert abs(n - got.dn.N_members[0, m // 3, m % 3]) <= 1e-12, (m, n)


@pytest.mark.parametrize("max_err", dr.MAX_ERRS)
@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", dr.CASES)
def test_twin_against_truth(name, solver, max_err):
    """N_members of three stencils per model against DOP853 with events; every centre's phase-B N is phase A's N_c to 1e-12; the
    stencils start 8 to 12 e-folds before the end."""
    c = dr.case(name)
    truth_n, truth_hc, truth_nc, _hs = dr.case_truth(name)
    assert np.isfinite(truth_n).all() and np.all((truth_nc > 8.0) & (truth_nc < 12.0)), truth_nc
    got = dr.case_twin(name).delta_n(c.p, c.x, c.v, velocity=c.velocity, max_err=max_err, solver=solver)
    assert np.all(got.dn.status == LOCATED) and np.all(got.member_status == LOCATED) and np.all(got.centre_status == LOCATED)
    err, b = dr.members_error(got.dn.N_members, truth_n), dr.bound(name, solver, max_err)
    print(f"{name} {solver} max_err {max_err:g}: worst |twin - truth| of N_members {err:.3e}, bound {b:.3e}; centre phase B - phase A "
          f"{np.abs(got.dn.N - got.N_c).max():.1e}")  # fmt: skip
    assert err <= b
    assert np.abs(got.dn.N - got.N_c).max() <= 1e-12 and np.array_equal(got.dn.N, got.dn.N_members[:, 1, 1])
    assert np.abs(got.dn.H_end - truth_hc).max() <= b  # (dH/dN = -eps H is below H < 1 on the surface: H_c errs by less than N_c)


@pytest.mark.parametrize("name", dr.CASES)
def test_outputs_are_the_formulas_on_the_twins_own_members(name):
    """Every derived output against ``formulas`` (numpy, G and Gamma from sympy) applied to the twin's own N_members: 1e-10 relative to
    max(|N_,IJ|, |Gamma| |grad N|) for the second derivatives, 1e-10 relative for the others."""
    c = dr.case(name)
    _g, geom = dr.case_functions(name)
    got = dr.case_twin(name).delta_n(c.p, c.x, c.v, velocity=c.velocity)
    h_star = dr.case_truth(name)[3]
    for b in range(c.x.shape[0]):
        G, gam, _up, _V = geom(*c.x[b], c.p)
        n_i, n_ij, cov, grad2, f_nl, p_zeta = dr.formulas(got.dn.N_members[b], G, gam, (H, H), h_star[b])
        scale = max(np.abs(n_ij).max(), np.abs(gam).max() * np.abs(n_i).max())
        assert np.allclose(got.dn.N_I[b], n_i, rtol=1e-10, atol=0) and np.abs(got.dn.N_IJ[b] - n_ij).max() <= 1e-10 * scale
        assert np.abs(got.dn.N_cov[b] - cov).max() <= 1e-10 * scale
        assert got.dn.grad2[b] == pytest.approx(grad2, rel=1e-10) and got.dn.P_zeta[b] == pytest.approx(p_zeta, rel=1e-9)
        assert abs(got.dn.f_NL[b] - f_nl) <= 1e-10 * scale / grad2 + 1e-10 * abs(f_nl)


def test_reduce_reproduces_a_quadratic(hyper):
    """Synthetic planes fed to the twin's reduce: N = a + b.d + d.C.d / 2 sampled at offsets that are exact in binary reproduces b and
    C to rounding, on a flat metric (the double-quadratic model: Gamma = 0, so N_;IJ = N_,IJ and |grad N|^2 = b.b)."""
    twin = dr.case_twin("double_quadratic")
    c = dr.case("double_quadratic")
    h = (2.0**-6, 2.0**-7)
    a, b, C = 9.5, np.array([-1.75, 0.375]), np.array([[0.5, -0.25], [-0.25, 1.5]])
    d = np.array([[[(i - 1) * h[0], (j - 1) * h[1]] for j in range(3)] for i in range(3)])
    n = a + d @ b + 0.5 * np.einsum("ijk,kl,ijl->ij", d, C, d)
    out, dn = twin.reduce(c.p, n[None], [[2.0, 1.0]], h, 0.5)
    assert dn.status[0] == LOCATED and np.array_equal(dn.N_members[0], n)
    assert np.allclose(dn.N_I[0], b, rtol=1e-13, atol=0) and np.allclose(dn.N_IJ[0], C, rtol=0, atol=1e-10) and np.array_equal(dn.N_cov[0], dn.N_IJ[0])
    up = b  # (G = 1)
    assert dn.grad2[0] == pytest.approx(b @ b, rel=1e-13) and dn.f_NL[0] == pytest.approx(5 / 6 * (up @ C @ up) / (b @ b) ** 2, rel=1e-9)
    assert dn.P_zeta[0] == pytest.approx((0.5 / (2 * math.pi)) ** 2 * (b @ b), rel=1e-13)


def test_reduce_covariant_term_on_the_hyperbolic_metric(hyper):
    """The same with the hyperbolic metric, against sympy: Gamma^phi_theta,theta = -L sinh(phi / L) cosh(phi / L), Gamma^theta_phi,theta
    = coth(phi / L) / L, G^theta,theta = 1 / (L sinh)^2."""
    c, twin = hyper
    L = float(c.p[int(c.artifact.symbol_dictionary["L"][5:-1])])
    phi = sp.Symbol("phi")
    x = np.array([1.25, 0.3])
    sh, ch = (float(f.subs(phi, x[0] / L)) for f in (sp.sinh(phi), sp.cosh(phi)))
    _g, geom = dr.case_functions("hyperbolic")
    G, gam, _up, _V = geom(*x, c.p)
    assert gam[0, 1, 1] == pytest.approx(-L * sh * ch, rel=1e-14) and gam[1, 0, 1] == pytest.approx(ch / (L * sh), rel=1e-14) and G[1, 1] == pytest.approx((L * sh) ** 2, rel=1e-14)
    h = (2.0**-6, 2.0**-6)
    b, C = np.array([-2.0, 0.5]), np.array([[0.25, 0.125], [0.125, -0.75]])
    d = np.array([[[(i - 1) * h[0], (j - 1) * h[1]] for j in range(3)] for i in range(3)])
    n = 11.0 + d @ b + 0.5 * np.einsum("ijk,kl,ijl->ij", d, C, d)
    _out, dn = twin.reduce(c.p, n[None], x[None], h, 1.0)
    want = np.array([[C[0, 0], C[0, 1] - ch / (L * sh) * b[1]], [0.0, C[1, 1] + L * sh * ch * b[0]]])
    want[1, 0] = want[0, 1]
    scale = max(np.abs(C).max(), np.abs(gam).max() * np.abs(b).max())
    assert np.abs(dn.N_cov[0] - want).max() <= 1e-10 * scale
    grad2 = b[0] ** 2 + b[1] ** 2 / (L * sh) ** 2
    up = np.array([b[0], b[1] / (L * sh) ** 2])
    assert dn.grad2[0] == pytest.approx(grad2, rel=1e-12) and dn.f_NL[0] == pytest.approx(5 / 6 * (up @ want @ up) / grad2**2, rel=1e-9)
    _n_i, _n_ij, cov, g2, f_nl, _pz = dr.formulas(n, G, gam, h, 1.0)
    assert np.abs(cov - want).max() <= 1e-10 * scale and g2 == pytest.approx(grad2, rel=1e-12) and f_nl == pytest.approx(dn.f_NL[0], rel=1e-9)


def power_law_checks(dn, x, b):
    """The exact case, shared with the GPU test: N_,phi = -1 / lam within b / h, every second derivative within 4 b / h^2, f_NL = 0
    within what that allows: |f_NL| <= (5/6) |N_,phiphi| / N_,phi^2."""
    import background_reference as br

    assert np.all(dn.status == LOCATED)
    phi1 = br.power_law_init()[0]
    t = np.exp(br.LAM * (x[:, 0, None, None] + (np.arange(3)[None, :, None] - 1) * H - phi1) / 2.0) + np.zeros((1, 1, 3))
    exact = br.P_POW * np.log(br.P_POW / dr.POWER_H_END / t)
    err = dr.members_error(dn.N_members, exact)
    print(f"power law: worst |N_members - exact| {err:.3e} (b = {b:.3e}); N_,phi + 1/lam {np.abs(dn.N_I[:, 0] + 1 / br.LAM).max():.2e} (b/h = {b / H:.2e}), "
          f"worst |N_,IJ| {np.abs(dn.N_IJ).max():.2e} (4b/h^2 = {4 * b / H**2:.2e}), worst |f_NL| {np.abs(dn.f_NL).max():.2e}")  # fmt: skip
    assert err <= b
    assert np.abs(dn.N_I[:, 0] + 1.0 / br.LAM).max() <= b / H and np.abs(dn.N_I[:, 1]).max() <= b / H
    assert np.abs(dn.N_IJ).max() <= 4 * b / H**2 and np.abs(dn.N_cov).max() <= 4 * b / H**2
    assert np.abs(dn.f_NL).max() <= 5 / 6 * (4 * b / H**2) / (1.0 / br.LAM - b / H) ** 2


def test_power_law_is_exact():
    """Explicit attractor velocities per member, H_end given (inflation never ends): N = -phi / lam + const."""
    art, p, x, vel, _h = dr.power_law_case()
    got = dr.DeltaNTwin(art).delta_n(p, x, vel, H_end=dr.POWER_H_END)
    power_law_checks(got.dn, x, 1e-10 + 2.0 * dr.recorded()["members"]["power_law/rkf/1e-10"])
    assert np.isnan(got.N_c).all() and np.all(got.dn.H_end == dr.POWER_H_END)


def killing_checks(dn, c, b):
    """theta is a Killing direction of the hyperbolic model and V does not depend on it: with the 'fixed' rule the three members of a
    row i are the same trajectory up to a shift in theta.  N_members agree along theta within b, so N_,theta <= b / h, N_,theta,theta and
    N_,phi,theta <= 4 b / h^2, and N_;theta,theta = L sinh cosh N_,phi within 4 b / h^2 plus the rounding of the connection term."""
    L = float(c.p[int(c.artifact.symbol_dictionary["L"][5:-1])])
    assert np.all(dn.status == LOCATED)
    spread = np.abs(dn.N_members - dn.N_members[:, :, 1:2]).max()
    print(f"hyperbolic: spread of N_members along theta {spread:.2e} (b = {b:.2e}); |N_,theta| {np.abs(dn.N_I[:, 1]).max():.2e}")
    assert spread <= b and np.abs(dn.N_I[:, 1]).max() <= b / H
    assert np.abs(dn.N_IJ[:, 1, 1]).max() <= 4 * b / H**2 and np.abs(dn.N_IJ[:, 0, 1]).max() <= 4 * b / H**2
    shch = L * np.sinh(c.x[:, 0] / L) * np.cosh(c.x[:, 0] / L)
    assert np.all(np.abs(dn.N_cov[:, 1, 1] - shch * dn.N_I[:, 0]) <= 4 * b / H**2 + 1e-10 * np.abs(shch * dn.N_I[:, 0]))


def test_hyperbolic_members_are_invariant_along_the_killing_direction(hyper):
    c, twin = hyper
    killing_checks(twin.delta_n(c.p, c.x, c.v).dn, c, dr.bound("hyperbolic", "rkf", 1e-10))


def singular_stencil():
    """The angular example model is singular on the unit circle.  With h = 2^-7 the stencil around (-1 + h, h) has its member 0 at
    (-1, 0) exactly and no other member on the circle: (centre x (2,), v (2,), h)."""
    h = 2.0**-7
    return np.array([-1.0 + h, h]), np.array([1e-7, 0.0]), h


def test_singular_stencil_has_exactly_one_member_that_is_not_finite():
    """Checked on the truth's right-hand side at the nine initial states, not on the code under test; then the twin: every derived
    output NaN, status NONFINITE + 16 x 0, and no N for that member."""
    import background_truth as bt

    spec, art = workloads.artifact_for("angular")
    model = workloads.model_for("angular")
    g = bt.truth_functions(model, art.symbol_dictionary)
    x, v, h = singular_stencil()
    p = np.asarray(spec.args, dtype=np.float64)
    states = dr.member_states(None, p, x, v, (h, h), dr.FIXED)
    assert states[0, 0] == -1.0 and states[0, 1] == 0.0

    def finite(s):
        try:
            with np.errstate(all="ignore"):
                return all(math.isfinite(w) for w in g(*s, p))
        except (ZeroDivisionError, OverflowError, ValueError):
            return False

    assert [finite(s) for s in states] == [False] + [True] * 8
    twin = dr.DeltaNTwin(art)
    got = twin.delta_n(p, x[None], v[None], h=h, H_end=1e-9, max_steps=2000)
    assert got.member_status[0, 0] == NONFINITE and got.accepted[0, 0] == 0  # (at init; what the other eight do is their own business)
    from inflatox_amd.background import delta_N_status

    code, member = (int(w) for w in delta_N_status(got.dn.status[0]))
    assert (code, member) == (NONFINITE, 0) and np.isnan(got.dn.N_members[0, 0, 0])
    assert all(np.isnan(getattr(got.dn, f)[0]).all() for f in ("N_I", "N_IJ", "N_cov", "grad2", "f_NL", "P_zeta"))


def test_statuses(hyper):
    """PAST_SURFACE: an H_end above the initial H stops every member at init.  max_steps exhausted: COMPLETE, from phase A (member 4)
    or, with H_end given, from member 0.  A good stencil beside a bad one is what it is alone, bit for bit."""
    from inflatox_amd.background import delta_N_status

    c, twin = hyper
    good = twin.delta_n(c.p, c.x, c.v)
    past = twin.delta_n(c.p, c.x, c.v, H_end=[100.0, float(good.dn.H_end[1]), 100.0])
    assert np.array_equal(delta_N_status(past.dn.status), ([PAST_SURFACE, LOCATED, PAST_SURFACE], [0, 0, 0]))
    assert np.all(past.member_status[[0, 2]] == PAST_SURFACE) and np.all(past.accepted[[0, 2]] == 0) and np.isnan(past.dn.N_members[[0, 2]]).all()
    assert np.isnan(past.dn.f_NL[[0, 2]]).all() and np.array_equal(past.out[:, 1], good.out[:, 1])
    short = twin.delta_n(c.p, c.x, c.v, max_steps=50)
    assert np.array_equal(delta_N_status(short.dn.status), ([COMPLETE] * 3, [4] * 3)) and np.all(short.centre_accepted == 50) and np.isnan(short.dn.H_end).all()
    assert np.all(short.member_status == NONFINITE) and np.isnan(short.out[:20]).all()
    short = twin.delta_n(c.p, c.x, c.v, max_steps=50, H_end=good.dn.H_end)
    assert np.array_equal(delta_N_status(short.dn.status), ([COMPLETE] * 3, [0] * 3)) and np.all(short.accepted == 50) and np.isnan(short.dn.N_members).all()
    # a centre that starts at the end of inflation: the surface is its own H, N = 0
    v_fast = np.array([[-2.0 * math.sqrt(0.5 * (c.x[0, 0] - 1.0) ** 2), 0.0]])  # kinetic = 2 V: eps_H = 3 K / (K + V) = 2 >= 1
    ended = twin.delta_n(c.p, c.x[:1], v_fast)
    assert ended.centre_status[0] == LOCATED and ended.centre_accepted[0] == 0 and ended.N_c[0] == 0.0
    assert ended.member_status[0, 4] == PAST_SURFACE and delta_N_status(ended.dn.status[0])[0] == PAST_SURFACE


def test_velocity_rules(hyper):
    """'slow_roll' gives every member chi^a = -G^ab d_b V / (3 H), H^2 = V / 3, at its own fields: the same run as explicit velocities
    computed from sympy, to rounding of the velocities (N_members within 1e-9: dN/dchi is of order 1 here); 'fixed' is explicit
    velocities all equal to the centre's, bit for bit."""
    c, twin = hyper
    _g, geom = dr.case_functions("hyperbolic")
    slow = twin.delta_n(c.p, c.x, None, velocity="slow_roll")
    vel = np.array([dr.member_states(geom, c.p, c.x[b], None, (H, H), dr.SLOW_ROLL)[:, 2:].reshape(3, 3, 2) for b in range(3)])
    explicit = twin.delta_n(c.p, c.x, vel)
    assert np.all(slow.dn.status == LOCATED) and np.abs(slow.dn.N_members - explicit.dn.N_members).max() <= 1e-9
    fixed = twin.delta_n(c.p, c.x, c.v)
    same = twin.delta_n(c.p, c.x, np.broadcast_to(c.v[:, None, None, :], (3, 3, 3, 2)))
    assert np.array_equal(fixed.out, same.out) and not np.array_equal(fixed.out[:9], slow.out[:9])


def test_parameter_rows_and_placement(hyper):
    """Stencil b uses parameter row b for all nine members; a stencil's outputs do not depend on its place in the batch."""
    c, twin = hyper
    rows = np.stack([c.p, c.p * [1.0, 1.0, 1.0], c.p * [1.1, 1.0, 0.9]])
    got = twin.delta_n(rows, c.x, c.v)
    one = twin.delta_n(c.p, c.x, c.v)
    assert np.array_equal(got.out[:, :2], one.out[:, :2]) and not np.array_equal(got.out[:, 2], one.out[:, 2])
    alone = twin.delta_n(rows[2], c.x[2:], c.v[2:])
    assert np.array_equal(alone.out[:, 0], got.out[:, 2])


def test_recorded_errors_are_anchored():
    """The bounds come from profiles/background_deltan.json, which tests/deltan_reference.py writes from the host build.  The file
    carries the hash of the stepper's code it was measured with, which must be the present code's, and every recorded error of
    N_members is at most 100 max_err^(4/5), the cap of the other background profiles."""
    rec = dr.recorded()
    assert rec["stepper_code"] == dr.stepper_code_hash()
    assert len(rec["members"]) == 3 * 2 * 2 + 1
    for key, value in rec["members"].items():
        assert 0.0 <= value <= 100.0 * float(key.rsplit("/", 1)[1]) ** 0.8, (key, value)
    assert set(rec["derivatives"]) == {f"{n}/{k}/{h:g}" for n in dr.CASES for k in ("located", "linear_end") for h in (1e-2, 1e-3, 1e-4)}


def test_public_names_and_unchanged_surface():
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import _DELTAN_SOURCES, _TENSOR_SOURCES, KERNEL_GROUPS, CompilationArtifact

    assert {"delta_N", "DeltaN", "fnl_map", "delta_N_status"} <= set(background.__all__)
    assert background.DeltaN._fields == ("N", "H_end", "N_members", "N_I", "N_IJ", "N_cov", "grad2", "f_NL", "P_zeta", "status")
    assert (background.LOCATED, background.PAST_SURFACE) == (LOCATED, PAST_SURFACE) == (_native.DN_LOCATED, _native.DN_PAST_SURFACE)
    assert {LOCATED, PAST_SURFACE} <= set(background.STATUS) and all(name in background.__doc__ for name in ("delta_N", "fnl_map"))
    assert callable(CompilationArtifact.ensure_deltan) and "deltan" not in KERNEL_GROUPS
    assert _DELTAN_SOURCES == ("inflx_deltan_kernels.hip", "inflx_deltan.h", "inflx_deltan_abi.h", "inflx_background.h", "inflx_background_abi.h")
    assert _DELTAN_SOURCES[3:] == _TENSOR_SOURCES[3:]
    # the C function: declared in the header that inflx_hip.h includes, bound in a table of its own, exported by the library
    import ctypes
    import re

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "inflx_hip_deltan.h")).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(inflx_[a-z_0-9]+)\s*\(", text))) == sorted(_native.DELTAN_SIGNATURES) == ["inflx_delta_n"]
    assert '#include "inflx_hip_deltan.h"' in open(os.path.join(ROOT, "include", "inflx_hip.h")).read()
    assert len(_native.DELTAN_SIGNATURES["inflx_delta_n"][1]) == 18 and not set(_native.DELTAN_SIGNATURES) & set(_native.SIGNATURES)
    _native.build_library()
    assert hasattr(ctypes.CDLL(_native.LIB_PATH), "inflx_delta_n") and callable(_native.InflatoxDevLib.delta_n)
    # the enums of the three layers agree
    header = open(os.path.join(ROOT, "inflatox_amd", "csrc", "inflx_deltan.h")).read()
    for name, value in (("INFLX_DN_LOCATED", 7), ("INFLX_DN_PAST_SURFACE", 8), ("INFLX_DN_FIXED", 0), ("INFLX_DN_SLOW_ROLL", 1), ("INFLX_DN_EXPLICIT", 2), ("INFLX_DN_NOUT", 21)):
        assert re.search(rf"\b{name} = {value},", header), name
    assert (_native.DN_FIXED, _native.DN_SLOW_ROLL, _native.DN_EXPLICIT, _native.DN_OUT_PLANES) == (0, 1, 2, 21)


def test_bad_arguments_raise_before_the_device(monkeypatch):
    from inflatox_amd import _native, background
    from inflatox_amd.compiler import CompilationArtifact

    def no_device(*a, **k):
        raise AssertionError("a device call was made")

    monkeypatch.setattr(background, "_dylib", no_device)
    for ensure in ("ensure_deltan", "ensure_background"):
        monkeypatch.setattr(CompilationArtifact, ensure, no_device)
    spec, art = workloads.artifact_for("hyperbolic")
    p = spec.args
    x, v = np.zeros((3, 2)) + 2.0, np.zeros((3, 2)) + 0.1
    shape, value = _native.InflatoxShapeError, ValueError
    three = CompilationArtifact({}, "/nonexistent/model.hsaco", 3, 3, auto_cleanup=False)
    for kw in (dict(max_steps=0), dict(max_steps=-1), dict(max_steps=2.5), dict(max_err=0.0), dict(max_err=-1e-6), dict(max_err=float("nan")), dict(solver="euler"),
               dict(dt=0.0), dict(dt=float("inf")), dict(h=0.0), dict(h=-1e-2), dict(h=float("nan")), dict(h=float("inf")), dict(h="abc"), dict(h=(1e-2, 0.0)),
               dict(velocity="attractor"), dict(velocity="explicit"), dict(H_end=0.0), dict(H_end=-1.0), dict(H_end=float("nan")), dict(H_end=[1.0, 2.0]),
               dict(H_end="abc")):  # fmt: skip
        with pytest.raises(value):
            background.delta_N(art, p, x, v, **kw)
    with pytest.raises(value):
        background.delta_N(art, p, x)  # 'fixed' needs the centres' velocities
    for args, kw in (((p[:2], x, v), {}), ((np.zeros((2, p.size)), x, v), {}), ((p, x, v[:2]), {}), ((p, np.zeros((3, 3)), np.zeros((3, 3))), {}),
                     ((p, x, np.zeros((3, 3, 3, 3))), {}), ((p, x, np.zeros((2, 3, 3, 2))), {}), ((p, x, v), dict(h=(1e-2, 1e-2, 1e-2))), ((p, x[0], v[0]), {})):  # fmt: skip
        with pytest.raises(shape):
            background.delta_N(art, *args, **kw)
    with pytest.raises(shape):
        background.delta_N(three, np.zeros(3), x, v)
    for kw in (dict(N_star=-1.0), dict(N_star=float("nan")), dict(N_star="abc"), dict(h=0.0), dict(h="abc"), dict(velocity="attractor"), dict(max_err=0.0),
               dict(solver="euler"), dict(max_steps=0)):  # fmt: skip
        with pytest.raises(value):
            background.fnl_map(art, p, [[1.5, 4.0], [-1.0, 1.0]], 3, 3, **kw)
    with pytest.raises(shape):
        background.fnl_map(art, p, [[1.5, 4.0], [-1.0, 1.0]], 3, 3, h=(1e-2, 1e-2, 1e-2))


def test_twin_program_under_address_and_ub_sanitizers(tmp_path):
    """tests/deltan_twin.cpp as a stand-alone program (DELTAN_TWIN_MAIN) under ASan + UBSan on the CPU: one stencil per velocity rule,
    both steppers, through phase A, phase B and the reduction."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ is not available")
    c, twin = dr.case("hyperbolic"), dr.case_twin("hyperbolic")
    exe = str(tmp_path / "deltan_twin")
    cmd = [gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DDELTAN_TWIN_MAIN",
           *twin.compile_options(*twin.headers), os.path.join(ROOT, "tests", "deltan_twin.cpp"), "-o", exe]  # fmt: skip
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe, *map(repr, c.p.tolist())], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and run.stdout.count("status 7") == 6, (run.stdout + run.stderr)[-3000:]
