"""The delta-N stencils on the GPU (inflatox_amd.background.delta_N, fnl_map, InflatoxDevLib.delta_n): N_members against the truth with
events on three models, the reduction against the formulas on the GPU's own N_members, batch shapes that leave a partial wavefront,
member planes that are not wave-aligned and planes that cross a workgroup, placement in the batch, parameter rows, a run whose
members stop in different launches, a stencil with a member that is not finite among good ones, PAST_SURFACE, exhausted steps, both
steppers, the exact power-law and Killing cases, and the refusal of an object of another layout.  Truth, twin and bounds are those
tests/test_background_deltan.py establishes on the host build (tests/deltan_reference.py, profiles/background_deltan.json): N_members
within b = 1e-10 + twice the twin's recorded error, N_,I within b / h, N_,IJ within 4 b / h^2.  Every difference is printed."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import deltan_reference as dr
import workloads
from deltan_reference import COMPLETE, LOCATED, NONFINITE, PAST_SURFACE
from test_background_deltan import killing_checks, power_law_checks, singular_stencil

pytestmark = pytest.mark.gpu

H = dr.H_DEFAULT
MEMBERS = ("N", "H_end", "N_members", "N_I", "N_IJ", "N_cov", "grad2", "f_NL", "P_zeta", "status")


@pytest.fixture(scope="module")
def bg():
    from inflatox_amd import background

    return background


@pytest.fixture(scope="module")
def hyper():
    return dr.case("hyperbolic")


def _same(a, b, rows=slice(None)):
    """the members of two DeltaN, bit for bit and NaN where NaN; ``rows`` selects from ``a``"""
    return all(np.array_equal(getattr(a, m)[rows], getattr(b, m), equal_nan=True) for m in MEMBERS)


def hyper_batch(B, seed=5):
    """B hyperbolic stencils 8 to 12 e-folds before the end ((phi - 1)^2 / 4 in [8.3, 11.7]), turning; the first three are the truth
    case's"""
    c = dr.case("hyperbolic")
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(6.8, 7.8, B), rng.uniform(-1, 1, B)], axis=1)
    v = np.stack([np.full(B, -0.8), rng.uniform(-2e-4, 2e-4, B)], axis=1)
    n = min(B, 3)
    x[:n], v[:n] = c.x[:n], c.v[:n]
    return x, v


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
@pytest.mark.parametrize("name", dr.CASES)
def test_members_against_truth(bg, name, solver):
    """Three stencils per model at the default max_err = 1e-10 against DOP853 with events; the derivatives against the same stencil of
    the truth's N within the propagated bounds."""
    c = dr.case(name, device=True)
    truth_n, truth_hc, _nc, h_star = dr.case_truth(name)
    _g, geom = dr.case_functions(name)
    dn = bg.delta_N(c.artifact, c.p, c.x, c.v, velocity=c.velocity, solver=solver)
    assert np.all(dn.status == LOCATED) and dn.status.dtype == np.int16
    twin = dr.case_twin(name).delta_n(c.p, c.x, c.v, velocity=c.velocity, solver=solver)
    err, b = dr.members_error(dn.N_members, truth_n), dr.bound(name, solver, 1e-10)
    print(f"{name} {solver}: worst |GPU - truth| of N_members {err:.3e} (b = {b:.3e}), |GPU - twin| {dr.members_error(dn.N_members, twin.dn.N_members):.3e}, "
          f"|H_end - truth| {np.abs(dn.H_end - truth_hc).max():.3e}")  # fmt: skip
    assert err <= b and np.abs(dn.H_end - truth_hc).max() <= b and np.array_equal(dn.N, dn.N_members[:, 1, 1])
    for k in range(c.x.shape[0]):
        G, gam, _up, _V = geom(*c.x[k], c.p)
        n_i, n_ij, cov, _g2, _f, p_zeta = dr.formulas(truth_n[k], G, gam, (H, H), h_star[k])
        assert np.abs(dn.N_I[k] - n_i).max() <= b / H and np.abs(dn.N_IJ[k] - n_ij).max() <= 4 * b / H**2
        assert np.abs(dn.N_cov[k] - cov).max() <= 4 * b / H**2 + np.abs(gam).max() * 2 * b / H
        assert dn.P_zeta[k] == pytest.approx(p_zeta, rel=4 * (b / H) / np.abs(n_i).max() + 1e-9)


@pytest.mark.parametrize("name", dr.CASES)
def test_reduce_outputs_are_the_formulas_on_the_gpus_own_members(bg, name):
    """1e-10 relative to max(|N_,IJ|, |Gamma| |grad N|), G and Gamma from sympy"""
    c = dr.case(name, device=True)
    _g, geom = dr.case_functions(name)
    dn = bg.delta_N(c.artifact, c.p, c.x, c.v, velocity=c.velocity)
    h_star = dr.case_truth(name)[3]
    for k in range(c.x.shape[0]):
        G, gam, _up, _V = geom(*c.x[k], c.p)
        n_i, n_ij, cov, grad2, f_nl, p_zeta = dr.formulas(dn.N_members[k], G, gam, (H, H), h_star[k])
        scale = max(np.abs(n_ij).max(), np.abs(gam).max() * np.abs(n_i).max())
        worst = max(np.abs(dn.N_IJ[k] - n_ij).max(), np.abs(dn.N_cov[k] - cov).max()) / scale
        print(f"{name} stencil {k}: second derivatives within {worst:.2e} of the formulas (relative to {scale:.3g}), f_NL {dn.f_NL[k]:.6f}")
        assert np.allclose(dn.N_I[k], n_i, rtol=1e-10, atol=0) and worst <= 1e-10
        assert dn.grad2[k] == pytest.approx(grad2, rel=1e-10) and dn.P_zeta[k] == pytest.approx(p_zeta, rel=1e-9)
        assert abs(dn.f_NL[k] - f_nl) <= 1e-10 * scale / grad2 + 1e-10 * abs(f_nl)
        assert np.array_equal(dn.N_IJ[k], dn.N_IJ[k].T) and np.array_equal(dn.N_cov[k], dn.N_cov[k].T)


@pytest.fixture(scope="module")
def batch257(bg, hyper):
    x, v = hyper_batch(257)
    dn = bg.delta_N(hyper.artifact, hyper.p, x, v)
    for a in dn:
        a.setflags(write=False)
    return x, v, dn


@pytest.mark.parametrize("B", [1, 5, 29, 257])
def test_batch_shapes(bg, hyper, batch257, B):
    """9 B lanes: B = 1 and 5 leave a partial wavefront, with B = 29 no member plane starts on a wavefront, with B = 257 every plane
    crosses a workgroup.  Every stencil is located, the three truth stencils are within b of the truth, and the first B stencils of
    the 257 are what the B-stencil batch gives, bit for bit."""
    x, v, big = batch257
    dn = bg.delta_N(hyper.artifact, hyper.p, x[:B], v[:B])
    assert dn.N_members.shape == (B, 3, 3) and dn.N_IJ.shape == (B, 2, 2) and dn.f_NL.shape == (B,)
    assert np.all(dn.status == LOCATED) and all(np.isfinite(m).all() for m in dn)
    n = min(B, 3)
    err, b = dr.members_error(dn.N_members[:n], dr.case_truth("hyperbolic")[0][:n]), dr.bound("hyperbolic", "rkf", 1e-10)
    print(f"B = {B}: worst |GPU - truth| of N_members {err:.3e} (b = {b:.3e}); N {dn.N.min():.2f} .. {dn.N.max():.2f}")
    assert err <= b and _same(big, dn, slice(0, B))


def test_placement_and_parameter_rows(bg, hyper, batch257):
    """A stencil alone, first, last or in the middle of a batch; one parameter row against the same row replicated."""
    x, v, big = batch257
    for k in (0, 63, 64, 128, 256):
        assert _same(big, bg.delta_N(hyper.artifact, hyper.p, x[k : k + 1], v[k : k + 1]), slice(k, k + 1)), k
    mid = bg.delta_N(hyper.artifact, hyper.p, x[100:131], v[100:131])
    assert _same(big, mid, slice(100, 131))
    rows = bg.delta_N(hyper.artifact, np.tile(hyper.p, (257, 1)), x, v)
    assert _same(big, rows)
    other = np.tile(hyper.p, (5, 1))
    other[3] *= [1.1, 1.0, 0.9]
    got = bg.delta_N(hyper.artifact, other, x[:5], v[:5])
    assert _same(big, bg.delta_N(hyper.artifact, hyper.p, x[:3], v[:3]), slice(0, 3)) and np.array_equal(got.N_members[[0, 1, 2, 4]], big.N_members[[0, 1, 2, 4]])
    assert _same(got, bg.delta_N(hyper.artifact, other[3], x[3:4], v[3:4]), slice(3, 4)) and not np.array_equal(got.N_members[3], big.N_members[3])


def test_members_of_one_stencil_stop_in_different_launches(bg, hyper):
    """One ``fnl_map`` of 4 x 3 at N_star = 55, with a wide stencil (h = 0.5) and max_err = 3.5e-10: the host twin from the same exit
    states takes about 512 accepted steps per member and every stencil has members on both sides of 512 -- they stop in the second
    and in the third launch of 256.  N_members of the first stencil against the truth from the same exit state, within 1e-10 plus
    twice the host twin's own error there; all against the twin within the same."""
    kw = dict(N_star=55.0, h=0.5, max_err=3.5e-10)
    dn, state, n_end, status = bg.fnl_map(hyper.artifact, hyper.p, [[16.6, 17.8], [-0.5, 0.5]], 4, 3, return_status=True, **kw)
    assert dn.f_NL.shape == (4, 3) and dn.N_members.shape == (4, 3, 3, 3) and dn.N_IJ.shape == (4, 3, 2, 2) and state.shape == (4, 3, 5)
    assert np.all(status == LOCATED) and np.array_equal(status, dn.status) and np.all(n_end >= 55.0)
    flat = state.reshape(-1, 5)
    twin = dr.case_twin("hyperbolic").delta_n(hyper.p, flat[:, :2], flat[:, 2:4], h=0.5, max_err=3.5e-10)
    lo, hi = twin.accepted.min(axis=1), twin.accepted.max(axis=1)
    print(f"accepted steps per member on the host: {lo.min()} .. {hi.max()}; stencils across 512: {int(np.sum((lo <= 512) & (hi > 512)))} of 12")
    assert np.all((lo <= 512) & (hi > 512))
    g, geom = dr.case_functions("hyperbolic")
    truth_n, _hc, _nc, _hs = dr.truth_members(g, geom, hyper.p, flat[0, :2], flat[0, 2:4], (0.5, 0.5), dr.FIXED)
    b = 1e-10 + 2.0 * dr.members_error(twin.dn.N_members[0], truth_n)
    err, diff = dr.members_error(dn.N_members[0, 0], truth_n), dr.members_error(dn.N_members.reshape(-1, 3, 3), twin.dn.N_members)
    print(f"fnl_map: |GPU - truth| of the first stencil's N_members {err:.3e} (bound {b:.3e}), worst |GPU - twin| over the map {diff:.3e}; "
          f"f_NL {np.nanmin(dn.f_NL):.5f} .. {np.nanmax(dn.f_NL):.5f}, N {dn.N.min():.3f} .. {dn.N.max():.3f}")  # fmt: skip
    assert err <= b and diff <= b
    again = bg.delta_N(hyper.artifact, hyper.p, flat[:, :2], flat[:, 2:4], h=0.5, max_err=3.5e-10)
    assert all(np.array_equal(getattr(again, m), getattr(dn, m).reshape(getattr(again, m).shape)) for m in MEMBERS)


def test_a_member_that_is_not_finite_spoils_its_stencil_alone(bg):
    """The angular example model next to its singular circle (``singular_stencil``: member 0 at (-1, 0) exactly, the only one whose
    right-hand side is not finite at the start), in the middle of six good stencils -- 63 lanes, one wavefront: it returns NaN with
    status NONFINITE + 16 x 0, and the six are bit for bit what they are without it."""
    spec, art = workloads.artifact_for("angular")
    p = np.asarray(spec.args, dtype=np.float64)
    xs, vs, h = singular_stencil()
    good = np.array([[0.5, 0.3], [-0.4, 0.6], [0.2, -0.7], [0.45, 0.35], [-0.35, 0.55], [0.25, -0.65]])
    h0 = np.sqrt(p[0] / 2 * ((p[2] * good[:, 0]) ** 2 + (p[1] * good[:, 1]) ** 2) / 3.0)  # sqrt(V / 3): H at rest
    x = np.concatenate([good[:3], xs[None], good[3:]])
    v = np.concatenate([np.zeros((3, 2)), vs[None], np.zeros((3, 2))])
    h_end = np.concatenate([0.9 * h0[:3], [1e-9], 0.9 * h0[3:]])
    dn = bg.delta_N(art, p, x, v, h=h, H_end=h_end, max_steps=2000)
    code, member = bg.delta_N_status(dn.status)
    assert code.tolist() == [LOCATED] * 3 + [NONFINITE] + [LOCATED] * 3 and member.tolist() == [0] * 7
    assert np.isnan(dn.N_members[3, 0, 0]) and all(np.isnan(getattr(dn, m)[3]).all() for m in ("N_I", "N_IJ", "N_cov", "grad2", "f_NL", "P_zeta"))
    keep = [0, 1, 2, 4, 5, 6]
    assert all(np.isfinite(getattr(dn, m)[keep]).all() for m in MEMBERS)
    assert _same(dn, bg.delta_N(art, p, x[keep], v[keep], h=h, H_end=h_end[keep], max_steps=2000), keep)
    twin = dr.DeltaNTwin(art).delta_n(p, x, v, h=h, H_end=h_end, max_steps=2000)
    assert np.array_equal(twin.dn.status, dn.status)


@pytest.mark.parametrize("solver", ["rk4", "rkf"])
def test_statuses(bg, hyper, solver):
    """PAST_SURFACE with an H_end above the initial H; max_steps exhausted in phase A (the centre, member 4) and in phase B (member
    0); a good stencil between two bad ones is what it is alone."""
    x, v = hyper.x, hyper.v
    good = bg.delta_N(hyper.artifact, hyper.p, x, v, solver=solver)
    assert np.all(good.status == LOCATED)
    past = bg.delta_N(hyper.artifact, hyper.p, x, v, solver=solver, H_end=[100.0, float(good.H_end[1]), 100.0])
    assert np.array_equal(bg.delta_N_status(past.status), ([PAST_SURFACE, LOCATED, PAST_SURFACE], [0, 0, 0]))
    assert np.isnan(past.N_members[[0, 2]]).all() and np.isnan(past.f_NL[[0, 2]]).all() and np.array_equal(past.H_end, [100.0, good.H_end[1], 100.0])
    assert all(np.array_equal(getattr(past, m)[1], getattr(good, m)[1]) for m in MEMBERS)
    short = bg.delta_N(hyper.artifact, hyper.p, x, v, solver=solver, max_steps=50)
    assert np.array_equal(bg.delta_N_status(short.status), ([COMPLETE] * 3, [4] * 3)) and np.isnan(short.H_end).all() and np.isnan(short.N_members).all()
    short = bg.delta_N(hyper.artifact, hyper.p, x, v, solver=solver, max_steps=300, H_end=good.H_end)  # (more than one launch)
    assert np.array_equal(bg.delta_N_status(short.status), ([COMPLETE] * 3, [0] * 3) if solver == "rk4" else ([LOCATED] * 3, [0] * 3))
    if solver == "rkf":  # (rkf needs 236 to 272 steps here: it is done in the second launch, and with H_end given it is the full run bit for bit)
        assert np.array_equal(short.N_members, good.N_members)


def test_velocity_rules_and_fixed_step(bg, hyper):
    """'slow_roll' against the twin (the velocities are computed on the device: N_members within 1e-9 of the host's, see the host
    test); explicit velocities equal to the centre's are the 'fixed' run bit for bit; a fixed dt runs and is located."""
    x, v = hyper.x, hyper.v
    slow = bg.delta_N(hyper.artifact, hyper.p, x, velocity="slow_roll")
    twin = dr.case_twin("hyperbolic").delta_n(hyper.p, x, None, velocity="slow_roll")
    assert np.all(slow.status == LOCATED) and dr.members_error(slow.N_members, twin.dn.N_members) <= 1e-9
    fixed = bg.delta_N(hyper.artifact, hyper.p, x, v)
    assert _same(fixed, bg.delta_N(hyper.artifact, hyper.p, x, np.broadcast_to(v[:, None, None, :], (3, 3, 3, 2))))
    stepped = bg.delta_N(hyper.artifact, hyper.p, x, v, dt=1e-2, max_steps=5000)
    assert np.all(stepped.status == LOCATED) and dr.members_error(stepped.N_members, fixed.N_members) <= 1e-6


def test_power_law_is_exact(bg):
    art, p, x, vel, _h = dr.power_law_case(device=True)
    dn = bg.delta_N(art, p, x, vel, H_end=dr.POWER_H_END)
    power_law_checks(dn, x, 1e-10 + 2.0 * dr.recorded()["members"]["power_law/rkf/1e-10"])
    assert np.all(dn.H_end == dr.POWER_H_END)


def test_hyperbolic_members_are_invariant_along_the_killing_direction(bg, hyper):
    killing_checks(bg.delta_N(hyper.artifact, hyper.p, hyper.x, hyper.v), hyper, dr.bound("hyperbolic", "rkf", 1e-10))


def test_deltan_object_of_another_layout_is_refused(bg):
    """An object built with -DINFLX_DN_ABI_VERSION=2 is refused with INFLX_ERR_VERSION, a missing one is INFLX_ERR_SYMBOL with the way
    to build it; the artefact's own build then replaces the refused file and works on the same handle."""
    from inflatox_amd import _native
    from inflatox_amd.compiler import _CSRC, hipcc_path

    art, p, x, vel, _h = dr.power_law_case(device=True)
    header_text, options, tag = art._build
    stale = art.shared_object_path + ".deltan"
    headers = {stale + ".model.h": header_text, stale + ".eom.h": art.eom_header_text()}
    centre = np.ascontiguousarray(np.concatenate([x[:1], vel[:1, 1, 1]], axis=1))
    vel9 = np.ascontiguousarray(vel[:1].reshape(1, 9, 2))
    p = np.ascontiguousarray(p, dtype=np.float64)
    h_end = np.array([dr.POWER_H_END])
    out, status = np.empty((21, 1)), np.empty(1, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    args = (vel9, _native.DN_EXPLICIT, H, H, h_end, 100_000, _native.EOM_RKF, 1e-10, 0.0)

    def raw(lib):  # the C entry point's own return code
        return lib._lib.inflx_delta_n(lib._h, p.ctypes.data_as(dp), 1, lib.n_parameters, centre.ctypes.data_as(dp), 1, vel9.ctypes.data_as(dp), _native.DN_EXPLICIT, H, H,
                                      h_end.ctypes.data_as(dp), 100_000, _native.EOM_RKF, 1e-10, 0.0, out.ctypes.data_as(dp), None, status.ctypes.data_as(C.POINTER(C.c_int32)))  # fmt: skip

    try:
        if os.path.exists(stale):
            os.remove(stale)
        lib = _native.InflatoxDevLib(art.shared_object_path)
        assert raw(lib) == _native.ERR_SYMBOL
        with pytest.raises(SystemError, match=r"ensure_deltan\(\)") as err:
            lib.delta_n(p, centre, *args)
        assert ".deltan exists" in str(err.value)
        for path, text in headers.items():
            with open(path, "w") as fh:
                fh.write(text)
        hdr, eom_hdr = headers
        cmd = [hipcc_path(), *options, "-DINFLX_DN_ABI_VERSION=2", f'-DINFLX_MODEL_TAG="{tag}"', f"-I{_CSRC}", f'-DINFLX_MODEL_HEADER="{hdr}"',
               f'-DINFLX_EOM_HEADER="{eom_hdr}"', os.path.join(_CSRC, "inflx_deltan_kernels.hip"), "-o", stale]  # fmt: skip
        subprocess.run(cmd, check=True)
        assert raw(lib) == _native.ERR_VERSION
        with pytest.raises(SystemError, match="does not belong") as err:
            lib.delta_n(p, centre, *args)
        assert "INFLX_DN_ABI 2, expected 1" in str(err.value)
        os.remove(stale)
        art.ensure_deltan()
        got = lib.delta_n(p, centre, *args)
        assert got[0].shape == (21, 1) and got[2][0] == LOCATED and np.isfinite(got[0]).all() and got[1][0, 0] == dr.POWER_H_END and np.isnan(got[1][1, 0])
        # arguments are checked before the device: a velocity array without the explicit rule, a stencil step of 0
        for bad in ((vel9, _native.DN_FIXED, H, H), (None, _native.DN_EXPLICIT, H, H), (vel9, _native.DN_EXPLICIT, 0.0, H), (vel9, 3, H, H)):
            with pytest.raises(Exception, match="rule|stencil steps"):
                lib.delta_n(p, centre, *bad, *args[4:])
        lib.close()
    finally:
        for path in (stale, *headers):
            if os.path.exists(path):
                os.remove(path)


@pytest.mark.parametrize("h_end", [None, 0.55], ids=["both-phases", "H_end"])
def test_more_than_one_pass_lands_behind_the_first_in_every_plane(bg, hyper, h_end):
    """A pass holds floor(2^20 / 9) = 116 508 stencils: B = 116 508 + 3 takes two, five fixed steps of dt = 0.1 each from centres
    0.1 e-folds before the end of inflation (H = 0.55 there), once with the centres' own search for the surface and once with
    ``H_end`` given.  The first five stencils, those on either side of the seam and the last five are the same stencils run alone,
    bit for bit and NaN where NaN, in ``out``, ``surface`` and ``status`` of ``InflatoxDevLib.delta_n``; stencils on both sides of
    the seam are LOCATED."""
    from inflatox_amd import _native

    first, B = 116_508, 116_508 + 3
    rng = np.random.default_rng(6)
    x = np.stack([rng.uniform(2.2, 2.3, B), rng.uniform(-1, 1, B)], axis=1)
    v = np.stack([-(x[:, 0] - 1) / (3 * np.sqrt((x[:, 0] - 1) ** 2 / 6)), rng.uniform(-1e-2, 1e-2, B)], axis=1)
    centre = np.concatenate([x, v], axis=1)
    hyper.artifact.ensure_deltan()
    lib = bg._dylib(hyper.artifact, background=False)

    def run(sl):
        surface = None if h_end is None else np.full(len(centre[sl]), h_end)
        return lib.delta_n(hyper.p, np.ascontiguousarray(centre[sl]), None, _native.DN_FIXED, H, H, surface, 5, _native.EOM_RKF, 1e-10, 0.1)

    out, surface, status = run(slice(None))
    print(f"statuses {np.unique(status, return_counts=True)}")
    assert out.shape == (21, B) and surface.shape == (2, B) and status.shape == (B,)
    assert (status[first - 3 : first] == LOCATED).any() and (status[first:] == LOCATED).any() and np.isfinite(out[:, status == LOCATED]).all()
    assert np.isnan(surface[1]).all() if h_end else np.isfinite(surface[:, status == LOCATED]).all()
    for sl in (slice(0, 5), slice(first - 3, first + 3), slice(B - 5, B)):
        o, s, st = run(sl)
        assert np.array_equal(out[:, sl], o, equal_nan=True) and np.array_equal(surface[:, sl], s, equal_nan=True) and np.array_equal(status[sl], st), sl
