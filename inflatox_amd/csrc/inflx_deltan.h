// The delta-N expansion: first and second derivatives of the e-fold count N with respect to the initial fields, and the local
// non-Gaussianity f_NL built from them (inflatox_amd.background.delta_N).
//
//     zeta = N_,I dphi^I + 1/2 N_,IJ dphi^I dphi^J,    N = e-folds from a flat slice at horizon exit to a surface of uniform density.
//
// A call has B stencils of 9 members: member m = 3 i + j, i, j in {0, 1, 2}, starts at the centre's fields plus the offsets
// ((i - 1) h_0, (j - 1) h_1); m = 4 is the centre.  Every member is one lane of csrc/inflx_background.h's stepper with that stepper's
// own per-lane step control -- nothing is shared across a stencil but the surface all nine stop on:
//   phase A (centres only, skipped when the caller gives H_end): the lane runs until the first accepted step with epsilon_H >= 1;
//           theta in (0, 1] with epsilon_H(y(theta)) = 1 is located on the step's Hermite dense output (inflx_bg_hermite), epsilon_H
//           evaluated through the model (inflx_bg_located_epsilon), by the Illinois iteration inside a bracket; H_c = H(theta) and
//           N_c = N(theta) come from the same interpolant.
//   phase B (all nine): a lane stops in the first accepted step with H_1 <= H_c < H_0; theta is inflx_bg_locate's bracketed Newton
//           iteration on the interpolant of H (H falls: the iteration runs on -H), and the lane's result is N(theta).
// Both events are located to the dense output's order, O(h^4), the order of the steppers' states: that, and a surface common to the
// stencil, is what a difference quotient of N needs.
//
// The reduction of one stencil (inflx_dn_reduce) takes central differences of the nine N and contracts them with the metric and the
// connection at the centre, both probed from inflx_eom_point.
//
// Everything is INFLX_FN code over one lane's registers, so that tests/deltan_twin.cpp compiles the very same code for the host.
#pragma once

// statuses of a delta-N lane beyond InflxBgStatus (0..5; 6 is taken by inflatox_amd.background.ENDED_SHORT)
enum InflxDnStatus {
  INFLX_DN_LOCATED = 7,       // the lane stopped on its surface: the located value is its result
  INFLX_DN_PAST_SURFACE = 8,  // phase B: the initial H is already <= H_c
};

// how a member's initial velocity follows from its fields
enum InflxDnVelocity {
  INFLX_DN_FIXED = 0,      // every member takes the centre's given coordinate velocity
  INFLX_DN_SLOW_ROLL = 1,  // every member, the centre included: chi^a = -G^ab d_b V / (3 H), H^2 = V / 3
  INFLX_DN_EXPLICIT = 2,   // the caller supplies the velocity of every member
};

#define INFLX_DN_MEMBERS 9
#define INFLX_DN_CENTRE 4
#define INFLX_DN_STATUS_STRIDE 16  // a stencil that failed: status = the member's status + 16 x the member's index

// outputs of one stencil (inflx_dn_reduce), in this order
enum InflxDnOut {
  INFLX_DN_OUT_MEMBERS = 0,  // 0..8: N of every member
  INFLX_DN_OUT_NI = 9,       // N_,0  N_,1
  INFLX_DN_OUT_NIJ = 11,     // N_,00  N_,11  N_,01
  INFLX_DN_OUT_NCOV = 14,    // N_;00  N_;11  N_;01
  INFLX_DN_OUT_GRAD2 = 17,   // G^IJ N_,I N_,J
  INFLX_DN_OUT_FNL = 18,
  INFLX_DN_OUT_PZETA = 19,
  INFLX_DN_OUT_STATUS = 20,
  INFLX_DN_NOUT = 21,
};

// the initial fields and velocity of member m: init[0..3]
INFLX_FN void inflx_dn_member(const double* centre, double h0, double h1, int m, int rule, const double* explicit_v, const double* __restrict__ p,
                              double* init) {
  const int i = m / 3, j = m % 3;
  init[0] = centre[0] + (double)(i - 1) * h0;
  init[1] = centre[1] + (double)(j - 1) * h1;
  if (rule == INFLX_DN_SLOW_ROLL) {
    double o[4];
    inflx_eom_point(init[0], init[1], 0.0, 0.0, p, o);  // o[0..1] = G^ab d_b V, o[2] = V
    const double h3 = 3.0 * sqrt(o[2] / 3.0);
    init[2] = -o[0] / h3;
    init[3] = -o[1] / h3;
  } else if (rule == INFLX_DN_EXPLICIT) {
    init[2] = explicit_v[0];
    init[3] = explicit_v[1];
  } else {
    init[2] = centre[2];
    init[3] = centre[3];
  }
}

// inflx_bg_init for a delta-N lane.  Phase A (h_c = NaN: none yet): a centre that starts at or past the end of inflation is located
// there, H_c = H_0 and N_c = 0.  Phase B: a lane whose H_0 is already <= h_c is INFLX_DN_PAST_SURFACE.  `result` is N_c / the lane's N
// on the surface (NaN unless INFLX_DN_LOCATED).
INFLX_FN int inflx_dn_init(InflxBgLane& s, const double* init, const double* __restrict__ p, double dt0, bool phase_a, double h_c, double& result) {
  double n_end = 0.0;
  const int st = inflx_bg_init(s, init, p, dt0, false, n_end);
  if (st != INFLX_BG_RUNNING) return st;
  if (phase_a) {
    if (inflx_bg_epsilon(s) >= 1.0) {
      result = 0.0;
      return INFLX_DN_LOCATED;
    }
    return INFLX_BG_RUNNING;
  }
  if (!isfinite(h_c)) return INFLX_BG_NONFINITE;  // (the centre found no surface: its own status is the stencil's)
  return s.y[4] <= h_c ? (int)INFLX_DN_PAST_SURFACE : (int)INFLX_BG_RUNNING;
}

// the state of the dense output at theta, and epsilon_H there through the model; false: not finite
INFLX_FN bool inflx_dn_dense_epsilon(const double* y0, const double* f0, const double* y1, const double* f1, double h, double th, const double* __restrict__ p,
                                     InflxBgLocated& loc) {
  for (int c = 0; c < 6; ++c) loc.y[c] = inflx_bg_hermite(y0[c], f0[c], y1[c], f1[c], h, th);
  loc.t = th;
  return inflx_bg_located_epsilon(loc, p);
}

// theta in (0, 1] with epsilon_H(y(theta)) = 1 for epsilon_H(0) = eps0 < 1 <= eps1 = epsilon_H(1): the Illinois iteration (a secant
// step inside the bracket [lo, hi], g(lo) < 0 <= g(hi); the end that stays twice has its g halved), an iterate that leaves the
// bracket replaced by the midpoint.  At most INFLX_BG_MAX_LOCATE iterations; stops at g == 0 or a bracket <= 1e-15.  `loc` is the
// state at the theta returned; false: an iterate was not finite.
INFLX_FN bool inflx_dn_locate_end(const double* y0, const double* f0, const double* y1, const double* f1, double h, double eps0, double eps1,
                                  const double* __restrict__ p, double& theta, InflxBgLocated& loc) {
  double lo = 0.0, hi = 1.0, glo = eps0 - 1.0, ghi = eps1 - 1.0;
  double th = 1.0;
  int side = 0;
  if (ghi == 0.0) {
    theta = th;
    return inflx_dn_dense_epsilon(y0, f0, y1, f1, h, th, p, loc);
  }
  for (int it = 0; it < INFLX_BG_MAX_LOCATE; ++it) {
    th = (lo * ghi - hi * glo) / (ghi - glo);
    if (!(th > lo && th < hi)) th = 0.5 * (lo + hi);
    if (!inflx_dn_dense_epsilon(y0, f0, y1, f1, h, th, p, loc)) return false;
    const double g = loc.eps - 1.0;
    if (g == 0.0) break;
    if (g < 0.0) {
      lo = th;
      glo = g;
      if (side == -1) ghi *= 0.5;
      side = -1;
    } else {
      hi = th;
      ghi = g;
      if (side == 1) glo *= 0.5;
      side = 1;
    }
    if (hi - lo <= 1e-15) break;
  }
  theta = th;
  return true;
}

// Phase A: one accepted step of a centre; when the new state has epsilon_H >= 1 the lane stops with INFLX_DN_LOCATED, h_c = H and
// n_c = N of the dense output where epsilon_H = 1.
template <int METHOD>
INFLX_FN int inflx_dn_step_end(InflxBgLane& s, const double* __restrict__ p, double max_err, double fixed_dt, double& h_c, double& n_c) {
  double y0[6], f0[6], h = 0.0, n_end = 0.0;
  for (int c = 0; c < 6; ++c) {
    y0[c] = s.y[c];
    f0[c] = s.f[c];
  }
  const double eps0 = inflx_bg_epsilon(s);
  const int st = inflx_bg_step_taken<METHOD>(s, p, max_err, fixed_dt, false, n_end, h);
  if (st != INFLX_BG_RUNNING) return st;
  const double eps1 = inflx_bg_epsilon(s);
  if (!(eps1 >= 1.0)) return INFLX_BG_RUNNING;
  double th = 1.0;
  InflxBgLocated loc;
  if (!inflx_dn_locate_end(y0, f0, s.y, s.f, h, eps0, eps1, p, th, loc)) return INFLX_BG_NONFINITE;
  h_c = loc.y[4];
  n_c = loc.y[5];
  return INFLX_DN_LOCATED;
}

// Phase B: one accepted step of a member; when it passes the surface, H_1 <= h_c < H_0, the lane stops with INFLX_DN_LOCATED and
// n_hit = N of the dense output where H = h_c.
template <int METHOD>
INFLX_FN int inflx_dn_step_surface(InflxBgLane& s, const double* __restrict__ p, double max_err, double fixed_dt, double h_c, double& n_hit) {
  const double H0 = s.y[4], dH0 = s.f[4], N0 = s.y[5], dN0 = s.f[5];
  double h = 0.0, n_end = 0.0;
  const int st = inflx_bg_step_taken<METHOD>(s, p, max_err, fixed_dt, false, n_end, h);
  if (st != INFLX_BG_RUNNING) return st;
  if (!(s.y[4] <= h_c && h_c < H0)) return INFLX_BG_RUNNING;
  const double th = inflx_bg_locate(-H0, -dH0, -s.y[4], -s.f[4], h, -h_c);
  const double n = inflx_bg_hermite(N0, dN0, s.y[5], s.f[5], h, th);
  if (!isfinite(n)) return INFLX_BG_NONFINITE;
  n_hit = n;
  return INFLX_DN_LOCATED;
}

// One stencil: n9 and st9 are the nine members' N and statuses, x the centre's fields, h_star the centre's initial H, status_a the
// centre's phase-A status (INFLX_DN_LOCATED when H_end was given).  out[INFLX_DN_NOUT].
//   N_,I  central differences; N_,00 and N_,11 three-point, N_,01 from the four corners
//   G_ab  = o[3] of inflx_eom_point at chi = (1,0), (0,1), (1,1);  Gamma^a_bc = o[0..1] at those velocities minus o[0..1] at chi = 0
//   N_;IJ = N_,IJ - Gamma^K_IJ N_,K;  |grad N|^2 = G^IJ N_,I N_,J;  f_NL = (5/6) N^;I N^;J N_;IJ / |grad N|^4;
//   P_zeta = (h_star / 2 pi)^2 |grad N|^2
// A member that is not INFLX_DN_LOCATED makes every derived output NaN; the status is then that member's (the lowest such m) plus
// INFLX_DN_STATUS_STRIDE m -- the centre's phase-A status with m = 4 when phase A failed.
INFLX_FN void inflx_dn_reduce(const double* n9, const int* st9, int status_a, const double* x, double h0, double h1, double h_star,
                              const double* __restrict__ p, double* out) {
  int status = INFLX_DN_LOCATED;
  if (status_a != INFLX_DN_LOCATED) {
    status = status_a + INFLX_DN_STATUS_STRIDE * INFLX_DN_CENTRE;
  } else {
    for (int m = INFLX_DN_MEMBERS - 1; m >= 0; --m)
      if (st9[m] != INFLX_DN_LOCATED) status = st9[m] + INFLX_DN_STATUS_STRIDE * m;
  }
  for (int m = 0; m < INFLX_DN_MEMBERS; ++m) out[INFLX_DN_OUT_MEMBERS + m] = n9[m];
  out[INFLX_DN_OUT_STATUS] = (double)status;
  if (status != INFLX_DN_LOCATED) {
    const double nan = __builtin_nan("");
    for (int c = INFLX_DN_OUT_NI; c < INFLX_DN_OUT_STATUS; ++c) out[c] = nan;
    return;
  }
  const double d0 = (n9[7] - n9[1]) / (2.0 * h0), d1 = (n9[5] - n9[3]) / (2.0 * h1);
  const double d00 = (n9[7] - 2.0 * n9[4] + n9[1]) / (h0 * h0), d11 = (n9[5] - 2.0 * n9[4] + n9[3]) / (h1 * h1);
  const double d01 = (n9[8] - n9[6] - n9[2] + n9[0]) / (4.0 * h0 * h1);
  double oz[4], oa[4], ob[4], oc[4];
  inflx_eom_point(x[0], x[1], 0.0, 0.0, p, oz);
  inflx_eom_point(x[0], x[1], 1.0, 0.0, p, oa);
  inflx_eom_point(x[0], x[1], 0.0, 1.0, p, ob);
  inflx_eom_point(x[0], x[1], 1.0, 1.0, p, oc);
  const double g00 = oa[3], g11 = ob[3], g01 = 0.5 * (oc[3] - oa[3] - ob[3]);
  double gam00[2], gam11[2], gam01[2];  // Gamma^a_00, Gamma^a_11, Gamma^a_01
  for (int a = 0; a < 2; ++a) {
    gam00[a] = oa[a] - oz[a];
    gam11[a] = ob[a] - oz[a];
    gam01[a] = 0.5 * ((oc[a] - oz[a]) - gam00[a] - gam11[a]);
  }
  const double det = g00 * g11 - g01 * g01;
  const double i00 = g11 / det, i11 = g00 / det, i01 = -g01 / det;
  const double c00 = d00 - (gam00[0] * d0 + gam00[1] * d1), c11 = d11 - (gam11[0] * d0 + gam11[1] * d1), c01 = d01 - (gam01[0] * d0 + gam01[1] * d1);
  const double u0 = i00 * d0 + i01 * d1, u1 = i01 * d0 + i11 * d1;
  const double grad2 = u0 * d0 + u1 * d1;
  const double num = u0 * u0 * c00 + 2.0 * u0 * u1 * c01 + u1 * u1 * c11;
  const double two_pi = 6.283185307179586476925286766559;
  out[INFLX_DN_OUT_NI] = d0;
  out[INFLX_DN_OUT_NI + 1] = d1;
  out[INFLX_DN_OUT_NIJ] = d00;
  out[INFLX_DN_OUT_NIJ + 1] = d11;
  out[INFLX_DN_OUT_NIJ + 2] = d01;
  out[INFLX_DN_OUT_NCOV] = c00;
  out[INFLX_DN_OUT_NCOV + 1] = c11;
  out[INFLX_DN_OUT_NCOV + 2] = c01;
  out[INFLX_DN_OUT_GRAD2] = grad2;
  out[INFLX_DN_OUT_FNL] = (5.0 / 6.0) * num / (grad2 * grad2);
  out[INFLX_DN_OUT_PZETA] = (h_star / two_pi) * (h_star / two_pi) * grad2;
}
