// Reheating: a two-field trajectory whose fields decay into a radiation bath at a constant rate Gamma, followed until the bath
// dominates (inflatox_amd.reheating).
//
// State y = (phi^0, phi^1, chi^0, chi^1, H, N, rho_r) in the units of csrc/inflx_background.h (reduced Planck mass 1, cosmic time,
// 3 H^2 = rho), one constant Gamma >= 0 per lane:
//     dphi^a/dt  = chi^a
//     dchi^a/dt  = -eom^a(phi, chi) - (3 H + Gamma) chi^a       eom^a from the generated inflx_eom_point, as in inflx_bg_rhs
//     dH/dt      = V - 3 H^2 + rho_r / 3                        (= -G_ab chi^a chi^b / 2 - 2 rho_r / 3 by the constraint)
//     dN/dt      = H
//     drho_r/dt  = -4 H rho_r + Gamma G_ab chi^a chi^b
// The constraint 3 H^2 = V + G_ab chi^a chi^b / 2 + rho_r fixes H_0 and holds along the flow; it is not imposed again.  The steppers
// are those of csrc/inflx_background.h on seven components -- the same tableau, acceptance rule (err <= 1.1 max_err), step factor
// (inflx_bg_factor), first dt and bounds (INFLX_BG_MAX_REJECTIONS, t + dt == t) -- with the absolute Euclidean error norm over phi,
// chi, H and rho_r (N is outside it, as there).
//
// Event: a lane stops INFLX_RH_REHEATED at the first accepted step whose end state has Omega_r = rho_r / (3 H^2) >= omega_r, tested
// as g = rho_r - 3 omega_r H^2 >= 0.  The state is located where g(theta) = rho_r(theta) - 3 omega_r H(theta)^2 = 0 on the step's
// cubic Hermite dense output (inflx_bg_hermite): a polynomial in theta, so the search -- the Illinois iteration of
// inflx_dn_locate_end, with its bracket, iteration count and stops -- evaluates no model.  All seven components and t come from the
// interpolant at that theta.
//
// Everything is INFLX_FN code over one lane's registers, so that tests/reheating_twin.cpp compiles the very same text for the host.
// Needs csrc/inflx_background.h (statuses, methods, constants, inflx_bg_factor, the Hermite interpolant) before it.
#pragma once

// the status of a reheating lane beyond InflxBgStatus and InflxDnStatus (0..8; 9 is inflatox_amd.background.OUTSIDE_AT_START)
enum InflxRhStatus {
  INFLX_RH_REHEATED = 10,  // Omega_r reached omega_r; the lane holds the state located there
};

#define INFLX_RH_COMPONENTS 7
#define INFLX_RH_RHO 6  // y[6] = rho_r

// One lane: the state, the right-hand side at it (k1 of the next step, and the kinetic term G_ab chi^a chi^b), t, dt and the lane's
// decay rate.
struct InflxRhLane {
  double y[INFLX_RH_COMPONENTS];
  double f[INFLX_RH_COMPONENTS];
  double kin;
  double t;
  double dt;
  double gamma;
};

// the located state of a lane that reheated: y[0..6] and t
struct InflxRhLocated {
  double y[INFLX_RH_COMPONENTS];
  double t;
};

// dy/dt at y; kin = G_ab chi^a chi^b
INFLX_FN void inflx_rh_rhs(const double* y, double gamma, const double* __restrict__ p, double* f, double& kin) {
  double o[4];
  inflx_eom_point(y[0], y[1], y[2], y[3], p, o);
  const double friction = 3.0 * y[4] + gamma;
  f[0] = y[2];
  f[1] = y[3];
  f[2] = -o[0] - friction * y[2];
  f[3] = -o[1] - friction * y[3];
  f[4] = o[2] - 3.0 * y[4] * y[4] + y[6] / 3.0;
  f[5] = y[4];
  f[6] = -4.0 * y[4] * y[6] + gamma * o[3];
  kin = o[3];
}

INFLX_FN bool inflx_rh_finite7(const double* v) {
  bool ok = true;
  for (int c = 0; c < INFLX_RH_COMPONENTS; ++c) ok = ok && isfinite(v[c]);
  return ok;
}

// the event function at a state: rho_r - 3 omega_r H^2, >= 0 where Omega_r >= omega_r
INFLX_FN double inflx_rh_event(double h, double rho_r, double omega_r) { return rho_r - 3.0 * omega_r * (h * h); }

// The initial state: fields and velocities given, rho_r = rho_r0, H from the constraint H_0 = sqrt((V + G_ab chi^a chi^b / 2 +
// rho_r0) / 3), N = 0, t = 0.  A state that already has Omega_r >= omega_r is INFLX_RH_REHEATED there: `loc` is the initial state.
INFLX_FN int inflx_rh_init(InflxRhLane& s, const double* init, double gamma, double rho_r0, const double* __restrict__ p, double dt0, double omega_r,
                           InflxRhLocated& loc) {
  double o[4];
  inflx_eom_point(init[0], init[1], init[2], init[3], p, o);
  s.y[0] = init[0];
  s.y[1] = init[1];
  s.y[2] = init[2];
  s.y[3] = init[3];
  s.y[4] = sqrt((o[2] + 0.5 * o[3] + rho_r0) / 3.0);
  s.y[5] = 0.0;
  s.y[6] = rho_r0;
  s.t = 0.0;
  s.dt = dt0;
  s.gamma = gamma;
  inflx_rh_rhs(s.y, gamma, p, s.f, s.kin);
  if (!(inflx_rh_finite7(s.y) && inflx_rh_finite7(s.f) && isfinite(s.kin))) return INFLX_BG_NONFINITE;
  if (inflx_rh_event(s.y[4], s.y[6], omega_r) >= 0.0) {
    for (int c = 0; c < INFLX_RH_COMPONENTS; ++c) loc.y[c] = s.y[c];
    loc.t = s.t;
    return INFLX_RH_REHEATED;
  }
  return INFLX_BG_RUNNING;
}

// the right-hand side at the lane's state again (a launch resumes from a carried state)
INFLX_FN void inflx_rh_resume(InflxRhLane& s, const double* __restrict__ p) { inflx_rh_rhs(s.y, s.gamma, p, s.f, s.kin); }

// one classical RK4 step of size h from (y, f0 = f(y))
INFLX_FN void inflx_rh_rk4(const double* y, const double* f0, double h, double gamma, const double* __restrict__ p, double* out) {
  constexpr int NC = INFLX_RH_COMPONENTS;
  double k2[NC], k3[NC], k4[NC], ys[NC], kin;
  for (int c = 0; c < NC; ++c) ys[c] = y[c] + h * (0.5 * f0[c]);
  inflx_rh_rhs(ys, gamma, p, k2, kin);
  for (int c = 0; c < NC; ++c) ys[c] = y[c] + h * (0.5 * k2[c]);
  inflx_rh_rhs(ys, gamma, p, k3, kin);
  for (int c = 0; c < NC; ++c) ys[c] = y[c] + h * (1.0 * k3[c]);
  inflx_rh_rhs(ys, gamma, p, k4, kin);
  for (int c = 0; c < NC; ++c) {
    double acc = (1.0 / 6.0) * f0[c];
    acc += (1.0 / 3.0) * k2[c];
    acc += (1.0 / 3.0) * k3[c];
    acc += (1.0 / 6.0) * k4[c];
    out[c] = y[c] + h * acc;
  }
}

// Fehlberg 4(5) with the tableau of inflx_bg_rkf: out = 4th-order state, e = |5th - 4th| per component
INFLX_FN void inflx_rh_rkf(const double* y, const double* f0, double h, double gamma, const double* __restrict__ p, double* out, double* e) {
  constexpr int NC = INFLX_RH_COMPONENTS;
  double k[6][NC], ys[NC], kin;
  for (int c = 0; c < NC; ++c) k[0][c] = f0[c];
  constexpr double A[6][5] = {
      {0., 0., 0., 0., 0.},
      {0.25, 0., 0., 0., 0.},
      {3. / 32., 9. / 32., 0., 0., 0.},
      {1932. / 2197., -7200. / 2197., 7296. / 2197., 0., 0.},
      {439. / 216., -8., 3680. / 513., -845. / 4104., 0.},
      {-8. / 27., 2., -3544. / 2565., 1859. / 4104., -11. / 40.},
  };
  constexpr double B5[6] = {16. / 135., 0., 6656. / 12825., 28561. / 56430., -9. / 50., 2. / 55.};
  constexpr double B4[6] = {25. / 216., 0., 1408. / 2565., 2197. / 4104., -1. / 5., 0.};
#pragma unroll
  for (int s = 1; s < 6; ++s) {
    for (int c = 0; c < NC; ++c) {
      double acc = A[s][0] * k[0][c];
#pragma unroll
      for (int j = 1; j < s; ++j) acc += A[s][j] * k[j][c];
      ys[c] = y[c] + h * acc;
    }
    inflx_rh_rhs(ys, gamma, p, k[s], kin);
  }
  for (int c = 0; c < NC; ++c) {
    double a4 = B4[0] * k[0][c], a5 = B5[0] * k[0][c];
#pragma unroll
    for (int j = 1; j < 6; ++j) {
      a4 += B4[j] * k[j][c];
      a5 += B5[j] * k[j][c];
    }
    out[c] = y[c] + h * a4;
    e[c] = fabs(h * a5 - h * a4);
  }
}

// the error norm: phi, chi, H and rho_r -- every component but N
INFLX_FN double inflx_rh_norm(const double* e) {
  double acc = e[0] * e[0];
  for (int c = 1; c < 5; ++c) acc += e[c] * e[c];
  acc += e[INFLX_RH_RHO] * e[INFLX_RH_RHO];
  return sqrt(acc);
}

// a trial step of size h: out = the state it reaches, return value = its error estimate (0 for a fixed step)
template <int METHOD>
INFLX_FN double inflx_rh_trial(const InflxRhLane& s, double h, bool adaptive, const double* __restrict__ p, double* out) {
  constexpr int NC = INFLX_RH_COMPONENTS;
  if constexpr (METHOD == INFLX_BG_RKF) {
    double e[NC];
    inflx_rh_rkf(s.y, s.f, h, s.gamma, p, out, e);
    return adaptive ? inflx_rh_norm(e) : 0.0;
  } else {
    if (!adaptive) {
      inflx_rh_rk4(s.y, s.f, h, s.gamma, p, out);
      return 0.0;
    }
    double big[NC], half[NC], fh[NC], kin, e[NC];
    inflx_rh_rk4(s.y, s.f, h, s.gamma, p, big);
    const double h2 = 0.5 * h;
    inflx_rh_rk4(s.y, s.f, h2, s.gamma, p, half);
    inflx_rh_rhs(half, s.gamma, p, fh, kin);
    inflx_rh_rk4(half, fh, h2, s.gamma, p, out);
    for (int c = 0; c < NC; ++c) e[c] = fabs(out[c] - big[c]);
    return inflx_rh_norm(e);
  }
}

// One accepted step (fixed_dt > 0: of that size, without error control), inflx_bg_step_taken on seven components without its event.
// Returns INFLX_BG_RUNNING, or the status that stops the lane; `h_taken` is the size of the accepted step (the lane's dt is already
// the next step's).  A lane that stops REJECTED or UNDERFLOW, or NONFINITE in a trial, keeps the state it held.
template <int METHOD>
INFLX_FN int inflx_rh_step_taken(InflxRhLane& s, const double* __restrict__ p, double max_err, double fixed_dt, double& h_taken) {
  const bool adaptive = !(fixed_dt > 0.0);
  double y1[INFLX_RH_COMPONENTS];
  int rejections = 0;
  for (;;) {
    if (s.t + s.dt == s.t) return INFLX_BG_UNDERFLOW;
    const double err = inflx_rh_trial<METHOD>(s, s.dt, adaptive, p, y1);
    const bool finite = inflx_rh_finite7(y1) && isfinite(err);
    if (!adaptive) {
      if (!finite) return INFLX_BG_NONFINITE;
      h_taken = s.dt;
      s.t += s.dt;
      break;
    }
    if (finite && err <= 1.1 * max_err) {
      h_taken = s.dt;
      s.t += s.dt;
      s.dt *= inflx_bg_factor(max_err, err);
      break;
    }
    s.dt *= finite ? inflx_bg_factor(max_err, err) : 0.2;
    if (++rejections >= INFLX_BG_MAX_REJECTIONS) return INFLX_BG_REJECTED;
  }
  for (int c = 0; c < INFLX_RH_COMPONENTS; ++c) s.y[c] = y1[c];
  inflx_rh_rhs(s.y, s.gamma, p, s.f, s.kin);
  if (!(inflx_rh_finite7(s.f) && isfinite(s.kin))) return INFLX_BG_NONFINITE;
  return INFLX_BG_RUNNING;
}

// g(theta) = rho_r(theta) - 3 omega_r H(theta)^2 on the dense output of a step given by H and rho_r and their slopes at its ends
INFLX_FN double inflx_rh_dense_event(const double* y0, const double* f0, const double* y1, const double* f1, double h, double th, double omega_r) {
  const double hub = inflx_bg_hermite(y0[4], f0[4], y1[4], f1[4], h, th);
  const double rho = inflx_bg_hermite(y0[INFLX_RH_RHO], f0[INFLX_RH_RHO], y1[INFLX_RH_RHO], f1[INFLX_RH_RHO], h, th);
  return inflx_rh_event(hub, rho, omega_r);
}

// theta in (0, 1] with g(theta) = 0 for g(0) = g0 < 0 <= g1 = g(1): the Illinois iteration of inflx_dn_locate_end (a secant step
// inside the bracket [lo, hi], g(lo) < 0 <= g(hi); the end that stays twice has its g halved; an iterate that leaves the bracket is
// replaced by the midpoint), at most INFLX_BG_MAX_LOCATE iterations, stopping at g == 0 or a bracket <= 1e-15.  False: an iterate's
// g was not finite.
INFLX_FN bool inflx_rh_locate(const double* y0, const double* f0, const double* y1, const double* f1, double h, double g0, double g1, double omega_r,
                              double& theta) {
  double lo = 0.0, hi = 1.0, glo = g0, ghi = g1;
  double th = 1.0;
  int side = 0;
  if (ghi == 0.0) {
    theta = th;
    return true;
  }
  for (int it = 0; it < INFLX_BG_MAX_LOCATE; ++it) {
    th = (lo * ghi - hi * glo) / (ghi - glo);
    if (!(th > lo && th < hi)) th = 0.5 * (lo + hi);
    const double g = inflx_rh_dense_event(y0, f0, y1, f1, h, th, omega_r);
    if (!isfinite(g)) return false;
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

// One accepted step of a reheating lane; when the new state has Omega_r >= omega_r the lane stops with INFLX_RH_REHEATED and `loc` =
// the dense output where g = 0: all seven components from the interpolant at the located theta, t = t0 + theta h (not finite:
// INFLX_BG_NONFINITE).  (g < 0 at the step's start: a lane that starts at or past omega_r stops in inflx_rh_init.)
template <int METHOD>
INFLX_FN int inflx_rh_step(InflxRhLane& s, const double* __restrict__ p, double max_err, double fixed_dt, double omega_r, InflxRhLocated& loc) {
  double y0[INFLX_RH_COMPONENTS], f0[INFLX_RH_COMPONENTS], h = 0.0;
  for (int c = 0; c < INFLX_RH_COMPONENTS; ++c) {
    y0[c] = s.y[c];
    f0[c] = s.f[c];
  }
  const double t0 = s.t;
  const double g0 = inflx_rh_event(y0[4], y0[INFLX_RH_RHO], omega_r);
  const int st = inflx_rh_step_taken<METHOD>(s, p, max_err, fixed_dt, h);
  if (st != INFLX_BG_RUNNING) return st;
  const double g1 = inflx_rh_event(s.y[4], s.y[INFLX_RH_RHO], omega_r);
  if (!(g1 >= 0.0)) return INFLX_BG_RUNNING;
  double th = 1.0;
  if (!inflx_rh_locate(y0, f0, s.y, s.f, h, g0, g1, omega_r, th)) return INFLX_BG_NONFINITE;
  for (int c = 0; c < INFLX_RH_COMPONENTS; ++c) loc.y[c] = inflx_bg_hermite(y0[c], f0[c], s.y[c], s.f[c], h, th);
  loc.t = t0 + th * h;
  return inflx_rh_finite7(loc.y) && isfinite(loc.t) ? (int)INFLX_RH_REHEATED : (int)INFLX_BG_NONFINITE;
}
