// Background trajectories: the integrator of a two-field model's equations of motion (inflatox_amd.background).
//
// State y = (phi^0, phi^1, chi^0, chi^1, H, N) in Planck units and cosmic time, the reference's system
// (src/background_solver.rs EoM::f, EoM::g) with the e-fold count added:
//     dphi^a/dt = chi^a
//     dchi^a/dt = -eom^a(phi, chi) - 3 H chi^a      eom^a = Gamma^a_bc chi^b chi^c + G^ab d_b V   (the model's eom_fields)
//     dH/dt     = V - 3 H^2
//     dN/dt     = H
// integrated as a plain first-order Runge-Kutta system (no Nystroem form):
//     INFLX_BG_RKF  Fehlberg 4(5) with the reference's tableau; the state advances with the 4th-order weights, the error
//                   is |5th - 4th|;
//     INFLX_BG_RK4  classical RK4; the adaptive error comes from step doubling (one step of dt against two of dt/2, the
//                   state advances with the two half steps).
// Error norm: the absolute Euclidean norm over phi, chi and H (N is not part of it).  A step is accepted when
// err <= 1.1 max_err; the next dt is dt * clamp(0.9 (max_err/err)^(1/5), 0.2, 5).  A fixed dt (> 0) takes every step without
// error control.  Every loop is bounded: INFLX_BG_MAX_REJECTIONS consecutive rejections, or a dt that no longer moves t, stop
// the lane with a status.
//
// Everything is INFLX_FN code over one lane's registers, so that tests/background_twin.cpp compiles the very same stepper for
// the host.  The model enters through the generated inflx_eom_point (staging.emit_eom_header).
#pragma once

enum InflxBgStatus {
  INFLX_BG_RUNNING = 0,    // (final value: every requested step was taken)
  INFLX_BG_ENDED = 1,      // stop_at_end: epsilon_H reached 1
  INFLX_BG_NONFINITE = 2,  // the state or the equations of motion at it are not finite
  INFLX_BG_REJECTED = 3,   // INFLX_BG_MAX_REJECTIONS consecutive rejected steps
  INFLX_BG_UNDERFLOW = 4,  // t + dt == t
  INFLX_BG_TARGET = 5,     // N reached its target (inflx_bg_step_target); the lane holds the state located there
};

enum InflxBgMethod { INFLX_BG_RK4 = 0, INFLX_BG_RKF = 1 };

#define INFLX_BG_MAX_REJECTIONS 50
#define INFLX_BG_FIRST_DT 1e-10
#define INFLX_BG_MAX_LOCATE 64  // iterations of the root search for theta inside a step (inflx_bg_locate)

// One lane: the state, the right-hand side at it (k1 of the next step, and the kinetic term G_ab chi^a chi^b), t and dt.
struct InflxBgLane {
  double y[6];
  double f[6];
  double kin;
  double t;
  double dt;
};

// dy/dt at y; kin = G_ab chi^a chi^b
INFLX_FN void inflx_bg_rhs(const double* y, const double* __restrict__ p, double* f, double& kin) {
  double o[4];
  inflx_eom_point(y[0], y[1], y[2], y[3], p, o);
  f[0] = y[2];
  f[1] = y[3];
  f[2] = -o[0] - 3.0 * y[4] * y[2];
  f[3] = -o[1] - 3.0 * y[4] * y[3];
  f[4] = o[2] - 3.0 * y[4] * y[4];
  f[5] = y[4];
  kin = o[3];
}

INFLX_FN bool inflx_bg_finite6(const double* v) {
  bool ok = true;
  for (int c = 0; c < 6; ++c) ok = ok && isfinite(v[c]);
  return ok;
}

// the initial state: fields and velocities given, H from the Friedmann constraint H0 = sqrt((V + G_ab chi^a chi^b / 2) / 3), N = 0.
// With stop_at_end, a state that is already past the end of inflation (epsilon_H >= 1) ends there: INFLX_BG_ENDED, N_end = 0.
INFLX_FN int inflx_bg_init(InflxBgLane& s, const double* init, const double* __restrict__ p, double dt0, bool stop_at_end, double& n_end) {
  double o[4];
  inflx_eom_point(init[0], init[1], init[2], init[3], p, o);
  s.y[0] = init[0];
  s.y[1] = init[1];
  s.y[2] = init[2];
  s.y[3] = init[3];
  s.y[4] = sqrt((o[2] + 0.5 * o[3]) / 3.0);
  s.y[5] = 0.0;
  s.t = 0.0;
  s.dt = dt0;
  inflx_bg_rhs(s.y, p, s.f, s.kin);
  if (!(inflx_bg_finite6(s.y) && inflx_bg_finite6(s.f) && isfinite(s.kin))) return INFLX_BG_NONFINITE;
  if (stop_at_end && 0.5 * s.kin / (s.y[4] * s.y[4]) >= 1.0) {
    n_end = 0.0;
    return INFLX_BG_ENDED;
  }
  return INFLX_BG_RUNNING;
}

// the right-hand side at the lane's state again (a launch resumes from a carried state)
INFLX_FN void inflx_bg_resume(InflxBgLane& s, const double* __restrict__ p) { inflx_bg_rhs(s.y, p, s.f, s.kin); }

// epsilon_H = (G_ab chi^a chi^b / 2) / H^2
INFLX_FN double inflx_bg_epsilon(const InflxBgLane& s) { return 0.5 * s.kin / (s.y[4] * s.y[4]); }

// one classical RK4 step of size h from (y, f0 = f(y))
INFLX_FN void inflx_bg_rk4(const double* y, const double* f0, double h, const double* __restrict__ p, double* out) {
  double k2[6], k3[6], k4[6], ys[6], kin;
  for (int c = 0; c < 6; ++c) ys[c] = y[c] + h * (0.5 * f0[c]);
  inflx_bg_rhs(ys, p, k2, kin);
  for (int c = 0; c < 6; ++c) ys[c] = y[c] + h * (0.5 * k2[c]);
  inflx_bg_rhs(ys, p, k3, kin);
  for (int c = 0; c < 6; ++c) ys[c] = y[c] + h * (1.0 * k3[c]);
  inflx_bg_rhs(ys, p, k4, kin);
  for (int c = 0; c < 6; ++c) {
    double acc = (1.0 / 6.0) * f0[c];
    acc += (1.0 / 3.0) * k2[c];
    acc += (1.0 / 3.0) * k3[c];
    acc += (1.0 / 6.0) * k4[c];
    out[c] = y[c] + h * acc;
  }
}

// Fehlberg 4(5), the reference's tableau (src/background_solver.rs:232-240): out = 4th-order state, e = |5th - 4th| per component
INFLX_FN void inflx_bg_rkf(const double* y, const double* f0, double h, const double* __restrict__ p, double* out, double* e) {
  double k[6][6], ys[6], kin;
  for (int c = 0; c < 6; ++c) k[0][c] = f0[c];
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
    for (int c = 0; c < 6; ++c) {
      double acc = A[s][0] * k[0][c];
#pragma unroll
      for (int j = 1; j < s; ++j) acc += A[s][j] * k[j][c];
      ys[c] = y[c] + h * acc;
    }
    inflx_bg_rhs(ys, p, k[s], kin);
  }
  for (int c = 0; c < 6; ++c) {
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

INFLX_FN double inflx_bg_norm5(const double* e) {
  double acc = e[0] * e[0];
  for (int c = 1; c < 5; ++c) acc += e[c] * e[c];
  return sqrt(acc);
}

// a trial step of size h: out = the state it reaches, return value = its error estimate (0 for a fixed step)
template <int METHOD>
INFLX_FN double inflx_bg_trial(const InflxBgLane& s, double h, bool adaptive, const double* __restrict__ p, double* out) {
  if constexpr (METHOD == INFLX_BG_RKF) {
    double e[6];
    inflx_bg_rkf(s.y, s.f, h, p, out, e);
    return adaptive ? inflx_bg_norm5(e) : 0.0;
  } else {
    if (!adaptive) {
      inflx_bg_rk4(s.y, s.f, h, p, out);
      return 0.0;
    }
    double big[6], half[6], fh[6], kin, e[6];
    inflx_bg_rk4(s.y, s.f, h, p, big);
    const double h2 = 0.5 * h;
    inflx_bg_rk4(s.y, s.f, h2, p, half);
    inflx_bg_rhs(half, p, fh, kin);
    inflx_bg_rk4(half, fh, h2, p, out);
    for (int c = 0; c < 6; ++c) e[c] = fabs(out[c] - big[c]);
    return inflx_bg_norm5(e);
  }
}

INFLX_FN double inflx_bg_factor(double max_err, double err) {
  if (!(err > 0.0)) return 5.0;  // (err == 0: the largest growth)
  const double q = 0.9 * pow(max_err / err, 0.2);
  return q < 0.2 ? 0.2 : (q > 5.0 ? 5.0 : q);
}

// One accepted step (fixed_dt > 0: of that size, without error control).  Returns INFLX_BG_RUNNING, or the status that stops the
// lane; `n_end` receives N at epsilon_H = 1 when stop_at_end ends it (linear in epsilon_H across the step); `h_taken` the size of
// the accepted step (the lane's dt is already the next step's).
template <int METHOD>
INFLX_FN int inflx_bg_step_taken(InflxBgLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end, double& n_end,
                                 double& h_taken) {
  const bool adaptive = !(fixed_dt > 0.0);
  const double eps0 = inflx_bg_epsilon(s), n0 = s.y[5];
  double y1[6];
  int rejections = 0;
  for (;;) {
    if (s.t + s.dt == s.t) return INFLX_BG_UNDERFLOW;
    const double err = inflx_bg_trial<METHOD>(s, s.dt, adaptive, p, y1);
    const bool finite = inflx_bg_finite6(y1) && isfinite(err);
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
  for (int c = 0; c < 6; ++c) s.y[c] = y1[c];
  inflx_bg_rhs(s.y, p, s.f, s.kin);
  if (!(inflx_bg_finite6(s.f) && isfinite(s.kin))) return INFLX_BG_NONFINITE;
  if (stop_at_end) {
    const double eps1 = inflx_bg_epsilon(s);
    if (eps1 >= 1.0) {
      n_end = n0 + (1.0 - eps0) / (eps1 - eps0) * (s.y[5] - n0);  // (eps0 < 1: a lane that starts at or past the end ends in init)
      return INFLX_BG_ENDED;
    }
  }
  return INFLX_BG_RUNNING;
}

template <int METHOD>
INFLX_FN int inflx_bg_step(InflxBgLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end, double& n_end) {
  double h_taken = 0.0;
  return inflx_bg_step_taken<METHOD>(s, p, max_err, fixed_dt, stop_at_end, n_end, h_taken);
}

// ---- a target on N: the state where a trajectory has made n_target e-folds ------------------------------------------------------
// Dense output over an accepted step of size h from (y0, f0 = f(y0)) to (y1, f1 = f(y1)): the cubic Hermite interpolant
//     y(theta) = h00 y0 + h10 h f0 + h01 y1 + h11 h f1,   theta in [0, 1],
// which is within O(h^4) of the solution, the order of both steppers' states.
INFLX_FN double inflx_bg_hermite(double y0, double f0, double y1, double f1, double h, double th) {
  const double u = 1.0 - th;
  const double h00 = (1.0 + 2.0 * th) * u * u, h10 = th * u * u, h01 = th * th * (3.0 - 2.0 * th), h11 = -(th * th) * u;
  return h00 * y0 + h10 * (h * f0) + h01 * y1 + h11 * (h * f1);
}

// d/dtheta of the interpolant
INFLX_FN double inflx_bg_hermite_slope(double y0, double f0, double y1, double f1, double h, double th) {
  const double u = 1.0 - th;
  const double d00 = -6.0 * th * u, d10 = u * (1.0 - 3.0 * th), d11 = th * (3.0 * th - 2.0);
  return d00 * y0 + d10 * (h * f0) - d00 * y1 + d11 * (h * f1);
}

// theta in [0, 1] with N(theta) = n_target, for N(0) < n_target <= N(1): Newton's iteration on the interpolant of N, kept inside a
// bracket [lo, hi] with N(lo) < n_target <= N(hi) that every iterate tightens; an iterate that leaves the bracket (N is monotone
// across the step only where H > 0) is replaced by the bracket's midpoint.  At most INFLX_BG_MAX_LOCATE iterations.
INFLX_FN double inflx_bg_locate(double n0, double h0, double n1, double h1, double h, double n_target) {
  double lo = 0.0, hi = 1.0;
  double th = (n_target - n0) / (n1 - n0);
  if (!(th > 0.0)) th = 0.0;
  if (th > 1.0) th = 1.0;
  for (int it = 0; it < INFLX_BG_MAX_LOCATE; ++it) {
    const double g = inflx_bg_hermite(n0, h0, n1, h1, h, th) - n_target;
    if (g == 0.0) break;
    if (g < 0.0)
      lo = th;
    else
      hi = th;
    double next = th - g / inflx_bg_hermite_slope(n0, h0, n1, h1, h, th);
    if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
    const double moved = fabs(next - th);
    th = next;
    if (moved <= 1e-15 || hi - lo <= 1e-15) break;
  }
  return th;
}

// the located state of a lane that reached its target: y[0..5] (N = the target exactly), t, and epsilon_H there
struct InflxBgLocated {
  double y[6];
  double t;
  double eps;
};

// epsilon_H at the located state (one evaluation of the model); false: the state or epsilon_H is not finite
INFLX_FN bool inflx_bg_located_epsilon(InflxBgLocated& loc, const double* __restrict__ p) {
  double o[4];
  inflx_eom_point(loc.y[0], loc.y[1], loc.y[2], loc.y[3], p, o);
  loc.eps = 0.5 * o[3] / (loc.y[4] * loc.y[4]);
  return inflx_bg_finite6(loc.y) && isfinite(loc.t) && isfinite(loc.eps);
}

// inflx_bg_init for a lane with a target: a target <= 0 is reached by the initial state (INFLX_BG_TARGET, t = 0) -- unless that
// state is already past the end of inflation with stop_at_end, which ends the lane as in inflx_bg_init.
INFLX_FN int inflx_bg_init_target(InflxBgLane& s, const double* init, const double* __restrict__ p, double dt0, bool stop_at_end, double n_target,
                                  double& n_end, InflxBgLocated& loc) {
  const int st = inflx_bg_init(s, init, p, dt0, stop_at_end, n_end);
  if (st != INFLX_BG_RUNNING || !(n_target <= 0.0)) return st;
  for (int c = 0; c < 6; ++c) loc.y[c] = s.y[c];
  loc.t = s.t;
  loc.eps = inflx_bg_epsilon(s);
  return INFLX_BG_TARGET;
}

// One accepted step of a lane with a target: inflx_bg_step, and when the new state has N >= n_target the lane stops with
// INFLX_BG_TARGET and `loc` = the state where N = n_target inside that step: the Hermite interpolant at the theta of
// inflx_bg_locate, N set to the target, t = t0 + theta h, epsilon_H from the model at that state (not finite: INFLX_BG_NONFINITE).
// A step that also ends inflation (stop_at_end) ends the lane instead when epsilon_H = 1 comes first, n_end < n_target.
template <int METHOD>
INFLX_FN int inflx_bg_step_target(InflxBgLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end, double n_target,
                                  double& n_end, InflxBgLocated& loc) {
  double y0[6], f0[6], h = 0.0;
  for (int c = 0; c < 6; ++c) {
    y0[c] = s.y[c];
    f0[c] = s.f[c];
  }
  const double t0 = s.t;
  const int st = inflx_bg_step_taken<METHOD>(s, p, max_err, fixed_dt, stop_at_end, n_end, h);
  if (st != INFLX_BG_RUNNING && st != INFLX_BG_ENDED) return st;
  if (!(s.y[5] >= n_target)) return st;
  if (st == INFLX_BG_ENDED && n_end < n_target) return st;
  const double th = inflx_bg_locate(y0[5], f0[5], s.y[5], s.f[5], h, n_target);
  for (int c = 0; c < 5; ++c) loc.y[c] = inflx_bg_hermite(y0[c], f0[c], s.y[c], s.f[c], h, th);
  loc.y[5] = n_target;
  loc.t = t0 + th * h;
  return inflx_bg_located_epsilon(loc, p) ? INFLX_BG_TARGET : INFLX_BG_NONFINITE;
}

// ---- samples: the state at every point of a list shared by all lanes ------------------------------------------------------------
// `samples` (n_samples, finite, >= 0, strictly increasing) are e-fold counts, or times when `sample_t`.  A lane emits sample k --
// sink(k, located state) -- from the accepted step that passes it, with the dense output above: for N the theta of
// inflx_bg_locate, N = the sample exactly and t = t0 + theta h, which is inflx_bg_step_target's located state bit for bit; for t,
// theta = (t_s - t0) / h, t = the sample exactly and N from the interpolant.  `cursor` counts the samples emitted.  The lane goes on
// from the step's end state, never from a located one, so its steps are those of the ordinary run.

// inflx_bg_init for a lane with samples: a sample equal to 0 is the initial state (also of a lane that is already past the end of
// inflation, which ends here as in inflx_bg_init); INFLX_BG_TARGET when that was the only sample.
template <class SINK>
INFLX_FN int inflx_bg_init_sampled(InflxBgLane& s, const double* init, const double* __restrict__ p, double dt0, bool stop_at_end,
                                   const double* __restrict__ samples, unsigned n_samples, unsigned& cursor, double& n_end, SINK& sink) {
  cursor = 0;
  const int st = inflx_bg_init(s, init, p, dt0, stop_at_end, n_end);
  if (st == INFLX_BG_NONFINITE) return st;
  if (n_samples > 0 && samples[0] == 0.0) {
    InflxBgLocated loc;
    for (int c = 0; c < 6; ++c) loc.y[c] = s.y[c];
    loc.t = s.t;
    loc.eps = inflx_bg_epsilon(s);
    sink(0u, loc);
    cursor = 1;
  }
  return st == INFLX_BG_RUNNING && cursor == n_samples ? INFLX_BG_TARGET : st;
}

// One accepted step of a lane with samples, and every sample that step passed: those with sample <= N1 (<= t1 when sample_t).  In
// the step that ends inflation (stop_at_end) only the samples up to epsilon_H = 1 are emitted -- N_s <= n_end, or
// t_s <= t0 + f h with n_end's fraction f = (1 - eps0) / (eps1 - eps0) --, inflx_bg_step_target's "which comes first".  Returns
// INFLX_BG_TARGET once every sample is emitted, INFLX_BG_NONFINITE when a located state is not finite (that sample is not emitted),
// and inflx_bg_step_taken's status otherwise.
template <int METHOD, class SINK>
INFLX_FN int inflx_bg_step_sampled(InflxBgLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end,
                                   const double* __restrict__ samples, unsigned n_samples, bool sample_t, unsigned& cursor, double& n_end,
                                   SINK& sink) {
  double y0[6], f0[6], h = 0.0;
  for (int c = 0; c < 6; ++c) {
    y0[c] = s.y[c];
    f0[c] = s.f[c];
  }
  const double t0 = s.t, eps0 = inflx_bg_epsilon(s);
  const int st = inflx_bg_step_taken<METHOD>(s, p, max_err, fixed_dt, stop_at_end, n_end, h);
  if (st != INFLX_BG_RUNNING && st != INFLX_BG_ENDED) return st;
  double t_end = 0.0;  // t at epsilon_H = 1 (sample_t, in the step that ends inflation)
  if (st == INFLX_BG_ENDED && sample_t) t_end = t0 + (1.0 - eps0) / (inflx_bg_epsilon(s) - eps0) * h;
  while (cursor < n_samples) {
    const double x = samples[cursor];
    if (sample_t ? !(x <= s.t) : !(s.y[5] >= x)) break;
    if (st == INFLX_BG_ENDED && (sample_t ? t_end < x : n_end < x)) break;
    InflxBgLocated loc;
    if (sample_t) {
      const double th = (x - t0) / h;
      for (int c = 0; c < 6; ++c) loc.y[c] = inflx_bg_hermite(y0[c], f0[c], s.y[c], s.f[c], h, th);
      loc.t = x;
    } else {
      const double th = inflx_bg_locate(y0[5], f0[5], s.y[5], s.f[5], h, x);
      for (int c = 0; c < 5; ++c) loc.y[c] = inflx_bg_hermite(y0[c], f0[c], s.y[c], s.f[c], h, th);
      loc.y[5] = x;
      loc.t = t0 + th * h;
    }
    if (!inflx_bg_located_epsilon(loc, p)) return INFLX_BG_NONFINITE;
    sink(cursor, loc);
    ++cursor;
  }
  return cursor == n_samples ? INFLX_BG_TARGET : st;
}
