// Super-horizon transfer functions T_RS and T_SS of a two-field model (inflatox_amd.background.transfer_functions): the background
// trajectory and, carried along it from horizon exit, the entropic perturbation and the curvature perturbation it sources.
//
// Lane state, cosmic time and Planck units: the background's y = (phi^0, phi^1, chi^0, chi^1, H, N) (csrc/inflx_background.h) plus
// (q, u, r) in y[6..8].  With kin = G_ab chi^a chi^b (inflx_eom_point o[3]), cross (inflx_kin_point o[1], csrc/inflx_kinematics.h)
// and m[.] (inflx_mass_point, csrc/inflx_masses.h), Omega = cross / kin (= omega H) and eps = kin / (2 H^2):
//     dq/dt = u
//     du/dt = -3 H u - (m[2] / kin + kin m[3] / 2 + 3 Omega^2) q      (= -3 H u - H^2 mu_s2 q, mu_s2 that of csrc/inflx_masses.h)
//     dr/dt = 2 Omega q sqrt(eps_star / eps)                          (eps_star = eps at the initial state)
// q = Q_s(t) / Q_s(0) is the entropic perturbation on super-horizon scales in units of its initial value;
// T_SS = q sqrt(eps_star / eps) is S / S_star with S = Q_s / sqrt(2 eps); T_RS = r, where R(N) = R_star + T_RS S_star.
// Initial values: q = 1, u = H0 dq_dN, r = 0.
//
// ORIENTATION.  Q_s is measured along T turned COUNTER-CLOCKWISE in the (x0, x1) chart.  That is -N of csrc/inflx_kinematics.h (whose
// N is T turned clockwise): the side the trajectory turns towards when omega > 0.  With that choice dR/dN = +2 omega S with the
// project's signed omega.  (Checked against the k = 0 field-basis system Q''^a + 3 H Q'^a + [V_ab - a^-3 d/dt(a^3 chi_a chi_b / H)]
// Q^b = 0 on the flat plane, which uses neither omega nor mu_s2: tests/transfer_reference.py.)
//
// Default dq_dN: the slowly decaying root of lambda^2 + (3 - eps_star) lambda + mu_s2_star = 0,
// lambda = [-(3 - eps_star) + sqrt((3 - eps_star)^2 - 4 mu_s2_star)] / 2, and its real part -(3 - eps_star) / 2 when the discriminant
// is negative.
//
// Steppers: inflx_background.h's over nine components -- the same tableau, acceptance rule (err <= 1.1 max_err), step factor, first
// dt, rejection and underflow bounds and statuses, and for the first six components the very expressions of inflx_bg_rhs,
// inflx_bg_rkf and inflx_bg_rk4, so that with a fixed dt the background part is solve_eom_sampled's bit for bit.  The ERROR NORM is
// the absolute Euclidean norm over phi, chi, H, q, u and r: eight components, N excluded.  An adaptive run therefore takes OTHER
// steps than solve_eom_sampled with the same max_err (never longer ones at the same state and dt).
//
// Samples are e-fold counts since the start, located as in inflx_bg_step_sampled: theta from inflx_bg_locate, the cubic Hermite
// interpolant for y, q and r from the values and right-hand sides at the step's two ends, eps from the model at the located state,
// T_SS = q_loc sqrt(eps_star / eps_loc).  A sample at 0 gives T_SS = 1 and T_RS = 0 exactly.  With stop_at_end, in the step where
// eps_H reaches 1 only samples up to N_end are emitted and the lane's end values are linear across that step at N_end's own
// fraction f = (1 - eps0) / (eps1 - eps0): q_end = q0 + f (q1 - q0), T_SS_end = q_end sqrt(eps_star), T_RS_end = r0 + f (r1 - r0).
// A lane that is past the end at the start (N_end = 0) has T_SS_end = 1, T_RS_end = 0.
//
// A lane stops with INFLX_BG_TARGET in the accepted step that emits its last sample, as in inflx_bg_step_sampled.  Unlike there, a
// sample emitted by init never stops a lane: a list that holds nothing but the sample 0 asks for the end values alone, and the lane
// runs on to the end of inflation (INFLX_BG_ENDED with stop_at_end) or until the steps run out (transfer_map does this).
//
// Init failures: a lane whose initial state has kin = 0 (a point has no direction), or whose eps_star, omega_star or mu_s2_star is
// not finite, stops at once with INFLX_BG_NONFINITE and emits nothing.
//
// INFLX_FN code over one lane's registers, every per-lane array indexed with compile-time constants once the loops are unrolled, so
// that tests/transfer_twin.cpp compiles the very same text for the host.  The model enters through the generated inflx_eom_point,
// inflx_kin_point and inflx_mass_point.  Include inflx_background.h first: its status and method enums, inflx_bg_init,
// inflx_bg_rhs, inflx_bg_hermite, inflx_bg_locate, inflx_bg_located_epsilon and inflx_bg_factor are used as they are.
#pragma once

#define INFLX_TR_NC 9  // components of the lane state
enum InflxTrComponent { INFLX_TR_Q = 6, INFLX_TR_U = 7, INFLX_TR_R = 8 };

// One lane: the state, the right-hand side at it (k1 of the next step, and kin there), t, dt and eps at the initial state.
struct InflxTrLane {
  double y[INFLX_TR_NC];
  double f[INFLX_TR_NC];
  double kin;
  double t;
  double dt;
  double eps_star;
};

// what a lane emits at a sample: the located background state (y[0..5], t, eps_H) and the two transfer functions there
struct InflxTrSample {
  InflxBgLocated loc;
  double t_ss;
  double t_rs;
};

// dy/dt at y over nine components; kin = G_ab chi^a chi^b.  f[0..5] are inflx_bg_rhs's.
// Kept OUT OF LINE (INFLX_FN_NOINLINE, csrc/inflx_device_math.h): a trial step evaluates it five (RKF) or eleven (RK4 with step
// doubling) times, each a copy of the model's three point functions when inlined.  The stage arrays it is handed then live in
// scratch, not in registers (DESIGN.md section 12 has the figures of both builds and why this one was chosen).
INFLX_FN_NOINLINE void inflx_tr_rhs(const double* y, const double* __restrict__ p, double eps_star, double* f, double& kin) {
  inflx_bg_rhs(y, p, f, kin);
  double k[2], m[4];
  inflx_kin_point(y[0], y[1], y[2], y[3], p, k);
  inflx_mass_point(y[0], y[1], y[2], y[3], p, m);
  const double H = y[4];
  const double Om = k[1] / kin;
  const double eps = 0.5 * kin / (H * H);
  const double mass = m[2] / kin + 0.5 * kin * m[3] + 3.0 * (Om * Om);  // H^2 mu_s2
  f[INFLX_TR_Q] = y[INFLX_TR_U];
  f[INFLX_TR_U] = -3.0 * H * y[INFLX_TR_U] - mass * y[INFLX_TR_Q];
  f[INFLX_TR_R] = 2.0 * Om * y[INFLX_TR_Q] * sqrt(eps_star / eps);
}

INFLX_FN bool inflx_tr_finite9(const double* v) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) ok = ok && isfinite(v[c]);
  return ok;
}

// eps_H = (G_ab chi^a chi^b / 2) / H^2: inflx_bg_epsilon's expression
INFLX_FN double inflx_tr_epsilon(const InflxTrLane& s) { return 0.5 * s.kin / (s.y[4] * s.y[4]); }

// the right-hand side at the lane's state again (a launch resumes from a carried state)
INFLX_FN void inflx_tr_resume(InflxTrLane& s, const double* __restrict__ p) { inflx_tr_rhs(s.y, p, s.eps_star, s.f, s.kin); }

// one classical RK4 step of size h from (y, f0 = f(y)): inflx_bg_rk4 over nine components
INFLX_FN void inflx_tr_rk4(const double* y, const double* f0, double h, const double* __restrict__ p, double eps_star, double* out) {
  double k2[INFLX_TR_NC], k3[INFLX_TR_NC], k4[INFLX_TR_NC], ys[INFLX_TR_NC], kin;
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) ys[c] = y[c] + h * (0.5 * f0[c]);
  inflx_tr_rhs(ys, p, eps_star, k2, kin);
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) ys[c] = y[c] + h * (0.5 * k2[c]);
  inflx_tr_rhs(ys, p, eps_star, k3, kin);
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) ys[c] = y[c] + h * (1.0 * k3[c]);
  inflx_tr_rhs(ys, p, eps_star, k4, kin);
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) {
    double acc = (1.0 / 6.0) * f0[c];
    acc += (1.0 / 3.0) * k2[c];
    acc += (1.0 / 3.0) * k3[c];
    acc += (1.0 / 6.0) * k4[c];
    out[c] = y[c] + h * acc;
  }
}

// Fehlberg 4(5), inflx_bg_rkf over nine components: out = 4th-order state, e = |5th - 4th| per component
INFLX_FN void inflx_tr_rkf(const double* y, const double* f0, double h, const double* __restrict__ p, double eps_star, double* out, double* e) {
  double k[6][INFLX_TR_NC], ys[INFLX_TR_NC], kin;
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) k[0][c] = f0[c];
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
#pragma unroll
    for (int c = 0; c < INFLX_TR_NC; ++c) {
      double acc = A[s][0] * k[0][c];
#pragma unroll
      for (int j = 1; j < s; ++j) acc += A[s][j] * k[j][c];
      ys[c] = y[c] + h * acc;
    }
    inflx_tr_rhs(ys, p, eps_star, k[s], kin);
  }
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) {
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

// the error norm: phi, chi, H, q, u, r -- eight components, N (component 5) excluded
INFLX_FN double inflx_tr_norm8(const double* e) {
  double acc = e[0] * e[0];
#pragma unroll
  for (int c = 1; c < 5; ++c) acc += e[c] * e[c];
#pragma unroll
  for (int c = 6; c < INFLX_TR_NC; ++c) acc += e[c] * e[c];
  return sqrt(acc);
}

// a trial step of size h: out = the state it reaches, return value = its error estimate (0 for a fixed step)
template <int METHOD>
INFLX_FN double inflx_tr_trial(const InflxTrLane& s, double h, bool adaptive, const double* __restrict__ p, double* out) {
  if constexpr (METHOD == INFLX_BG_RKF) {
    double e[INFLX_TR_NC];
    inflx_tr_rkf(s.y, s.f, h, p, s.eps_star, out, e);
    return adaptive ? inflx_tr_norm8(e) : 0.0;
  } else {
    if (!adaptive) {
      inflx_tr_rk4(s.y, s.f, h, p, s.eps_star, out);
      return 0.0;
    }
    double big[INFLX_TR_NC], half[INFLX_TR_NC], fh[INFLX_TR_NC], kin, e[INFLX_TR_NC];
    inflx_tr_rk4(s.y, s.f, h, p, s.eps_star, big);
    const double h2 = 0.5 * h;
    inflx_tr_rk4(s.y, s.f, h2, p, s.eps_star, half);
    inflx_tr_rhs(half, p, s.eps_star, fh, kin);
    inflx_tr_rk4(half, fh, h2, p, s.eps_star, out);
#pragma unroll
    for (int c = 0; c < INFLX_TR_NC; ++c) e[c] = fabs(out[c] - big[c]);
    return inflx_tr_norm8(e);
  }
}

// One accepted step, inflx_bg_step_taken over nine components.  `frac_end`: the fraction of the step at which epsilon_H = 1 when
// stop_at_end ends the lane, n_end = n0 + frac_end (N1 - n0).
template <int METHOD>
INFLX_FN int inflx_tr_step_taken(InflxTrLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end, double& n_end,
                                 double& h_taken, double& frac_end) {
  const bool adaptive = !(fixed_dt > 0.0);
  const double eps0 = inflx_tr_epsilon(s), n0 = s.y[5];
  double y1[INFLX_TR_NC];
  int rejections = 0;
  for (;;) {
    if (s.t + s.dt == s.t) return INFLX_BG_UNDERFLOW;
    const double err = inflx_tr_trial<METHOD>(s, s.dt, adaptive, p, y1);
    const bool finite = inflx_tr_finite9(y1) && isfinite(err);
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
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) s.y[c] = y1[c];
  inflx_tr_rhs(s.y, p, s.eps_star, s.f, s.kin);
  if (!(inflx_tr_finite9(s.f) && isfinite(s.kin))) return INFLX_BG_NONFINITE;
  if (stop_at_end) {
    const double eps1 = inflx_tr_epsilon(s);
    if (eps1 >= 1.0) {
      frac_end = (1.0 - eps0) / (eps1 - eps0);  // (eps0 < 1: a lane that starts at or past the end ends in init)
      n_end = n0 + frac_end * (s.y[5] - n0);
      return INFLX_BG_ENDED;
    }
  }
  return INFLX_BG_RUNNING;
}

// The initial state of a lane with samples: inflx_bg_init's background state, eps_star, (q, u, r) = (1, H0 dq_dN, 0) -- dq_dN the
// caller's when `has_dq`, the documented root otherwise -- and the right-hand side there.  A sample equal to 0 is the initial state
// (T_SS = 1, T_RS = 0); it does not stop the lane, even when it was the only sample.  `ends` = (T_SS_end, T_RS_end), set when the
// lane ends.
template <class SINK>
INFLX_FN int inflx_tr_init(InflxTrLane& s, const double* init, const double* __restrict__ p, double dt0, bool stop_at_end, bool has_dq, double dq_dn,
                           const double* __restrict__ samples, unsigned n_samples, unsigned& cursor, double& n_end, double* ends, SINK& sink) {
  cursor = 0;
  InflxBgLane b;
  const int st = inflx_bg_init(b, init, p, dt0, stop_at_end, n_end);
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    s.y[c] = b.y[c];
    s.f[c] = b.f[c];
  }
  s.y[INFLX_TR_Q] = s.y[INFLX_TR_U] = s.y[INFLX_TR_R] = 0.0;
  s.f[INFLX_TR_Q] = s.f[INFLX_TR_U] = s.f[INFLX_TR_R] = 0.0;
  s.kin = b.kin;
  s.t = b.t;
  s.dt = b.dt;
  s.eps_star = 0.0;
  if (st == INFLX_BG_NONFINITE) return st;
  double k[2], m[4];
  inflx_kin_point(s.y[0], s.y[1], s.y[2], s.y[3], p, k);
  inflx_mass_point(s.y[0], s.y[1], s.y[2], s.y[3], p, m);
  const double H = s.y[4], kin = s.kin;
  const double eps_star = 0.5 * kin / (H * H);
  const double omega = k[1] / (kin * H);
  const double mu = m[2] / kin / (H * H) + eps_star * m[3] + 3.0 * (omega * omega);
  if (kin == 0.0 || !(isfinite(eps_star) && isfinite(omega) && isfinite(mu))) return INFLX_BG_NONFINITE;
  s.eps_star = eps_star;
  if (!has_dq) {
    const double b1 = 3.0 - eps_star, disc = b1 * b1 - 4.0 * mu;
    dq_dn = disc >= 0.0 ? 0.5 * (sqrt(disc) - b1) : -0.5 * b1;
  }
  s.y[INFLX_TR_Q] = 1.0;
  s.y[INFLX_TR_U] = H * dq_dn;
  s.y[INFLX_TR_R] = 0.0;
  inflx_tr_rhs(s.y, p, s.eps_star, s.f, s.kin);
  if (!(inflx_tr_finite9(s.y) && inflx_tr_finite9(s.f) && isfinite(s.kin))) return INFLX_BG_NONFINITE;
  if (st == INFLX_BG_ENDED) {
    ends[0] = 1.0;
    ends[1] = 0.0;
  }
  if (n_samples > 0 && samples[0] == 0.0) {
    InflxTrSample out;
#pragma unroll
    for (int c = 0; c < 6; ++c) out.loc.y[c] = s.y[c];
    out.loc.t = s.t;
    out.loc.eps = inflx_tr_epsilon(s);
    out.t_ss = 1.0;
    out.t_rs = 0.0;
    sink(0u, out);
    cursor = 1;
  }
  return st;
}

// One accepted step of a lane and every sample (an e-fold count) that step passed, as inflx_bg_step_sampled emits them; in the step
// that ends inflation only the samples up to N_end, and `ends` = (T_SS_end, T_RS_end).  Returns INFLX_BG_TARGET when this step emitted
// the last sample, INFLX_BG_NONFINITE when a located state or a transfer function there is not finite (that sample is not emitted), and
// inflx_tr_step_taken's status otherwise.
template <int METHOD, class SINK>
INFLX_FN int inflx_tr_step_sampled(InflxTrLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end,
                                   const double* __restrict__ samples, unsigned n_samples, unsigned& cursor, double& n_end, double* ends, SINK& sink) {
  double y0[INFLX_TR_NC], f0[INFLX_TR_NC], h = 0.0, frac = 0.0;
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) {
    y0[c] = s.y[c];
    f0[c] = s.f[c];
  }
  const double t0 = s.t;
  bool emitted = false;
  const int st = inflx_tr_step_taken<METHOD>(s, p, max_err, fixed_dt, stop_at_end, n_end, h, frac);
  if (st != INFLX_BG_RUNNING && st != INFLX_BG_ENDED) return st;
  if (st == INFLX_BG_ENDED) {
    const double q_end = y0[INFLX_TR_Q] + frac * (s.y[INFLX_TR_Q] - y0[INFLX_TR_Q]);
    ends[0] = q_end * sqrt(s.eps_star);
    ends[1] = y0[INFLX_TR_R] + frac * (s.y[INFLX_TR_R] - y0[INFLX_TR_R]);
  }
  while (cursor < n_samples) {
    const double x = samples[cursor];
    if (!(s.y[5] >= x)) break;
    if (st == INFLX_BG_ENDED && n_end < x) break;
    InflxTrSample out;
    const double th = inflx_bg_locate(y0[5], f0[5], s.y[5], s.f[5], h, x);
#pragma unroll
    for (int c = 0; c < 5; ++c) out.loc.y[c] = inflx_bg_hermite(y0[c], f0[c], s.y[c], s.f[c], h, th);
    out.loc.y[5] = x;
    out.loc.t = t0 + th * h;
    if (!inflx_bg_located_epsilon(out.loc, p)) return INFLX_BG_NONFINITE;
    const double q_loc = inflx_bg_hermite(y0[INFLX_TR_Q], f0[INFLX_TR_Q], s.y[INFLX_TR_Q], s.f[INFLX_TR_Q], h, th);
    out.t_ss = q_loc * sqrt(s.eps_star / out.loc.eps);
    out.t_rs = inflx_bg_hermite(y0[INFLX_TR_R], f0[INFLX_TR_R], s.y[INFLX_TR_R], s.f[INFLX_TR_R], h, th);
    if (!(isfinite(out.t_ss) && isfinite(out.t_rs))) return INFLX_BG_NONFINITE;
    sink(cursor, out);
    ++cursor;
    emitted = true;
  }
  return emitted && cursor == n_samples ? INFLX_BG_TARGET : st;
}
