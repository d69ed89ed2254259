// Tensor modes and the tensor power spectrum P_T of a two-field model (inflatox_amd.background.tensor_spectra): the background
// trajectory and, carried along it from the Bunch-Davies vacuum deep inside the horizon, one complex tensor amplitude of one
// wavenumber.
//
// CONVENTIONS (reduced Planck units, cosmic time: the units of dH/dt = V - 3 H^2).  u = h / 2 is the canonically normalised
// amplitude of one polarisation, u'' + 3 H u' + (k / a)^2 u = 0: the equation of a massless spectator.  In the scaled variables of
// csrc/inflx_modes.h, with the physical wavenumber k / a = kappa e^-N, N the lane's own e-fold count from its start and kappa = k / a
// at the lane's start:
//     ht = a_in sqrt(2 k) u        pt = d ht/dt
//     d ht/dt = pt                 d pt/dt = -3 H pt - kappa^2 e^-2N ht
// complex, stored as real and imaginary parts; at the start ht = 1 and pt = -i kappa - H_in.  The Wronskian
// e^3N (ht conj(pt) - pt conj(ht)) = 2 i kappa is conserved.
//
// Lane state: the background's y[0..5] = (phi^0, phi^1, chi^0, chi^1, H, N) (csrc/inflx_background.h), then
//     y[6], y[7] = Re, Im ht       y[8], y[9] = Re, Im pt
// 10 components.
//
// Spectrum, where the lane stops, both polarisations counted:
//     P_T = 2 kappa^2 |ht|^2 / pi^2
// (P_T = 8 k^3 |u|^2 / (2 pi^2) and k^3 |u|^2 = kappa^2 |ht|^2 / 2 with a = 1 at the lane's start; 2 H^2 / pi^2 in de Sitter.)  With
// csrc/inflx_modes.h's P_R = kappa^2 sum |Qt|^2 / (8 pi^2 eps), r = P_T / P_R is 16 eps in single-field slow roll.
//
// Steppers: inflx_background.h's over 10 components -- the same tableaux, acceptance rule (err <= 1.1 max_err), step factor, first
// dt, rejection and underflow bounds and statuses, and for the first six components the very expressions of inflx_bg_rhs,
// inflx_bg_rkf and inflx_bg_rk4, so that with a fixed dt the background part is solve_eom_sampled's bit for bit.  The ERROR NORM is
// the absolute Euclidean norm over phi, chi, H, the two components of ht and the two of pt / kappa (both O(1) at the start): 9
// components, N excluded.
//
// Stop rules: inflx_md_step's.  INFLX_BG_TARGET at the lane's own local e-fold target (NaN: none), located with inflx_bg_locate and
// the cubic Hermite interpolant for all 10 components, eps from the model at the located state; a target <= 0 is reached by the
// initial state.  INFLX_BG_ENDED with stop_at_end: the outputs are linear across the step that ends inflation at N_end's own fraction
// f = (1 - eps0) / (eps1 - eps0), with eps = 1; when the step passes the target as well, whichever comes first decides.  A lane that
// is past the end at the start ends there with its initial mode.  A lane whose steps run out emits nothing.  A lane AT REST at the
// start (kin = 0) runs like any other: a tensor mode needs no direction in field space and P_T does not divide by eps.  A lane whose
// state or right-hand side is not finite, or whose kappa is not a positive finite number, stops with INFLX_BG_NONFINITE and emits
// nothing.
//
// INFLX_FN code over one lane's registers, so that tests/tensor_twin.cpp compiles the very same text for the host.  The model enters
// through the generated inflx_eom_point alone.  Include inflx_background.h first.
#pragma once

#define INFLX_TN_NC 10   // components of the lane state
#define INFLX_TN_H 6     // first component of ht
#define INFLX_TN_P 8     // first component of pt
#define INFLX_TN_NOUT 8  // what a lane emits: P_T, the 4 mode components y[6..9], N, t, eps

enum InflxTnOut { INFLX_TN_OUT_PT = 0, INFLX_TN_OUT_MODES = 1, INFLX_TN_OUT_N = 5, INFLX_TN_OUT_T = 6, INFLX_TN_OUT_EPS = 7 };

// One lane: the state, the right-hand side at it (k1 of the next step, and kin there), t, dt and kappa.
struct InflxTnLane {
  double y[INFLX_TN_NC];
  double f[INFLX_TN_NC];
  double kin;
  double t;
  double dt;
  double kappa;
};

// dy/dt at y over 10 components; kin = G_ab chi^a chi^b.  f[0..5] are inflx_bg_rhs's.  Inlined, as the plain background kernels
// inline inflx_bg_rhs (DESIGN.md section 12 has the register figures).
INFLX_FN void inflx_tn_rhs(const double* y, const double* __restrict__ p, double kappa, double* f, double& kin) {
  inflx_bg_rhs(y, p, f, kin);
  const double k2 = (kappa * kappa) * exp(-2.0 * y[5]);
  const double h3 = 3.0 * y[4];
  f[6] = y[8];
  f[7] = y[9];
  f[8] = -h3 * y[8] - k2 * y[6];
  f[9] = -h3 * y[9] - k2 * y[7];
}

INFLX_FN bool inflx_tn_finite(const double* v) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) ok = ok && isfinite(v[c]);
  return ok;
}

// eps_H = (G_ab chi^a chi^b / 2) / H^2: inflx_bg_epsilon's expression
INFLX_FN double inflx_tn_epsilon(const InflxTnLane& s) { return 0.5 * s.kin / (s.y[4] * s.y[4]); }

// the right-hand side at the lane's state again (a launch resumes from a carried state)
INFLX_FN void inflx_tn_resume(InflxTnLane& s, const double* __restrict__ p) { inflx_tn_rhs(s.y, p, s.kappa, s.f, s.kin); }

// one classical RK4 step of size h from (y, f0 = f(y)): inflx_bg_rk4 over 10 components
INFLX_FN void inflx_tn_rk4(const double* y, const double* f0, double h, const double* __restrict__ p, double kappa, double* out) {
  double k2[INFLX_TN_NC], k3[INFLX_TN_NC], k4[INFLX_TN_NC], ys[INFLX_TN_NC], kin;
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) ys[c] = y[c] + h * (0.5 * f0[c]);
  inflx_tn_rhs(ys, p, kappa, k2, kin);
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) ys[c] = y[c] + h * (0.5 * k2[c]);
  inflx_tn_rhs(ys, p, kappa, k3, kin);
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) ys[c] = y[c] + h * (1.0 * k3[c]);
  inflx_tn_rhs(ys, p, kappa, k4, kin);
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) {
    double acc = (1.0 / 6.0) * f0[c];
    acc += (1.0 / 3.0) * k2[c];
    acc += (1.0 / 3.0) * k3[c];
    acc += (1.0 / 6.0) * k4[c];
    out[c] = y[c] + h * acc;
  }
}

// Fehlberg 4(5), inflx_bg_rkf over 10 components: out = 4th-order state, e = |5th - 4th| per component
INFLX_FN void inflx_tn_rkf(const double* y, const double* f0, double h, const double* __restrict__ p, double kappa, double* out, double* e) {
  double k[6][INFLX_TN_NC], ys[INFLX_TN_NC], kin;
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) k[0][c] = f0[c];
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
    for (int c = 0; c < INFLX_TN_NC; ++c) {
      double acc = A[s][0] * k[0][c];
#pragma unroll
      for (int j = 1; j < s; ++j) acc += A[s][j] * k[j][c];
      ys[c] = y[c] + h * acc;
    }
    inflx_tn_rhs(ys, p, kappa, k[s], kin);
  }
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) {
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

// the error norm: phi, chi, H, the two components of ht and the two of pt / kappa -- 9 components, N (component 5) excluded
INFLX_FN double inflx_tn_norm(const double* e, double kappa) {
  double acc = e[0] * e[0];
#pragma unroll
  for (int c = 1; c < 5; ++c) acc += e[c] * e[c];
#pragma unroll
  for (int c = INFLX_TN_H; c < INFLX_TN_P; ++c) acc += e[c] * e[c];
#pragma unroll
  for (int c = INFLX_TN_P; c < INFLX_TN_NC; ++c) {
    const double s = e[c] / kappa;
    acc += s * s;
  }
  return sqrt(acc);
}

// a trial step of size h: out = the state it reaches, return value = its error estimate (0 for a fixed step)
template <int METHOD>
INFLX_FN double inflx_tn_trial(const InflxTnLane& s, double h, bool adaptive, const double* __restrict__ p, double* out) {
  if constexpr (METHOD == INFLX_BG_RKF) {
    double e[INFLX_TN_NC];
    inflx_tn_rkf(s.y, s.f, h, p, s.kappa, out, e);
    return adaptive ? inflx_tn_norm(e, s.kappa) : 0.0;
  } else {
    if (!adaptive) {
      inflx_tn_rk4(s.y, s.f, h, p, s.kappa, out);
      return 0.0;
    }
    double big[INFLX_TN_NC], half[INFLX_TN_NC], fh[INFLX_TN_NC], kin, e[INFLX_TN_NC];
    inflx_tn_rk4(s.y, s.f, h, p, s.kappa, big);
    const double h2 = 0.5 * h;
    inflx_tn_rk4(s.y, s.f, h2, p, s.kappa, half);
    inflx_tn_rhs(half, p, s.kappa, fh, kin);
    inflx_tn_rk4(half, fh, h2, p, s.kappa, out);
#pragma unroll
    for (int c = 0; c < INFLX_TN_NC; ++c) e[c] = fabs(out[c] - big[c]);
    return inflx_tn_norm(e, s.kappa);
  }
}

// One accepted step, inflx_bg_step_taken over 10 components.  `frac_end`: the fraction of the step at which epsilon_H = 1 when
// stop_at_end ends the lane, n_end = n0 + frac_end (N1 - n0).
template <int METHOD>
INFLX_FN int inflx_tn_step_taken(InflxTnLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end, double& n_end,
                                 double& h_taken, double& frac_end) {
  const bool adaptive = !(fixed_dt > 0.0);
  const double eps0 = inflx_tn_epsilon(s), n0 = s.y[5];
  double y1[INFLX_TN_NC];
  int rejections = 0;
  for (;;) {
    if (s.t + s.dt == s.t) return INFLX_BG_UNDERFLOW;
    const double err = inflx_tn_trial<METHOD>(s, s.dt, adaptive, p, y1);
    const bool finite = inflx_tn_finite(y1) && isfinite(err);
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
  for (int c = 0; c < INFLX_TN_NC; ++c) s.y[c] = y1[c];
  inflx_tn_rhs(s.y, p, s.kappa, s.f, s.kin);
  if (!(inflx_tn_finite(s.f) && isfinite(s.kin))) return INFLX_BG_NONFINITE;
  if (stop_at_end) {
    const double eps1 = inflx_tn_epsilon(s);
    if (eps1 >= 1.0) {
      frac_end = (1.0 - eps0) / (eps1 - eps0);  // (eps0 < 1: a lane that starts at or past the end ends in init)
      n_end = n0 + frac_end * (s.y[5] - n0);
      return INFLX_BG_ENDED;
    }
  }
  return INFLX_BG_RUNNING;
}

// what a lane emits from the 4 mode components `md` (ht first), N, t and eps at the evaluation point; false: a value is not finite
INFLX_FN bool inflx_tn_outputs(const double* md, double kappa, double n, double t, double eps, double* out) {
  constexpr double pi = 3.14159265358979323846;
  out[INFLX_TN_OUT_PT] = 2.0 * (kappa * kappa) * (md[0] * md[0] + md[1] * md[1]) / (pi * pi);
  bool ok = isfinite(out[INFLX_TN_OUT_PT]) && isfinite(n) && isfinite(t) && isfinite(eps);
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    out[INFLX_TN_OUT_MODES + c] = md[c];
    ok = ok && isfinite(md[c]);
  }
  out[INFLX_TN_OUT_N] = n;
  out[INFLX_TN_OUT_T] = t;
  out[INFLX_TN_OUT_EPS] = eps;
  return ok;
}

// The initial state of a lane: inflx_bg_init's background state, ht = 1, pt = -i kappa - H_in, and the right-hand side there.
// INFLX_BG_ENDED (past the end at the start) and INFLX_BG_TARGET (a target <= 0) emit from the initial state.
template <class SINK>
INFLX_FN int inflx_tn_init(InflxTnLane& s, const double* init, const double* __restrict__ p, double dt0, bool stop_at_end, double kappa, double n_target,
                           double& n_end, SINK& sink) {
  InflxBgLane b;
  int st = inflx_bg_init(b, init, p, dt0, stop_at_end, n_end);
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    s.y[c] = b.y[c];
    s.f[c] = b.f[c];
  }
#pragma unroll
  for (int c = 6; c < INFLX_TN_NC; ++c) s.y[c] = s.f[c] = 0.0;
  s.kin = b.kin;
  s.t = b.t;
  s.dt = b.dt;
  s.kappa = kappa;
  if (st == INFLX_BG_NONFINITE) return st;
  if (!(isfinite(kappa) && kappa > 0.0)) return INFLX_BG_NONFINITE;
  s.y[INFLX_TN_H + 0] = 1.0;      // Re ht
  s.y[INFLX_TN_P + 0] = -s.y[4];  // Re pt
  s.y[INFLX_TN_P + 1] = -kappa;   // Im pt
  inflx_tn_rhs(s.y, p, s.kappa, s.f, s.kin);
  if (!(inflx_tn_finite(s.y) && inflx_tn_finite(s.f) && isfinite(s.kin))) return INFLX_BG_NONFINITE;
  if (st == INFLX_BG_RUNNING && n_target <= 0.0) st = INFLX_BG_TARGET;
  if (st != INFLX_BG_RUNNING) {
    double out[INFLX_TN_NOUT];
    if (!inflx_tn_outputs(s.y + INFLX_TN_H, kappa, 0.0, s.t, st == INFLX_BG_ENDED ? 1.0 : inflx_tn_epsilon(s), out)) return INFLX_BG_NONFINITE;
    sink(out);
  }
  return st;
}

// One accepted step of a lane.  Returns INFLX_BG_TARGET when the step reached the lane's target (the outputs at the located state are
// emitted), INFLX_BG_ENDED when it ended inflation first (the outputs at N_end's fraction are emitted), INFLX_BG_NONFINITE when an
// output is not finite (nothing is emitted), and inflx_tn_step_taken's status otherwise.
template <int METHOD, class SINK>
INFLX_FN int inflx_tn_step(InflxTnLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end, double n_target, double& n_end,
                           SINK& sink) {
  double y0[INFLX_TN_NC], f0[INFLX_TN_NC], h = 0.0, frac = 0.0;
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) {
    y0[c] = s.y[c];
    f0[c] = s.f[c];
  }
  const double t0 = s.t;
  const int st = inflx_tn_step_taken<METHOD>(s, p, max_err, fixed_dt, stop_at_end, n_end, h, frac);
  if (st != INFLX_BG_RUNNING && st != INFLX_BG_ENDED) return st;
  const bool hit = s.y[5] >= n_target && !(st == INFLX_BG_ENDED && n_end < n_target);  // (a NaN target is never hit)
  if (!hit && st == INFLX_BG_RUNNING) return st;
  double md[4], out[INFLX_TN_NOUT];
  if (hit) {
    InflxBgLocated loc;
    const double th = inflx_bg_locate(y0[5], f0[5], s.y[5], s.f[5], h, n_target);
#pragma unroll
    for (int c = 0; c < 5; ++c) loc.y[c] = inflx_bg_hermite(y0[c], f0[c], s.y[c], s.f[c], h, th);
    loc.y[5] = n_target;
    loc.t = t0 + th * h;
    if (!inflx_bg_located_epsilon(loc, p)) return INFLX_BG_NONFINITE;
#pragma unroll
    for (int c = 0; c < 4; ++c) md[c] = inflx_bg_hermite(y0[6 + c], f0[6 + c], s.y[6 + c], s.f[6 + c], h, th);
    if (!inflx_tn_outputs(md, s.kappa, n_target, loc.t, loc.eps, out)) return INFLX_BG_NONFINITE;
    sink(out);
    return INFLX_BG_TARGET;
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) md[c] = y0[6 + c] + frac * (s.y[6 + c] - y0[6 + c]);
  if (!inflx_tn_outputs(md, s.kappa, n_end, t0 + frac * h, 1.0, out)) return INFLX_BG_NONFINITE;
  sink(out);
  return INFLX_BG_ENDED;
}
