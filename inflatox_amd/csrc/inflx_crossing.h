// Horizon crossings: the state of a trajectory where the comoving Hubble scale ln(a H) reaches given values, and the located end of
// inflation (inflatox_amd.background.horizon_crossings, inflation_end).
//
// Units are the stepper's (csrc/inflx_background.h): 3 H^2 = rho, a = 1 at the trajectory's start, so
//     L = ln(a H) = N + ln H,      L_0 = ln H_0.
// A lane has an offset c and all lanes share a strictly increasing list s_0 < s_1 < ...; the lane's targets are tau_j = c + s_j.
// Sample j is emitted from the first accepted step whose end state has L >= tau_j, at the theta in (0, 1] with
//     g(theta) = N(theta) + ln H(theta) - tau_j = 0,
// N and H the cubic Hermite interpolants of the step (inflx_bg_hermite).  All six components of the located state come from the
// interpolant at that theta, t = t0 + theta h, and epsilon_H from the model there; neither N nor H is overwritten, so the residual
// N + ln H - tau is whatever the iteration's stopping rule leaves.  Targets below L_0 belong to modes that were outside the horizon
// before the start: they are counted, not emitted.  The lane goes on from the step's end state, never from a located one, so its
// steps are those of the ordinary run.
//
// The end of inflation is located on the same dense output by inflx_dn_locate_end (csrc/inflx_deltan.h), which returns the whole
// state where epsilon_H = 1.
//
// Everything is INFLX_FN code over one lane's registers, so that tests/crossing_twin.cpp compiles the very same code for the host.
// Include csrc/inflx_background.h and csrc/inflx_deltan.h first.
#pragma once

// theta in [0, 1] with N(theta) + ln H(theta) = tau, for L(0) < tau <= L(1): Newton's iteration on the two interpolants, kept inside
// a bracket [lo, hi] with g(lo) < 0 <= g(hi) that every finite iterate tightens; an iterate that leaves the bracket is replaced by the
// bracket's midpoint, and so is the successor of an iterate at which g is not finite (an interpolated H <= 0 has no logarithm).  At
// most INFLX_BG_MAX_LOCATE iterations, with inflx_bg_locate's stopping rule.
INFLX_FN double inflx_hx_locate(double n0, double dn0, double n1, double dn1, double H0, double dH0, double H1, double dH1, double h, double tau) {
  double lo = 0.0, hi = 1.0;
  const double l0 = n0 + log(H0), l1 = n1 + log(H1);
  double th = (tau - l0) / (l1 - l0);
  if (!(th > 0.0)) th = 0.0;
  if (th > 1.0) th = 1.0;
  for (int it = 0; it < INFLX_BG_MAX_LOCATE; ++it) {
    const double Hth = inflx_bg_hermite(H0, dH0, H1, dH1, h, th);
    const double g = inflx_bg_hermite(n0, dn0, n1, dn1, h, th) + log(Hth) - tau;
    if (g == 0.0) break;
    double next = 0.5 * (lo + hi);
    if (isfinite(g)) {
      if (g < 0.0)
        lo = th;
      else
        hi = th;
      next = th - g / (inflx_bg_hermite_slope(n0, dn0, n1, dn1, h, th) + inflx_bg_hermite_slope(H0, dH0, H1, dH1, h, th) / Hth);
      if (!(next > lo && next < hi)) next = 0.5 * (lo + hi);
    }
    const double moved = fabs(next - th);
    th = next;
    if (moved <= 1e-15 || hi - lo <= 1e-15) break;
  }
  return th;
}

// inflx_bg_init for a lane with crossings.  The targets below L_0 = ln H_0 are skipped and counted in `n_before`; a target equal to
// L_0 is the initial state (also of a lane that is already past the end of inflation, which ends here as in inflx_bg_init).
// `cursor` is the index of the next target, the skipped ones included.  INFLX_BG_TARGET when no target is left.
template <class SINK>
INFLX_FN int inflx_hx_init_crossings(InflxBgLane& s, const double* init, const double* __restrict__ p, double dt0, bool stop_at_end, double offset,
                                     const double* __restrict__ samples, unsigned n_samples, unsigned& cursor, unsigned& n_before, double& n_end, SINK& sink) {
  cursor = 0;
  n_before = 0;
  const int st = inflx_bg_init(s, init, p, dt0, stop_at_end, n_end);
  if (st == INFLX_BG_NONFINITE) return st;
  const double l0 = s.y[5] + log(s.y[4]);
  while (cursor < n_samples && offset + samples[cursor] < l0) {
    ++cursor;
    ++n_before;
  }
  if (cursor < n_samples && offset + samples[cursor] == l0) {
    InflxBgLocated loc;
    for (int c = 0; c < 6; ++c) loc.y[c] = s.y[c];
    loc.t = s.t;
    loc.eps = inflx_bg_epsilon(s);
    sink(cursor, loc);
    ++cursor;
  }
  return st == INFLX_BG_RUNNING && cursor == n_samples ? INFLX_BG_TARGET : st;
}

// One accepted step of a lane with crossings, and every target that step reached: those with tau <= L of the new state.  In the
// step that ends inflation (stop_at_end) only the crossings whose located N is <= n_end are emitted, inflx_bg_step_sampled's rule.
// Returns INFLX_BG_TARGET once no target is left, INFLX_BG_NONFINITE when a located state is not finite or has H <= 0 (that sample is
// not emitted), and inflx_bg_step_taken's status otherwise.
template <int METHOD, class SINK>
INFLX_FN int inflx_hx_step_crossings(InflxBgLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end, double offset,
                                     const double* __restrict__ samples, unsigned n_samples, unsigned& cursor, double& n_end, SINK& sink) {
  double y0[6], f0[6], h = 0.0;
  for (int c = 0; c < 6; ++c) {
    y0[c] = s.y[c];
    f0[c] = s.f[c];
  }
  const double t0 = s.t;
  const int st = inflx_bg_step_taken<METHOD>(s, p, max_err, fixed_dt, stop_at_end, n_end, h);
  if (st != INFLX_BG_RUNNING && st != INFLX_BG_ENDED) return st;
  const double l1 = s.y[5] + log(s.y[4]);
  while (cursor < n_samples) {
    const double tau = offset + samples[cursor];
    if (!(l1 >= tau)) break;
    const double th = inflx_hx_locate(y0[5], f0[5], s.y[5], s.f[5], y0[4], f0[4], s.y[4], s.f[4], h, tau);
    InflxBgLocated loc;
    for (int c = 0; c < 6; ++c) loc.y[c] = inflx_bg_hermite(y0[c], f0[c], s.y[c], s.f[c], h, th);
    loc.t = t0 + th * h;
    if (st == INFLX_BG_ENDED && n_end < loc.y[5]) break;
    if (!(loc.y[4] > 0.0) || !inflx_bg_located_epsilon(loc, p)) return INFLX_BG_NONFINITE;  // (an interpolated H <= 0 has no ln(a H))
    sink(cursor, loc);
    ++cursor;
  }
  return cursor == n_samples ? INFLX_BG_TARGET : st;
}

// inflx_bg_init for a lane that looks for the end of inflation: a lane that starts at or past it ends here, INFLX_BG_ENDED with `loc`
// the initial state (N = 0, t = 0).
INFLX_FN int inflx_hx_init_end(InflxBgLane& s, const double* init, const double* __restrict__ p, double dt0, InflxBgLocated& loc) {
  double n_end = 0.0;
  const int st = inflx_bg_init(s, init, p, dt0, true, n_end);
  if (st != INFLX_BG_ENDED) return st;
  for (int c = 0; c < 6; ++c) loc.y[c] = s.y[c];
  loc.t = s.t;
  loc.eps = inflx_bg_epsilon(s);
  return st;
}

// One accepted step of such a lane; when the new state has epsilon_H >= 1 the lane stops with INFLX_BG_ENDED and `loc` = the state
// of the dense output where epsilon_H = 1 (inflx_dn_locate_end's Illinois iteration), t = t0 + theta h.
template <int METHOD>
INFLX_FN int inflx_hx_step_end(InflxBgLane& s, const double* __restrict__ p, double max_err, double fixed_dt, InflxBgLocated& loc) {
  double y0[6], f0[6], h = 0.0, n_end = 0.0;
  for (int c = 0; c < 6; ++c) {
    y0[c] = s.y[c];
    f0[c] = s.f[c];
  }
  const double t0 = s.t, eps0 = inflx_bg_epsilon(s);
  const int st = inflx_bg_step_taken<METHOD>(s, p, max_err, fixed_dt, false, n_end, h);
  if (st != INFLX_BG_RUNNING) return st;
  const double eps1 = inflx_bg_epsilon(s);
  if (!(eps1 >= 1.0)) return INFLX_BG_RUNNING;
  double th = 1.0;
  if (!inflx_dn_locate_end(y0, f0, s.y, s.f, h, eps0, eps1, p, th, loc)) return INFLX_BG_NONFINITE;
  loc.t = t0 + th * h;
  return isfinite(loc.t) ? (int)INFLX_BG_ENDED : (int)INFLX_BG_NONFINITE;
}
