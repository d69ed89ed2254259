// Spectra of a mode sampled along its evolution (inflatox_amd.background.spectra_evolution): the lane of csrc/inflx_modes.h -- the
// same 22-component state, equations, steppers, error norm, first dt, rejection and underflow bounds and statuses, all of them through
// inflx_md_init and inflx_md_step_taken, untouched -- which, besides the 22 values where it stops, emits P_R, P_S, C_RS, N, t and
// eps_H at every point of a list of e-fold counts that all lanes of a launch share.
//
// SAMPLES.  `samples` (n_samples, finite, strictly increasing) and a per-lane `shift`: the lane-local sample k is
//     x_k = samples[k] - shift
// by that one subtraction wherever it is formed (here, the host twin, the front end), so that a front end which hands in the target
// n_target = N_eval - shift of csrc/inflx_modes.h gets x_k == n_target exactly for a sample at N_eval.  `cursor` counts the samples
// the lane has passed, emitted or not; it is carried between steps and launches.
//   * x_k < 0: the mode does not exist yet; the sample is passed by inflx_ev_init and never emitted.
//   * x_k == 0: the initial state, P_R = P_S = kappa^2 / (8 pi^2 eps_0) and C_RS = 0 exactly -- inflx_bg_init_sampled's rule with the
//     shift.
//   * otherwise the accepted step that passes x_k emits it: theta from inflx_bg_locate, the five background components and the 16
//     mode components from the cubic Hermite interpolant at theta, eps from the model at the located state, the values through
//     inflx_md_outputs (inflx_ev_located).  These are the statements of inflx_md_step's target emission, and the target emission
//     here goes through the same function: a sample at x_k == n_target is the target's numbers bit for bit, and both are what the
//     lane of csrc/inflx_modes.h emits when it is asked to stop there.
// A step emits every sample with x_k <= N1; the step that ends inflation only those with x_k <= n_end, and the step that reaches the
// target only those with x_k <= n_target ("whichever comes first", as in inflx_md_step).  The lane goes on from the step's end state,
// never from a located one, so its steps are those of the ordinary run.  A sample whose values are not finite stops the lane with
// INFLX_BG_NONFINITE and is not emitted.  After the samples the target and end logic of inflx_md_step runs unchanged; a lane with
// neither a target (NaN) nor stop_at_end stops with INFLX_BG_TARGET once its last sample is passed, and emits no final values.
//
// The sink is called sink(out) with the 22 final values, as csrc/inflx_modes.h calls it, and sink.sample(k, out) with the 22 values
// at sample k, of which the kernels keep INFLX_EV_NSAMPLE: the planes INFLX_EV_SAMPLE_OF.
//
// INFLX_FN code over one lane's registers, so that tests/evolution_twin.cpp compiles the very same text for the host.  Include
// inflx_background.h and inflx_modes.h first.
#pragma once

#define INFLX_EV_NSAMPLE 6  // what a lane keeps of a sample: P_R, P_S, C_RS, local N, local t, eps_H
// the place among inflx_md_outputs' 22 values of sample value c
#define INFLX_EV_SAMPLE_OF(c) ((c) < 3 ? (c) : INFLX_MD_OUT_N + ((c) - 3))

// The 22 values at the local e-fold count x inside the accepted step of size h from (y0, f0, t0) to the lane's state: inflx_md_step's
// target emission.  false: a value is not finite.
INFLX_FN bool inflx_ev_located(const double* y0, const double* f0, double t0, const InflxMdLane& s, double h, const double* __restrict__ p, double x,
                               double* out) {
  InflxBgLocated loc;
  const double th = inflx_bg_locate(y0[5], f0[5], s.y[5], s.f[5], h, x);
#pragma unroll
  for (int c = 0; c < 5; ++c) loc.y[c] = inflx_bg_hermite(y0[c], f0[c], s.y[c], s.f[c], h, th);
  loc.y[5] = x;
  loc.t = t0 + th * h;
  if (!inflx_bg_located_epsilon(loc, p)) return false;
  double md[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) md[c] = inflx_bg_hermite(y0[6 + c], f0[6 + c], s.y[6 + c], s.f[6 + c], h, th);
  return inflx_md_outputs(md, s.kappa, x, loc.t, loc.eps, out);
}

// a lane that has passed its last sample and has nowhere else to stop
INFLX_FN bool inflx_ev_samples_only(unsigned cursor, unsigned n_samples, bool stop_at_end, double n_target) {
  return cursor == n_samples && !stop_at_end && n_target != n_target;
}

// inflx_md_init for a lane with samples: the samples before the lane's start are passed, and a sample at its start is the initial
// state (also of a lane that ends or reaches its target there).
template <class SINK>
INFLX_FN int inflx_ev_init(InflxMdLane& s, const double* init, const double* __restrict__ p, double dt0, bool stop_at_end, double kappa, double n_target,
                           const double* __restrict__ samples, unsigned n_samples, double shift, unsigned& cursor, double& n_end, SINK& sink) {
  cursor = 0;
  const int st = inflx_md_init(s, init, p, dt0, stop_at_end, kappa, n_target, n_end, sink);
  if (st == INFLX_BG_NONFINITE) return st;
  while (cursor < n_samples && samples[cursor] - shift < 0.0) ++cursor;
  if (cursor < n_samples && samples[cursor] - shift == 0.0) {
    double out[INFLX_MD_NOUT];
    if (!inflx_md_outputs(s.y + INFLX_MD_Q, kappa, 0.0, s.t, inflx_md_epsilon(s), out)) return INFLX_BG_NONFINITE;
    sink.sample(cursor, out);
    ++cursor;
  }
  return st == INFLX_BG_RUNNING && inflx_ev_samples_only(cursor, n_samples, stop_at_end, n_target) ? INFLX_BG_TARGET : st;
}

// One accepted step of a lane with samples: inflx_md_step with the samples the step passed emitted before the final values.
template <int METHOD, class SINK>
INFLX_FN int inflx_ev_step(InflxMdLane& s, const double* __restrict__ p, double max_err, double fixed_dt, bool stop_at_end, double n_target,
                           const double* __restrict__ samples, unsigned n_samples, double shift, unsigned& cursor, double& n_end, SINK& sink) {
  double y0[INFLX_MD_NC], f0[INFLX_MD_NC], h = 0.0, frac = 0.0;
#pragma unroll
  for (int c = 0; c < INFLX_MD_NC; ++c) {
    y0[c] = s.y[c];
    f0[c] = s.f[c];
  }
  const double t0 = s.t;
  const int st = inflx_md_step_taken<METHOD>(s, p, max_err, fixed_dt, stop_at_end, n_end, h, frac);
  if (st != INFLX_BG_RUNNING && st != INFLX_BG_ENDED) return st;
  const bool hit = s.y[5] >= n_target && !(st == INFLX_BG_ENDED && n_end < n_target);  // (a NaN target is never hit)
  double md[16], out[INFLX_MD_NOUT];
  while (cursor < n_samples) {
    const double x = samples[cursor] - shift;
    if (!(s.y[5] >= x)) break;
    if (st == INFLX_BG_ENDED && n_end < x) break;
    if (hit && n_target < x) break;
    if (!inflx_ev_located(y0, f0, t0, s, h, p, x, out)) return INFLX_BG_NONFINITE;
    sink.sample(cursor, out);
    ++cursor;
  }
  if (!hit && st == INFLX_BG_RUNNING) return inflx_ev_samples_only(cursor, n_samples, stop_at_end, n_target) ? INFLX_BG_TARGET : st;
  if (hit) {
    if (!inflx_ev_located(y0, f0, t0, s, h, p, n_target, out)) return INFLX_BG_NONFINITE;
    sink(out);
    return INFLX_BG_TARGET;
  }
#pragma unroll
  for (int c = 0; c < 16; ++c) md[c] = y0[6 + c] + frac * (s.y[6 + c] - y0[6 + c]);
  if (!inflx_md_outputs(md, s.kappa, n_end, t0 + frac * h, 1.0, out)) return INFLX_BG_NONFINITE;
  sink(out);
  return INFLX_BG_ENDED;
}
