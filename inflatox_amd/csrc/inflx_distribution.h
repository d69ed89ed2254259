// First-passage histograms: the distribution P(N) of the e-fold count of csrc/inflx_stochastic.h, on lanes that are used again
// (inflatox_amd.background.stochastic_distribution).
//
// A realisation of a point depends on (seed, stream, r) alone: its Philox counter is (its own accepted-step index, r, stream).  So a
// fixed set of lanes per point can run realisation after realisation.  A lane holds a TICKET t, the index of its realisation among
// the R of this call (r = first_realisation + t).  When the realisation stops, the lane reports (status, N_end), draws the next
// ticket of its point, and -- if that is below R -- starts afresh from the point's initial state through inflx_st_init: the state, dt,
// the right-hand side, the step count and N_end all start over, nothing is inherited.  A ticket >= R retires the lane.  A realisation
// stops with a status other than INFLX_BG_RUNNING, or after max_steps accepted steps, and is then reported as INFLX_BG_RUNNING: the
// verdict inflx_stochastic_efolds gives it.  Reports are counts in integers, which commute: the histogram does not depend on which
// lane ran which realisation, or when.
//
// The bin rule, with lo and scale = bins / (hi - lo) formed once on the host in binary64:
//     k = floor((N - lo) * scale);   N < lo or k < 0: below;   k >= bins: above (so N = hi is above);   else bin k.
// A subtraction, then a multiplication: there is nothing an FMA contraction could fuse, and host, device and numpy agree bit for bit.
// The rule is the definition of the histogram; edges lo + k (hi - lo) / bins are nominal.
//
// inflx_pd_window is one lane's launch: a budget of `budget` units, one per accepted step and one per fresh start.  (The fresh start
// is charged so that a point whose initial state is already past the end of inflation -- every realisation stops at once -- cannot
// draw all its R tickets inside one launch.)  Reporting and drawing go through SINK, so that the kernels (atomics,
// csrc/inflx_distribution_kernels.hip) and the host twin (serial, tests/distribution_twin.cpp) run this very code.
#pragma once
#include "inflx_stochastic.h"

// the slot of N in a point's row [below, bin 0 .. bins - 1, above]
INFLX_FN uint32_t inflx_pd_slot(double n, double lo, double scale, uint32_t bins) {
  if (n < lo) return 0u;
  const double d = n - lo;
  const double k = floor(d * scale);
  if (k < 0.0) return 0u;
  if (!(k < (double)bins)) return bins + 1u;  // (a NaN goes here too; an ENDED lane's N_end is finite)
  return 1u + (uint32_t)k;
}

// what the realisations of one point share
struct InflxPdPoint {
  uint64_t seed;
  uint64_t first;      // first_realisation: ticket t is realisation first + t
  uint64_t R;          // tickets of this call
  uint64_t max_steps;  // accepted steps a realisation may take
  uint32_t stream;
  double noise_scale, dn_max, max_err, fixed_dt;
};

// what a lane carries from launch to launch beside its InflxBgLane (y, t, dt; f and kin are recomputed: inflx_st_resume)
struct InflxPdCarry {
  double n_end;
  uint64_t steps;   // accepted steps of the realisation so far: the Philox step index of its next kick
  uint64_t ticket;  // >= R: the lane is retired
  int status;
};

// One launch of a lane that is not retired: `s` resumed (f and kin valid).  SINK: void report(int status, double n_end) and
// uint64_t draw().  Returns false when the lane has retired.
template <int METHOD, class SINK>
INFLX_FN bool inflx_pd_window(InflxBgLane& s, InflxPdCarry& c, const InflxPdPoint& q, const double* init, const double* __restrict__ p, uint32_t budget,
                              SINK& sink) {
  const double nan = __builtin_nan("");
  for (uint32_t used = 0;;) {
    if (used >= budget) return true;  // (a realisation that stopped on the last unit is reported by the next launch)
    if (c.status != INFLX_BG_RUNNING || c.steps >= q.max_steps) {
      sink.report(c.status, c.n_end);
      c.ticket = sink.draw();
      if (c.ticket >= q.R) return false;
      c.n_end = nan;
      c.steps = 0;
      c.status = inflx_st_init(s, init, p, q.fixed_dt > 0.0 ? q.fixed_dt : INFLX_BG_FIRST_DT, c.n_end);
      ++used;
      continue;
    }
    const InflxStNoise nz = {q.seed, (uint32_t)(q.first + c.ticket), q.stream, q.noise_scale};
    c.status = inflx_st_step<METHOD>(s, p, q.max_err, q.fixed_dt, q.dn_max, nan, nz, c.steps, c.n_end);
    ++c.steps;
    ++used;
  }
}
