// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_solve_eom_crossings and inflx_inflation_end) and the crossing kernels
// (csrc/inflx_crossing_kernels.hip): the kernels' argument block, the carry planes and the sample planes.  Both sides include this
// header; the crossing object exports INFLX_HX_ABI, and the host refuses an object whose value differs from its own.  The layout word
// is the crossing object's own: no other companion object's is involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_HX_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_HX_ABI_VERSION
#define INFLX_HX_ABI_VERSION 1
#endif

// the artefact ABI major a crossing object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there and
// here with -DINFLX_ABI_VERSION_MAJOR, which the crossing object is built with whenever the core object is)
#define INFLX_HX_DEFAULT_ABI_MAJOR 5

#define INFLX_HX_THREADS 256
#define INFLX_HX_SAMPLE_PLANES 8  // y[0..5], t, epsilon_H of one sample

// carry planes [plane][lane] between launches
enum InflxHxCarry {
  INFLX_HX_CARRY_Y = 0,        // 0..5: phi^0, phi^1, chi^0, chi^1, H, N -- the state the lane integrates from; inflx_hx_end_*: the located
                               // end state once the lane is INFLX_BG_ENDED
  INFLX_HX_CARRY_T = 6,
  INFLX_HX_CARRY_DT = 7,
  INFLX_HX_CARRY_NEND = 8,     // inflx_hx_advance_*: N at epsilon_H = 1 (NaN until the lane ends there)
  INFLX_HX_CARRY_STATUS = 9,
  INFLX_HX_CARRY_CURSOR = 10,  // index of the lane's next target, those before the start included
  INFLX_HX_CARRY_BEFORE = 11,  // targets below L_0: modes outside the horizon before the start
  INFLX_HX_CARRY_EPS = 12,     // inflx_hx_end_*: epsilon_H at the located end state (NaN until the lane ends)
  INFLX_HX_CARRY_PLANES = 13,
};

// Argument block of inflx_hx_init, inflx_hx_advance_* and inflx_hx_end_*.  With `samples` the lanes look for crossings: lane l has the
// targets offset[l] + samples[j], and sample j goes to out[(j * 8 + c) * n + l], c = 0..7: y[0..5], t, epsilon_H.  The host fills `out`
// with NaN first: a sample that a lane does not emit stays NaN.  Without `samples` (inflx_hx_init, inflx_hx_end_*) the lanes look for the
// end of inflation.  A launch of the advance and end kernels takes at most `steps` accepted steps of every lane that still runs, skips
// a lane that has stopped, and adds the number of lanes still running after the launch to *running.
struct InflxHxArgs {
  const double* p;        // parameter rows of lane 0 of this pass
  uint64_t p_stride;      // doubles between the parameter rows of two lanes (0: one row for all)
  const double* init;     // (n, 4): phi^0, phi^1, chi^0, chi^1 (init kernel)
  double* carry;          // [INFLX_HX_CARRY_PLANES][n]
  double* out;            // [sample][8][n] -- or NULL
  uint64_t n;             // lanes
  uint32_t steps;         // accepted steps this launch takes at most (at most INFLX_BG_STEPS_PER_LAUNCH)
  uint32_t flags;         // bit 0: stop at epsilon_H = 1 (crossings)
  uint32_t n_samples;     // points in `samples`
  uint32_t reserved;
  double max_err;
  double fixed_dt;        // > 0: fixed step
  const double* offset;   // (n,): the offset of every lane's targets -- or NULL
  const double* samples;  // (n_samples,): strictly increasing -- or NULL: the end of inflation
  uint32_t* running;      // one word, += the lanes still running when the launch ends
};
static_assert(sizeof(InflxHxArgs) == 104, "InflxHxArgs layout");
static_assert(offsetof(InflxHxArgs, p_stride) == 8 && offsetof(InflxHxArgs, init) == 16 && offsetof(InflxHxArgs, carry) == 24 && offsetof(InflxHxArgs, out) == 32 &&
                  offsetof(InflxHxArgs, n) == 40 && offsetof(InflxHxArgs, steps) == 48 && offsetof(InflxHxArgs, flags) == 52 &&
                  offsetof(InflxHxArgs, n_samples) == 56 && offsetof(InflxHxArgs, max_err) == 64 && offsetof(InflxHxArgs, fixed_dt) == 72 &&
                  offsetof(InflxHxArgs, offset) == 80 && offsetof(InflxHxArgs, samples) == 88 && offsetof(InflxHxArgs, running) == 96,
              "InflxHxArgs layout");
