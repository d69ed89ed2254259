// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_mode_evolution) and the evolution kernels
// (csrc/inflx_evolution_kernels.hip): the kernels' argument block, the carry planes and the two kinds of output planes.  Both sides
// include this header; the evolution object exports INFLX_EV_ABI, and the host refuses an object whose value differs from its own.
// The layout word is the evolution object's own: the modes object's (csrc/inflx_modes_abi.h) is not involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_EV_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_EV_ABI_VERSION
#define INFLX_EV_ABI_VERSION 1
#endif

// the artefact ABI major an evolution object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there
// and here with -DINFLX_ABI_VERSION_MAJOR, which the evolution object is built with whenever the core object is)
#define INFLX_EV_DEFAULT_ABI_MAJOR 5

#define INFLX_EV_THREADS 256
#define INFLX_EV_OUT_PLANES 22    // the final values: those of csrc/inflx_modes_abi.h
#define INFLX_EV_SAMPLE_PLANES 6  // per sample: P_R, P_S, C_RS, the lane's local N, its local t, eps_H

// carry planes [plane][lane] between launches: the modes object's 26 and the sample cursor
enum InflxEvCarry {
  INFLX_EV_CARRY_Y = 0,  // 0..21: the lane state of csrc/inflx_modes.h
  INFLX_EV_CARRY_T = 22,
  INFLX_EV_CARRY_DT = 23,
  INFLX_EV_CARRY_NEND = 24,  // N at epsilon_H = 1 (NaN until the lane ends there)
  INFLX_EV_CARRY_STATUS = 25,
  INFLX_EV_CARRY_CURSOR = 26,  // the samples the lane has passed (a count, stored as a double)
  INFLX_EV_CARRY_PLANES = 27,  // (inflx_mode_evolution reads back NEND and STATUS, [24, 26))
};

// Argument block of inflx_ev_init and inflx_ev_advance_*: InflxMdArgs' fields, then the samples.  A launch of the advance kernels
// takes at most `steps` accepted steps of every lane that still runs, skips a lane that has stopped, and adds the number of lanes still
// running after the launch to *running.  A lane emits sample k -- the local e-fold count samples[k] - shift[lane] -- into
// sampled[(k * INFLX_EV_SAMPLE_PLANES + plane) * n + lane] from the step that passes it, and its INFLX_EV_OUT_PLANES final values into
// out[plane * n + lane] in the step that stops it with INFLX_BG_TARGET or INFLX_BG_ENDED.  The host fills both with NaN first; every
// value is written at most once.
struct InflxEvArgs {
  const double* p;         // parameter rows of lane 0 of this launch
  uint64_t p_stride;       // doubles between the parameter rows of two lanes (0: one row for all)
  const double* init;      // (n, 4): phi^0, phi^1, chi^0, chi^1 (init kernel)
  const double* kappa;     // (n,): k / a at the lane's start
  const double* n_target;  // (n,): the e-fold count since the lane's start at which it is evaluated; NaN: no target
  double* carry;           // [INFLX_EV_CARRY_PLANES][n]
  double* out;             // [INFLX_EV_OUT_PLANES][n]
  uint32_t* running;       // one word, += the lanes still running when the launch ends
  uint64_t n;              // lanes
  uint32_t steps;          // accepted steps this launch takes at most (at most INFLX_BG_STEPS_PER_LAUNCH)
  uint32_t flags;          // bit 0: stop at epsilon_H = 1
  double max_err;
  double fixed_dt;         // > 0: fixed step
  const double* shift;     // (n,): what is subtracted from a sample to make it the lane's own
  const double* samples;   // (n_samples,): shared by all lanes, strictly increasing
  double* sampled;         // [n_samples][INFLX_EV_SAMPLE_PLANES][n]
  uint32_t n_samples;
  uint32_t reserved;       // 0
};
static_assert(sizeof(InflxEvArgs) == 128, "InflxEvArgs layout");
static_assert(offsetof(InflxEvArgs, kappa) == 24 && offsetof(InflxEvArgs, n_target) == 32 && offsetof(InflxEvArgs, carry) == 40 &&
                  offsetof(InflxEvArgs, out) == 48 && offsetof(InflxEvArgs, running) == 56 && offsetof(InflxEvArgs, n) == 64 &&
                  offsetof(InflxEvArgs, steps) == 72 && offsetof(InflxEvArgs, flags) == 76 && offsetof(InflxEvArgs, max_err) == 80 &&
                  offsetof(InflxEvArgs, fixed_dt) == 88 && offsetof(InflxEvArgs, shift) == 96 && offsetof(InflxEvArgs, samples) == 104 &&
                  offsetof(InflxEvArgs, sampled) == 112 && offsetof(InflxEvArgs, n_samples) == 120,
              "InflxEvArgs layout");
