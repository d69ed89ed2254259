// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_transfer_functions) and the transfer kernels
// (csrc/inflx_transfer_kernels.hip): the kernels' argument block, the carry planes and the output planes.  Both sides include this
// header; the transfer object exports INFLX_TR_ABI, and the host refuses an object whose value differs from its own.  The layout
// word is the transfer object's own: the background, kinematics and masses objects' are not involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_TR_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_TR_ABI_VERSION
#define INFLX_TR_ABI_VERSION 1
#endif

// the artefact ABI major a transfer object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there
// and here with -DINFLX_ABI_VERSION_MAJOR, which the transfer object is built with whenever the core object is)
#define INFLX_TR_DEFAULT_ABI_MAJOR 5

#define INFLX_TR_THREADS 256
#define INFLX_TR_OUT_PLANES 10  // per sample: y[0..5] = phi^0, phi^1, chi^0, chi^1, H, N; t; eps_H; T_SS; T_RS

// carry planes [plane][lane] between launches: the background's (csrc/inflx_background_abi.h) in an order of their own, plus q, u, r,
// eps_star and the two end values
enum InflxTrCarry {
  INFLX_TR_CARRY_Y = 0,        // 0..8: phi^0, phi^1, chi^0, chi^1, H, N, q, u, r
  INFLX_TR_CARRY_T = 9,
  INFLX_TR_CARRY_DT = 10,
  INFLX_TR_CARRY_NEND = 11,    // N at epsilon_H = 1 (NaN until the lane ends there)
  INFLX_TR_CARRY_STATUS = 12,
  INFLX_TR_CARRY_CURSOR = 13,  // the number of samples emitted
  INFLX_TR_CARRY_END_SS = 14,  // T_SS at epsilon_H = 1 (NaN until the lane ends there)
  INFLX_TR_CARRY_END_RS = 15,  // T_RS at epsilon_H = 1 (NaN until the lane ends there)
  INFLX_TR_CARRY_HOST_PLANES = 16,  // the planes inflx_transfer_functions reads back: NEND .. END_RS are [11, 16)
  INFLX_TR_CARRY_EPS_STAR = 16,     // epsilon_H at the initial state
  INFLX_TR_CARRY_PLANES = 17,
};

// Argument block of inflx_tr_init and inflx_tr_advance_*.  A launch of the advance kernels takes at most `steps` accepted steps of
// every lane that still runs, skips a lane that has stopped, and adds the number of lanes still running after the launch to
// *running.  A lane emits sample k -- the ten planes above -- into out[(k * INFLX_TR_OUT_PLANES + plane) * n + lane] from the accepted
// step that passes it.  The host fills `out` with NaN first: a sample that a lane never reaches stays NaN.
struct InflxTrArgs {
  const double* p;        // parameter rows of lane 0 of this launch
  uint64_t p_stride;      // doubles between the parameter rows of two lanes (0: one row for all)
  const double* init;     // (n, 4): phi^0, phi^1, chi^0, chi^1 (init kernel)
  const double* dq_dn;    // (n,): dq/dN at the start (init kernel) -- or NULL: the slowly decaying root
  double* carry;          // [INFLX_TR_CARRY_PLANES][n]
  double* out;            // [sample][INFLX_TR_OUT_PLANES][n]
  const double* samples;  // (n_samples,): e-fold counts, strictly increasing
  uint32_t* running;      // one word, += the lanes still running when the launch ends
  uint64_t n;             // lanes
  uint32_t steps;         // accepted steps this launch takes at most (at most INFLX_BG_STEPS_PER_LAUNCH)
  uint32_t n_samples;     // points in `samples`
  uint32_t flags;         // bit 0: stop at epsilon_H = 1
  uint32_t reserved;
  double max_err;
  double fixed_dt;        // > 0: fixed step
};
static_assert(sizeof(InflxTrArgs) == 104, "InflxTrArgs layout");
static_assert(offsetof(InflxTrArgs, dq_dn) == 24 && offsetof(InflxTrArgs, carry) == 32 && offsetof(InflxTrArgs, out) == 40 &&
                  offsetof(InflxTrArgs, samples) == 48 && offsetof(InflxTrArgs, running) == 56 && offsetof(InflxTrArgs, n) == 64 &&
                  offsetof(InflxTrArgs, steps) == 72 && offsetof(InflxTrArgs, flags) == 80 && offsetof(InflxTrArgs, max_err) == 88 &&
                  offsetof(InflxTrArgs, fixed_dt) == 96,
              "InflxTrArgs layout");
