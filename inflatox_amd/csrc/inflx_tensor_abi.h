// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_mode_spectra with INFLX_MODES_TENSOR) and the tensor-mode kernels
// (csrc/inflx_tensor_kernels.hip): the kernels' argument block, the carry planes and the output planes.  Both sides include this
// header; the tensor object exports INFLX_TN_ABI, and the host refuses an object whose value differs from its own.  The layout word
// is the tensor object's own: the background, kinematics, masses, transfer and modes objects' are not involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_TN_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_TN_ABI_VERSION
#define INFLX_TN_ABI_VERSION 1
#endif

// the artefact ABI major a tensor object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there and
// here with -DINFLX_ABI_VERSION_MAJOR, which the tensor object is built with whenever the core object is)
#define INFLX_TN_DEFAULT_ABI_MAJOR 5

#define INFLX_TN_THREADS 256
#define INFLX_TN_OUT_PLANES 8  // P_T; the 4 mode components Re ht, Im ht, Re pt, Im pt (csrc/inflx_tensor.h y[6..9]); N; t; eps_H

// carry planes [plane][lane] between launches
enum InflxTnCarry {
  INFLX_TN_CARRY_Y = 0,  // 0..9: the lane state of csrc/inflx_tensor.h
  INFLX_TN_CARRY_T = 10,
  INFLX_TN_CARRY_DT = 11,
  INFLX_TN_CARRY_NEND = 12,  // N at epsilon_H = 1 (NaN until the lane ends there)
  INFLX_TN_CARRY_STATUS = 13,
  INFLX_TN_CARRY_PLANES = 14,  // (inflx_mode_spectra reads back NEND and STATUS, [12, 14))
};

// Argument block of inflx_tn_init and inflx_tn_advance_*: the fields of InflxMdArgs (csrc/inflx_modes_abi.h).  A launch of the
// advance kernels takes at most `steps` accepted steps of every lane that still runs, skips a lane that has stopped, and adds the
// number of lanes still running after the launch to *running.  A lane emits its INFLX_TN_OUT_PLANES values into
// out[plane * n + lane] in the step that stops it with INFLX_BG_TARGET or INFLX_BG_ENDED.  The host fills `out` with NaN first: a
// lane that stops otherwise keeps NaN.
struct InflxTnArgs {
  const double* p;         // parameter rows of lane 0 of this launch
  uint64_t p_stride;       // doubles between the parameter rows of two lanes (0: one row for all)
  const double* init;      // (n, 4): phi^0, phi^1, chi^0, chi^1 (init kernel)
  const double* kappa;     // (n,): k / a at the lane's start
  const double* n_target;  // (n,): the e-fold count since the lane's start at which it is evaluated; NaN: no target
  double* carry;           // [INFLX_TN_CARRY_PLANES][n]
  double* out;             // [INFLX_TN_OUT_PLANES][n]
  uint32_t* running;       // one word, += the lanes still running when the launch ends
  uint64_t n;              // lanes
  uint32_t steps;          // accepted steps this launch takes at most (at most INFLX_BG_STEPS_PER_LAUNCH)
  uint32_t flags;          // bit 0: stop at epsilon_H = 1
  double max_err;
  double fixed_dt;         // > 0: fixed step
};
static_assert(sizeof(InflxTnArgs) == 96, "InflxTnArgs layout");
static_assert(offsetof(InflxTnArgs, p) == 0 && offsetof(InflxTnArgs, p_stride) == 8 && offsetof(InflxTnArgs, init) == 16 &&
                  offsetof(InflxTnArgs, kappa) == 24 && offsetof(InflxTnArgs, n_target) == 32 && offsetof(InflxTnArgs, carry) == 40 &&
                  offsetof(InflxTnArgs, out) == 48 && offsetof(InflxTnArgs, running) == 56 && offsetof(InflxTnArgs, n) == 64 &&
                  offsetof(InflxTnArgs, steps) == 72 && offsetof(InflxTnArgs, flags) == 76 && offsetof(InflxTnArgs, max_err) == 80 &&
                  offsetof(InflxTnArgs, fixed_dt) == 88,
              "InflxTnArgs layout");
