// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_mode_spectra) and the mode-function kernels
// (csrc/inflx_modes_kernels.hip): the kernels' argument block, the carry planes and the output planes.  Both sides include this
// header; the modes object exports INFLX_MD_ABI, and the host refuses an object whose value differs from its own.  The layout word
// is the modes object's own: the background, kinematics, masses and transfer objects' are not involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_MD_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_MD_ABI_VERSION
#define INFLX_MD_ABI_VERSION 1
#endif

// the artefact ABI major a modes object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there and
// here with -DINFLX_ABI_VERSION_MAJOR, which the modes object is built with whenever the core object is)
#define INFLX_MD_DEFAULT_ABI_MAJOR 5

#define INFLX_MD_THREADS 256
#define INFLX_MD_OUT_PLANES 22  // P_R, P_S, C_RS; the 16 mode components Qt^I_J, Pt^I_J (csrc/inflx_modes.h y[6..21]); N; t; eps_H

// carry planes [plane][lane] between launches
enum InflxMdCarry {
  INFLX_MD_CARRY_Y = 0,  // 0..21: the lane state of csrc/inflx_modes.h
  INFLX_MD_CARRY_T = 22,
  INFLX_MD_CARRY_DT = 23,
  INFLX_MD_CARRY_NEND = 24,  // N at epsilon_H = 1 (NaN until the lane ends there)
  INFLX_MD_CARRY_STATUS = 25,
  INFLX_MD_CARRY_PLANES = 26,  // (inflx_mode_spectra reads back NEND and STATUS, [24, 26))
};

// Argument block of inflx_md_init and inflx_md_advance_*.  A launch of the advance kernels takes at most `steps` accepted steps of
// every lane that still runs, skips a lane that has stopped, and adds the number of lanes still running after the launch to
// *running.  A lane emits its INFLX_MD_OUT_PLANES values into out[plane * n + lane] in the step that stops it with INFLX_BG_TARGET or
// INFLX_BG_ENDED.  The host fills `out` with NaN first: a lane that stops otherwise keeps NaN.
struct InflxMdArgs {
  const double* p;         // parameter rows of lane 0 of this launch
  uint64_t p_stride;       // doubles between the parameter rows of two lanes (0: one row for all)
  const double* init;      // (n, 4): phi^0, phi^1, chi^0, chi^1 (init kernel)
  const double* kappa;     // (n,): k / a at the lane's start
  const double* n_target;  // (n,): the e-fold count since the lane's start at which it is evaluated; NaN: no target
  double* carry;           // [INFLX_MD_CARRY_PLANES][n]
  double* out;             // [INFLX_MD_OUT_PLANES][n]
  uint32_t* running;       // one word, += the lanes still running when the launch ends
  uint64_t n;              // lanes
  uint32_t steps;          // accepted steps this launch takes at most (at most INFLX_BG_STEPS_PER_LAUNCH)
  uint32_t flags;          // bit 0: stop at epsilon_H = 1
  double max_err;
  double fixed_dt;         // > 0: fixed step
};
static_assert(sizeof(InflxMdArgs) == 96, "InflxMdArgs layout");
static_assert(offsetof(InflxMdArgs, kappa) == 24 && offsetof(InflxMdArgs, n_target) == 32 && offsetof(InflxMdArgs, carry) == 40 &&
                  offsetof(InflxMdArgs, out) == 48 && offsetof(InflxMdArgs, running) == 56 && offsetof(InflxMdArgs, n) == 64 &&
                  offsetof(InflxMdArgs, steps) == 72 && offsetof(InflxMdArgs, flags) == 76 && offsetof(InflxMdArgs, max_err) == 80 &&
                  offsetof(InflxMdArgs, fixed_dt) == 88,
              "InflxMdArgs layout");
