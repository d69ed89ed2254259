// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_reheating) and the reheating kernels
// (csrc/inflx_reheating_kernels.hip): the kernels' argument block and the carry planes.  Both sides include this header; the
// reheating object exports INFLX_RH_ABI, and the host refuses an object whose value differs from its own.  The layout word is the
// reheating object's own: no other companion object's is involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_RH_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_RH_ABI_VERSION
#define INFLX_RH_ABI_VERSION 1
#endif

// the artefact ABI major a reheating object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there
// and here with -DINFLX_ABI_VERSION_MAJOR, which the reheating object is built with whenever the core object is)
#define INFLX_RH_DEFAULT_ABI_MAJOR 5

#define INFLX_RH_THREADS 256

// carry planes [plane][lane] between launches
enum InflxRhCarry {
  INFLX_RH_CARRY_Y = 0,  // 0..6: phi^0, phi^1, chi^0, chi^1, H, N, rho_r -- the state the lane integrates from; the located state
                         // once the lane is INFLX_RH_REHEATED; the last state the lane held for every other stop
  INFLX_RH_CARRY_T = 7,
  INFLX_RH_CARRY_DT = 8,
  INFLX_RH_CARRY_STATUS = 9,
  INFLX_RH_CARRY_H0 = 10,  // H of the initial state
  INFLX_RH_CARRY_PLANES = 11,
};

// Argument block of inflx_rh_init and inflx_rh_advance_*.  A launch of the advance kernels takes at most `steps` accepted steps of
// every lane that still runs, skips a lane that has stopped, and adds the number of lanes still running after the launch to *running.
struct InflxRhArgs {
  const double* p;       // parameter rows of lane 0 of this pass
  uint64_t p_stride;     // doubles between the parameter rows of two lanes (0: one row for all)
  const double* init;    // (n, 4): phi^0, phi^1, chi^0, chi^1 (init kernel)
  const double* gamma;   // (n,): the decay rate of every lane
  const double* rho_r0;  // (n,): the initial radiation density (init kernel) -- or NULL: 0
  double* carry;         // [INFLX_RH_CARRY_PLANES][n]
  uint64_t n;            // lanes
  uint32_t steps;        // accepted steps this launch takes at most (at most INFLX_BG_STEPS_PER_LAUNCH)
  uint32_t reserved;
  double max_err;
  double fixed_dt;       // > 0: fixed step
  double omega_r;        // the lanes stop where rho_r / (3 H^2) reaches it
  uint32_t* running;     // one word, += the lanes still running when the launch ends
};
static_assert(sizeof(InflxRhArgs) == 96, "InflxRhArgs layout");
static_assert(offsetof(InflxRhArgs, p_stride) == 8 && offsetof(InflxRhArgs, init) == 16 && offsetof(InflxRhArgs, gamma) == 24 && offsetof(InflxRhArgs, rho_r0) == 32 &&
                  offsetof(InflxRhArgs, carry) == 40 && offsetof(InflxRhArgs, n) == 48 && offsetof(InflxRhArgs, steps) == 56 && offsetof(InflxRhArgs, max_err) == 64 &&
                  offsetof(InflxRhArgs, fixed_dt) == 72 && offsetof(InflxRhArgs, omega_r) == 80 && offsetof(InflxRhArgs, running) == 88,
              "InflxRhArgs layout");
