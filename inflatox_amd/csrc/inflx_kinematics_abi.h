// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_kinematics) and the kinematics kernel
// (csrc/inflx_kinematics_kernels.hip): the kernel's argument block and the output planes.  Both sides include this header; the
// kinematics object exports INFLX_KIN_ABI, and the host refuses an object whose value differs from its own.  The layout word is the
// kinematics object's own: the background object's (csrc/inflx_background_abi.h) is not involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_KIN_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_KIN_ABI_VERSION
#define INFLX_KIN_ABI_VERSION 1
#endif

// the artefact ABI major a kinematics object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there
// and here with -DINFLX_ABI_VERSION_MAJOR, which the kinematics object is built with whenever the core object is)
#define INFLX_KIN_DEFAULT_ABI_MAJOR 5

#define INFLX_KIN_THREADS 256
#define INFLX_KIN_PLANES 6  // eps_H, eta_par, omega, sigma_dot, V_sigma, V_N (csrc/inflx_kinematics.h InflxKinQuantity)

// Argument block of inflx_kin_states: one lane per state.  State i of the launch is y[i * ld + c], c = 0..4 = phi^0, phi^1, chi^0,
// chi^1, H (ld = 5 for an (n, 5) array, 6 for the solver's (B, steps, 6) rows, whose sixth column is not read); it is state
// first + i of the call, whose parameter row is p + ((first + i) / traj_len) * p_stride.  Quantity q of state i goes to
// out[q * n + i]: planes, lane fastest.
struct InflxKinArgs {
  const double* y;    // states of this launch
  const double* p;    // parameter row 0 of the call
  double* out;        // [INFLX_KIN_PLANES][n]
  uint64_t n;         // states of this launch
  uint64_t ld;        // doubles between two states (>= 5)
  uint64_t traj_len;  // consecutive states of the call that share a parameter row (>= 1)
  uint64_t p_stride;  // doubles between two parameter rows (0: one row for all)
  uint64_t first;     // index in the call of state 0 of this launch
};
static_assert(sizeof(InflxKinArgs) == 64, "InflxKinArgs layout");
static_assert(offsetof(InflxKinArgs, p) == 8 && offsetof(InflxKinArgs, out) == 16 && offsetof(InflxKinArgs, n) == 24 && offsetof(InflxKinArgs, ld) == 32 &&
                  offsetof(InflxKinArgs, traj_len) == 40 && offsetof(InflxKinArgs, p_stride) == 48 && offsetof(InflxKinArgs, first) == 56,
              "InflxKinArgs layout");
