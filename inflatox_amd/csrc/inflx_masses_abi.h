// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_masses) and the masses kernel (csrc/inflx_masses_kernels.hip): the
// kernel's argument block and the output planes.  Both sides include this header; the masses object exports INFLX_MASS_ABI, and the
// host refuses an object whose value differs from its own.  The layout word is the masses object's own: the background object's
// (csrc/inflx_background_abi.h) and the kinematics object's (csrc/inflx_kinematics_abi.h) are not involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_MASS_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_MASS_ABI_VERSION
#define INFLX_MASS_ABI_VERSION 1
#endif

// the artefact ABI major a masses object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there
// and here with -DINFLX_ABI_VERSION_MAJOR, which the masses object is built with whenever the core object is)
#define INFLX_MASS_DEFAULT_ABI_MAJOR 5

#define INFLX_MASS_THREADS 256
#define INFLX_MASS_PLANES 8  // V_TT, V_TN, V_NN, ricci, eps_H, omega, M_eff2, mu_s2 (csrc/inflx_masses.h InflxMassQuantity)

// Argument block of inflx_mass_states, with the fields and the meaning of InflxKinArgs: one lane per state.  State i of the launch
// is y[i * ld + c], c = 0..4 = phi^0, phi^1, chi^0, chi^1, H (ld = 5 for an (n, 5) array, 6 for the solver's (B, steps, 6) rows,
// whose sixth column is not read); it is state first + i of the call, whose parameter row is p + ((first + i) / traj_len) *
// p_stride.  Quantity q of state i goes to out[q * n + i]: planes, lane fastest.
struct InflxMassArgs {
  const double* y;    // states of this launch
  const double* p;    // parameter row 0 of the call
  double* out;        // [INFLX_MASS_PLANES][n]
  uint64_t n;         // states of this launch
  uint64_t ld;        // doubles between two states (>= 5)
  uint64_t traj_len;  // consecutive states of the call that share a parameter row (>= 1)
  uint64_t p_stride;  // doubles between two parameter rows (0: one row for all)
  uint64_t first;     // index in the call of state 0 of this launch
};
static_assert(sizeof(InflxMassArgs) == 64, "InflxMassArgs layout");
static_assert(offsetof(InflxMassArgs, p) == 8 && offsetof(InflxMassArgs, out) == 16 && offsetof(InflxMassArgs, n) == 24 && offsetof(InflxMassArgs, ld) == 32 &&
                  offsetof(InflxMassArgs, traj_len) == 40 && offsetof(InflxMassArgs, p_stride) == 48 && offsetof(InflxMassArgs, first) == 56,
              "InflxMassArgs layout");
