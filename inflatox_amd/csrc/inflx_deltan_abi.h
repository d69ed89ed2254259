// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_delta_n) and the delta-N kernels (csrc/inflx_deltan_kernels.hip): the
// kernels' argument blocks, the carry planes and the output planes.  Both sides include this header; the delta-N object exports
// INFLX_DN_ABI, and the host refuses an object whose value differs from its own.  The layout word is the delta-N object's own: the
// background, kinematics, masses, transfer, modes and tensor objects' are not involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_DN_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_DN_ABI_VERSION
#define INFLX_DN_ABI_VERSION 1
#endif

// the artefact ABI major a delta-N object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there and
// here with -DINFLX_ABI_VERSION_MAJOR, which the delta-N object is built with whenever the core object is)
#define INFLX_DN_DEFAULT_ABI_MAJOR 5

#define INFLX_DN_THREADS 256
#define INFLX_DN_OUT_PLANES 21  // csrc/inflx_deltan.h InflxDnOut: N of the 9 members, N_,I, N_,IJ, N_;IJ, |grad N|^2, f_NL, P_zeta, status

// carry planes [plane][lane] between launches; lane = member * nb + stencil (phase A: lane = stencil, the centres alone)
enum InflxDnCarry {
  INFLX_DN_CARRY_Y = 0,  // 0..5: phi^0, phi^1, chi^0, chi^1, H, N
  INFLX_DN_CARRY_T = 6,
  INFLX_DN_CARRY_DT = 7,
  INFLX_DN_CARRY_STATUS = 8,
  INFLX_DN_CARRY_RESULT = 9,  // N where the lane met its surface (NaN until it is INFLX_DN_LOCATED)
  INFLX_DN_CARRY_H0 = 10,     // the lane's initial H
  INFLX_DN_CARRY_PLANES = 11,
};

// Argument block of inflx_dn_init, inflx_dn_end_* (phase A) and inflx_dn_surface_* (phase B).  A pass holds nb stencils; `members`
// is 1 in phase A (nb lanes, every one the centre, member 4) and 9 in phase B (9 nb lanes, lane = member * nb + stencil).  Stencil b
// reads the parameter row p + b * p_stride, the centre centre[4 b .. 4 b + 3] and, with the explicit rule, the velocity
// vel[(9 b + member) * 2 ..].  A launch of the advance kernels takes at most `steps` accepted steps of every lane that still runs,
// skips a lane that has stopped, and adds the number of lanes still running after the launch to *running.  Phase A writes hc[b] when
// its lane is located (the host fills hc with NaN first); phase B reads it.
struct InflxDnArgs {
  const double* p;       // parameter rows of stencil 0 of this pass
  uint64_t p_stride;     // doubles between the parameter rows of two stencils (0: one row for all)
  const double* centre;  // (nb, 4): phi^0, phi^1, chi^0, chi^1 of the centres
  const double* vel;     // (nb, 9, 2): the members' velocities (rule INFLX_DN_EXPLICIT) -- or NULL
  double* carry;         // [INFLX_DN_CARRY_PLANES][members * nb]
  double* hc;            // (nb,): H on the surface of every stencil
  uint32_t* running;     // one word, += the lanes still running when the launch ends
  uint64_t nb;           // stencils of this pass
  uint32_t members;      // 1 (phase A) or 9 (phase B)
  uint32_t rule;         // InflxDnVelocity
  uint32_t steps;        // accepted steps this launch takes at most (at most INFLX_BG_STEPS_PER_LAUNCH)
  uint32_t reserved;
  double h0, h1;         // the stencil's steps in the two fields
  double max_err;
  double fixed_dt;       // > 0: fixed step
};
static_assert(sizeof(InflxDnArgs) == 112, "InflxDnArgs layout");
static_assert(offsetof(InflxDnArgs, p_stride) == 8 && offsetof(InflxDnArgs, centre) == 16 && offsetof(InflxDnArgs, vel) == 24 &&
                  offsetof(InflxDnArgs, carry) == 32 && offsetof(InflxDnArgs, hc) == 40 && offsetof(InflxDnArgs, running) == 48 &&
                  offsetof(InflxDnArgs, nb) == 56 && offsetof(InflxDnArgs, members) == 64 && offsetof(InflxDnArgs, rule) == 68 &&
                  offsetof(InflxDnArgs, steps) == 72 && offsetof(InflxDnArgs, h0) == 80 && offsetof(InflxDnArgs, h1) == 88 &&
                  offsetof(InflxDnArgs, max_err) == 96 && offsetof(InflxDnArgs, fixed_dt) == 104,
              "InflxDnArgs layout");

// Argument block of inflx_dn_reduce: one thread per stencil.  It reads the planes RESULT, STATUS and H0 of the phase-B carry (the
// nine members of stencil b at lanes m * nb + b: every read of a wavefront is contiguous) and writes out[plane * nb + b].
struct InflxDnReduceArgs {
  const double* p;
  uint64_t p_stride;
  const double* centre;    // (nb, 4)
  const double* carry;     // phase B: [INFLX_DN_CARRY_PLANES][9 nb]
  const double* status_a;  // (nb,): the STATUS plane of the phase-A carry -- or NULL (H_end was given)
  double* out;             // [INFLX_DN_OUT_PLANES][nb]
  uint64_t nb;
  double h0, h1;
};
static_assert(sizeof(InflxDnReduceArgs) == 72, "InflxDnReduceArgs layout");
static_assert(offsetof(InflxDnReduceArgs, centre) == 16 && offsetof(InflxDnReduceArgs, carry) == 24 && offsetof(InflxDnReduceArgs, status_a) == 32 &&
                  offsetof(InflxDnReduceArgs, out) == 40 && offsetof(InflxDnReduceArgs, nb) == 48 && offsetof(InflxDnReduceArgs, h0) == 56 &&
                  offsetof(InflxDnReduceArgs, h1) == 64,
              "InflxDnReduceArgs layout");
