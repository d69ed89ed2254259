// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_stochastic_efolds) and the stochastic kernels
// (csrc/inflx_stochastic_kernels.hip): the kernels' argument blocks, the carry planes and the output planes.  Both sides include this
// header; the stochastic object exports INFLX_ST_ABI, and the host refuses an object whose value differs from its own.  The layout word
// is the stochastic object's own: no other companion object's is involved.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_ST_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_ST_ABI_VERSION
#define INFLX_ST_ABI_VERSION 1
#endif

// the artefact ABI major a stochastic object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there
// and here with -DINFLX_ABI_VERSION_MAJOR, which the stochastic object is built with whenever the core object is)
#define INFLX_ST_DEFAULT_ABI_MAJOR 5

#define INFLX_ST_THREADS 256
#define INFLX_ST_OUT_PLANES 12     // csrc/inflx_stochastic.h InflxStOut: mean, m2, m3, m4, min, max, lanes per status 0..5
#define INFLX_ST_OUT_COUNT_PLANE 6  // the first of the six planes of lanes per status: InflxStOut's INFLX_ST_OUT_COUNTS
#define INFLX_ST_SAMPLE_PLANES 7   // N, phi^0, phi^1, chi^0, chi^1, H, status of every lane
#define INFLX_ST_MAX_REALISATIONS (1u << 20)

// carry planes [plane][lane] between launches, laid out like the delta-N object's; lane = point * R + realisation
enum InflxStCarry {
  INFLX_ST_CARRY_Y = 0,  // 0..5: phi^0, phi^1, chi^0, chi^1, H, N
  INFLX_ST_CARRY_T = 6,
  INFLX_ST_CARRY_DT = 7,
  INFLX_ST_CARRY_STATUS = 8,
  INFLX_ST_CARRY_RESULT = 9,  // N_end of a lane that is INFLX_BG_ENDED (NaN until then)
  INFLX_ST_CARRY_PLANES = 10,
};

// Argument block of inflx_st_init and inflx_st_advance_*.  A pass holds nb points of R realisations, lane = point * R + realisation:
// the lanes of a wavefront are realisations of one point (or of neighbours).  Point b reads the parameter row p + b * p_stride, the
// initial state init[4 b .. 4 b + 3] and its stream id streams[b].  A launch of the advance kernels processes the accepted-step
// indices [step_begin, step_begin + steps) of every lane that still runs -- the index is the Philox counter of the step's kick --,
// skips a lane that has stopped, and adds the number of lanes still running after the launch to *running.
struct InflxStArgs {
  const double* p;          // parameter rows of point 0 of this pass
  uint64_t p_stride;        // doubles between the parameter rows of two points (0: one row for all)
  const double* init;       // (nb, 4): phi^0, phi^1, chi^0, chi^1
  const uint32_t* streams;  // (nb,): the points' stream ids
  double* carry;            // [INFLX_ST_CARRY_PLANES][nb * R]
  uint32_t* running;        // one word, += the lanes still running when the launch ends
  uint64_t nb;              // points of this pass
  uint64_t seed;            // the Philox key
  uint64_t step_begin;      // first accepted-step index of this launch
  uint32_t R;               // realisations per point, at most INFLX_ST_MAX_REALISATIONS
  uint32_t steps;           // accepted-step indices this launch processes (at most INFLX_BG_STEPS_PER_LAUNCH)
  double noise_scale;
  double dn_max;            // adaptive runs: no step is tried that is longer than dn_max / H
  double n_stop;            // stop at this e-fold count (INFLX_BG_TARGET) -- or NaN
  double max_err;
  double fixed_dt;          // > 0: fixed step
};
static_assert(sizeof(InflxStArgs) == 120, "InflxStArgs layout");
static_assert(offsetof(InflxStArgs, p_stride) == 8 && offsetof(InflxStArgs, init) == 16 && offsetof(InflxStArgs, streams) == 24 &&
                  offsetof(InflxStArgs, carry) == 32 && offsetof(InflxStArgs, running) == 40 && offsetof(InflxStArgs, nb) == 48 &&
                  offsetof(InflxStArgs, seed) == 56 && offsetof(InflxStArgs, step_begin) == 64 && offsetof(InflxStArgs, R) == 72 &&
                  offsetof(InflxStArgs, steps) == 76 && offsetof(InflxStArgs, noise_scale) == 80 && offsetof(InflxStArgs, dn_max) == 88 &&
                  offsetof(InflxStArgs, n_stop) == 96 && offsetof(InflxStArgs, max_err) == 104 && offsetof(InflxStArgs, fixed_dt) == 112,
              "InflxStArgs layout");

// Argument block of inflx_st_reduce: one workgroup per point.  It reads the planes RESULT and STATUS of the point's R lanes (lanes
// point * R .. point * R + R - 1: contiguous) and writes out[plane * nb + point].
struct InflxStReduceArgs {
  const double* carry;  // [INFLX_ST_CARRY_PLANES][nb * R]
  double* out;          // [INFLX_ST_OUT_PLANES][nb]
  uint64_t nb;
  uint32_t R;
  uint32_t reserved;
};
static_assert(sizeof(InflxStReduceArgs) == 32, "InflxStReduceArgs layout");
static_assert(offsetof(InflxStReduceArgs, out) == 8 && offsetof(InflxStReduceArgs, nb) == 16 && offsetof(InflxStReduceArgs, R) == 24, "InflxStReduceArgs layout");
