// Reheating kernels of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_reheating into `<artefact>.reheating`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_reheating).  It carries the core object's MODEL_TAG and a layout word of
// its own, INFLX_RH_ABI (csrc/inflx_reheating_abi.h); it is neither a kernel group nor part of any other companion object.
//
// One lane per trajectory, 256-lane workgroups, the seven-component lane state of csrc/inflx_reheating.h in registers.  A launch
// advances every running lane by at most INFLX_BG_STEPS_PER_LAUNCH accepted steps; between launches the state lives in `carry`,
// planes [INFLX_RH_CARRY_PLANES][n] (lane fastest, so that a wavefront's access to one plane is 512 contiguous bytes).
#include <hip/hip_runtime.h>
#include <stdint.h>

// No contraction of a*b+c into FMAs anywhere in this object, whatever -ffp-contract the core object's options name: a lane resolves
// thousands of oscillations of the fields, and a located state next to a zero of an oscillating velocity carries the rounding of all
// of them.  Without contraction the lanes take the host build's arithmetic (tests/reheating_twin.cpp, -ffp-contract=off) operation
// for operation -- 5e-14 of a value's scale after 3055 steps, against 1.3e-11 with contraction -- so that the host build is a
// reference for the device at any length of run.  (The fma calls that the generated model code spells out stay: the host has them too.)
#pragma clang fp contract(off)

#include "inflx_device_math.h"
#include "inflx_kernel_abi.h"
#include "inflx_ops.h"

#ifndef INFLX_MODEL_HEADER
#error "INFLX_MODEL_HEADER must name the generated model header"
#endif
#include INFLX_MODEL_HEADER
#ifndef INFLX_EOM_HEADER
#error "INFLX_EOM_HEADER must name the generated equations-of-motion header"
#endif
#include INFLX_EOM_HEADER
#include "inflx_background.h"
#include "inflx_deltan.h"
#include "inflx_reheating.h"

static_assert(INFLX_DIM == 2, "the reheating kernels need a two-field model");

#include "inflx_background_abi.h"  // INFLX_BG_STEPS_PER_LAUNCH
#include "inflx_reheating_abi.h"

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_RH_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxRhArgs and the carry planes (csrc/inflx_reheating_abi.h)
INFLX_EXPORT uint32_t INFLX_RH_ABI = INFLX_RH_ABI_VERSION;

__device__ __forceinline__ void store_lane(double* cy, uint64_t n, const double* y, double t, double dt, int status) {
#pragma unroll
  for (int c = 0; c < INFLX_RH_COMPONENTS; ++c) cy[(uint64_t)(INFLX_RH_CARRY_Y + c) * n] = y[c];
  cy[(uint64_t)INFLX_RH_CARRY_T * n] = t;
  cy[(uint64_t)INFLX_RH_CARRY_DT * n] = dt;
  cy[(uint64_t)INFLX_RH_CARRY_STATUS * n] = (double)status;
}

// every lane's initial state and its H_0; a lane whose radiation already dominates stops here
extern "C" __global__ __launch_bounds__(INFLX_RH_THREADS) void inflx_rh_init(const InflxRhArgs a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_RH_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  const double* p = a.p + lane * a.p_stride;
  double init[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) init[c] = a.init[lane * 4u + c];
  const double dt0 = a.fixed_dt > 0.0 ? a.fixed_dt : INFLX_BG_FIRST_DT;
  InflxRhLane s;
  InflxRhLocated loc;
  const int st = inflx_rh_init(s, init, a.gamma[lane], a.rho_r0 ? a.rho_r0[lane] : 0.0, p, dt0, a.omega_r, loc);
  double* cy = a.carry + lane;
  store_lane(cy, a.n, s.y, s.t, s.dt, st);  // (a lane reheated at the start: the located state is the initial state)
  cy[(uint64_t)INFLX_RH_CARRY_H0 * a.n] = s.y[4];
}

// A running lane: at most a.steps accepted steps; true while it still runs.  A lane that reheats keeps the located state in its
// carry, every other lane the state it holds.
template <int METHOD>
__device__ __forceinline__ bool advance_lane(const InflxRhArgs& a, uint64_t lane, const double* p, double* cy) {
  InflxRhLane s;
#pragma unroll
  for (int c = 0; c < INFLX_RH_COMPONENTS; ++c) s.y[c] = cy[(uint64_t)(INFLX_RH_CARRY_Y + c) * a.n];
  s.t = cy[(uint64_t)INFLX_RH_CARRY_T * a.n];
  s.dt = cy[(uint64_t)INFLX_RH_CARRY_DT * a.n];
  s.gamma = a.gamma[lane];
  inflx_rh_resume(s, p);
  InflxRhLocated loc;
  int status = INFLX_BG_RUNNING;
  for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i) status = inflx_rh_step<METHOD>(s, p, a.max_err, a.fixed_dt, a.omega_r, loc);
  const bool located = status == INFLX_RH_REHEATED;
  store_lane(cy, a.n, located ? loc.y : s.y, located ? loc.t : s.t, s.dt, status);
  return status == INFLX_BG_RUNNING;
}

// a lane that has stopped is left as it is; every wavefront adds its lanes that still run to *a.running (the lanes of a wavefront are
// consecutive, so its lane 0 is inside the pass whenever any of its lanes is)
template <int METHOD>
__device__ __forceinline__ void advance(const InflxRhArgs& a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_RH_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  double* cy = a.carry + lane;
  const double* p = a.p + lane * a.p_stride;
  const bool was_running = (int)cy[(uint64_t)INFLX_RH_CARRY_STATUS * a.n] == INFLX_BG_RUNNING;
  bool runs_on = false;
  if (was_running) runs_on = advance_lane<METHOD>(a, lane, p, cy);
  const unsigned long long mask = __ballot(runs_on);
  if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
}
extern "C" __global__ __launch_bounds__(INFLX_RH_THREADS) void inflx_rh_advance_rk4(const InflxRhArgs a) { advance<INFLX_BG_RK4>(a); }
extern "C" __global__ __launch_bounds__(INFLX_RH_THREADS) void inflx_rh_advance_rkf(const InflxRhArgs a) { advance<INFLX_BG_RKF>(a); }
