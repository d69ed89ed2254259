// Horizon-crossing kernels of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_crossing into `<artefact>.crossing`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_solve_eom_crossings, inflx_inflation_end).  It carries the core object's
// MODEL_TAG and a layout word of its own, INFLX_HX_ABI (csrc/inflx_crossing_abi.h); it is neither a kernel group nor part of any other
// companion object.
//
// One lane per trajectory, 256-lane workgroups, the six-component lane state of csrc/inflx_background.h in registers; the events are
// csrc/inflx_crossing.h.  A launch advances every running lane by at most INFLX_BG_STEPS_PER_LAUNCH accepted steps; between launches
// the state lives in `carry`, planes [INFLX_HX_CARRY_PLANES][n] (lane fastest).  Samples go to planes [sample][8][n]: y[0..5], t,
// epsilon_H -- lane fastest, so that a wavefront's store of one component is 512 contiguous bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

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
#include "inflx_crossing.h"

static_assert(INFLX_DIM == 2, "the crossing kernels need a two-field model");

#include "inflx_background_abi.h"  // INFLX_BG_STEPS_PER_LAUNCH
#include "inflx_crossing_abi.h"

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_HX_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxHxArgs, the carry planes and the sample planes (csrc/inflx_crossing_abi.h)
INFLX_EXPORT uint32_t INFLX_HX_ABI = INFLX_HX_ABI_VERSION;

// sample `k` of one lane: the located state, its time and epsilon_H there
struct CrossingSink {
  double* base;  // plane 0 of sample 0, at this lane
  uint64_t n;
  __device__ __forceinline__ void operator()(unsigned k, const InflxBgLocated& loc) const {
    double* out = base + (uint64_t)k * INFLX_HX_SAMPLE_PLANES * n;
#pragma unroll
    for (int c = 0; c < 6; ++c) out[(uint64_t)c * n] = loc.y[c];
    out[6u * n] = loc.t;
    out[7u * n] = loc.eps;
  }
};

__device__ __forceinline__ void load_lane(const double* cy, uint64_t n, InflxBgLane& s) {
#pragma unroll
  for (int c = 0; c < 6; ++c) s.y[c] = cy[(uint64_t)(INFLX_HX_CARRY_Y + c) * n];
  s.t = cy[(uint64_t)INFLX_HX_CARRY_T * n];
  s.dt = cy[(uint64_t)INFLX_HX_CARRY_DT * n];
}

__device__ __forceinline__ void store_lane(double* cy, uint64_t n, const double* y, double t, double dt, int status) {
#pragma unroll
  for (int c = 0; c < 6; ++c) cy[(uint64_t)(INFLX_HX_CARRY_Y + c) * n] = y[c];
  cy[(uint64_t)INFLX_HX_CARRY_T * n] = t;
  cy[(uint64_t)INFLX_HX_CARRY_DT * n] = dt;
  cy[(uint64_t)INFLX_HX_CARRY_STATUS * n] = (double)status;
}

// every lane's initial state; with samples, the targets before the start counted and one at the start emitted
extern "C" __global__ __launch_bounds__(INFLX_HX_THREADS) void inflx_hx_init(const InflxHxArgs a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_HX_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  const double* p = a.p + lane * a.p_stride;
  double init[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) init[c] = a.init[lane * 4u + c];
  const double dt0 = a.fixed_dt > 0.0 ? a.fixed_dt : INFLX_BG_FIRST_DT;
  InflxBgLane s;
  double n_end = __builtin_nan(""), eps = __builtin_nan("");
  unsigned cursor = 0, n_before = 0;
  double* cy = a.carry + lane;
  int st;
  if (a.samples) {
    CrossingSink sink{a.out + lane, a.n};
    st = inflx_hx_init_crossings(s, init, p, dt0, (a.flags & 1u) != 0, a.offset ? a.offset[lane] : 0.0, a.samples, a.n_samples, cursor, n_before, n_end, sink);
  } else {
    InflxBgLocated loc;
    st = inflx_hx_init_end(s, init, p, dt0, loc);
    if (st == INFLX_BG_ENDED) {
      eps = loc.eps;
      n_end = loc.y[5];
    }
  }
  store_lane(cy, a.n, s.y, s.t, s.dt, st);
  cy[(uint64_t)INFLX_HX_CARRY_NEND * a.n] = n_end;
  cy[(uint64_t)INFLX_HX_CARRY_CURSOR * a.n] = (double)cursor;
  cy[(uint64_t)INFLX_HX_CARRY_BEFORE * a.n] = (double)n_before;
  cy[(uint64_t)INFLX_HX_CARRY_EPS * a.n] = eps;
}

// A running lane with crossings: at most a.steps accepted steps, every crossing they reach stored; true while it still runs.  The
// carry holds the state the lane integrates from, never a located one.
template <int METHOD>
__device__ __forceinline__ bool advance_crossings(const InflxHxArgs& a, uint64_t lane, const double* p, double* cy) {
  InflxBgLane s;
  load_lane(cy, a.n, s);
  double n_end = cy[(uint64_t)INFLX_HX_CARRY_NEND * a.n];
  unsigned cursor = (unsigned)cy[(uint64_t)INFLX_HX_CARRY_CURSOR * a.n];
  const bool stop_at_end = (a.flags & 1u) != 0;
  const double offset = a.offset ? a.offset[lane] : 0.0;
  inflx_bg_resume(s, p);
  CrossingSink sink{a.out + lane, a.n};
  int status = INFLX_BG_RUNNING;
  for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i)
    status = inflx_hx_step_crossings<METHOD>(s, p, a.max_err, a.fixed_dt, stop_at_end, offset, a.samples, a.n_samples, cursor, n_end, sink);
  store_lane(cy, a.n, s.y, s.t, s.dt, status);
  cy[(uint64_t)INFLX_HX_CARRY_NEND * a.n] = n_end;
  cy[(uint64_t)INFLX_HX_CARRY_CURSOR * a.n] = (double)cursor;
  return status == INFLX_BG_RUNNING;
}

// A running lane that looks for the end of inflation: at most a.steps accepted steps; true while it still runs.  A lane that ends
// keeps the located end state in its carry.
template <int METHOD>
__device__ __forceinline__ bool advance_to_end(const InflxHxArgs& a, const double* p, double* cy) {
  InflxBgLane s;
  load_lane(cy, a.n, s);
  inflx_bg_resume(s, p);
  InflxBgLocated loc;
  int status = INFLX_BG_RUNNING;
  for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i) status = inflx_hx_step_end<METHOD>(s, p, a.max_err, a.fixed_dt, loc);
  const bool located = status == INFLX_BG_ENDED;
  store_lane(cy, a.n, located ? loc.y : s.y, located ? loc.t : s.t, s.dt, status);
  if (located) {
    cy[(uint64_t)INFLX_HX_CARRY_NEND * a.n] = loc.y[5];
    cy[(uint64_t)INFLX_HX_CARRY_EPS * a.n] = loc.eps;
  }
  return status == INFLX_BG_RUNNING;
}

// a lane that has stopped is left as it is; every wavefront adds its lanes that still run to *a.running (the lanes of a wavefront are
// consecutive, so its lane 0 is inside the pass whenever any of its lanes is)
template <int METHOD, bool END>
__device__ __forceinline__ void advance(const InflxHxArgs& a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_HX_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  double* cy = a.carry + lane;
  const double* p = a.p + lane * a.p_stride;
  const bool was_running = (int)cy[(uint64_t)INFLX_HX_CARRY_STATUS * a.n] == INFLX_BG_RUNNING;
  bool runs_on = false;
  if (was_running) {
    if constexpr (END)
      runs_on = advance_to_end<METHOD>(a, p, cy);
    else
      runs_on = advance_crossings<METHOD>(a, lane, p, cy);
  }
  const unsigned long long mask = __ballot(runs_on);
  if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
}
extern "C" __global__ __launch_bounds__(INFLX_HX_THREADS) void inflx_hx_advance_rk4(const InflxHxArgs a) { advance<INFLX_BG_RK4, false>(a); }
extern "C" __global__ __launch_bounds__(INFLX_HX_THREADS) void inflx_hx_advance_rkf(const InflxHxArgs a) { advance<INFLX_BG_RKF, false>(a); }
extern "C" __global__ __launch_bounds__(INFLX_HX_THREADS) void inflx_hx_end_rk4(const InflxHxArgs a) { advance<INFLX_BG_RK4, true>(a); }
extern "C" __global__ __launch_bounds__(INFLX_HX_THREADS) void inflx_hx_end_rkf(const InflxHxArgs a) { advance<INFLX_BG_RKF, true>(a); }
