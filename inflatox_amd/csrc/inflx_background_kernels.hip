// Background-trajectory kernels of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_background into `<artefact>.background`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_solve_eom).  It carries the core object's MODEL_TAG; it is not a
// kernel group (INFLX_GROUPS / inflx_groups do not see it).
//
// One lane per trajectory, 256-lane workgroups, the whole integrator state in registers (csrc/inflx_background.h).  A launch advances
// every lane by at most INFLX_BG_STEPS_PER_LAUNCH accepted steps, whatever the number of steps per row; between launches the state
// lives in `carry`, planes [INFLX_BG_CARRY_PLANES][n] (lane fastest, csrc/inflx_background_abi.h).
// Rows go to `rows`, planes [row][7][n]: y[0..5], t -- lane fastest, so that a wavefront's store of one component is 512 contiguous
// bytes.  STORE_ROWS = false is the final-only mode (e-fold maps): nothing but the carry is written.  TARGET = true (final-only)
// adds a per-lane target on N: a lane stops at the state where N = target, located inside the accepted step that passes it
// (inflx_bg_step_target), and that state -- with epsilon_H there -- is what its carry holds.  The *_sampled kernels (final-only)
// emit the state at every point of a list of e-fold counts or times shared by all lanes (inflx_bg_step_sampled) into planes
// [sample][8][n]: y[0..5], t, epsilon_H.
// inflx_bg_rows_transpose, which knows nothing of the model, copies a window of row planes into the trajectory-major arrays
// inflx_solve_eom hands out (csrc/inflx_background_rows.h); it lives here because this is the object inflx_solve_eom loads.
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

static_assert(INFLX_DIM == 2, "the background kernels need a two-field model");

#include "inflx_background_abi.h"
#include "inflx_background_rows.h"

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_BG_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxBgArgs and the carry / row planes (csrc/inflx_background_abi.h)
INFLX_EXPORT uint32_t INFLX_BG_ABI = INFLX_BG_ABI_VERSION;

constexpr int kBgThreads = 256;

__device__ __forceinline__ void store_row(double* rows, uint64_t n, uint32_t slot, uint64_t lane, const double* y, double t, bool valid) {
  double* base = rows + (uint64_t)slot * 7u * n + lane;
  const double nan = __builtin_nan("");
#pragma unroll
  for (int c = 0; c < 6; ++c) base[(uint64_t)c * n] = valid ? y[c] : nan;
  base[6u * n] = valid ? t : nan;
}

// sample `k` of one lane: the located state, its time and epsilon_H there
struct SampleSink {
  double* base;  // plane 0 of sample 0, at this lane
  uint64_t n;
  __device__ __forceinline__ void operator()(unsigned k, const InflxBgLocated& loc) const {
    double* out = base + (uint64_t)k * 8u * n;
#pragma unroll
    for (int c = 0; c < 6; ++c) out[(uint64_t)c * n] = loc.y[c];
    out[6u * n] = loc.t;
    out[7u * n] = loc.eps;
  }
};

extern "C" __global__ __launch_bounds__(kBgThreads) void inflx_bg_init(const InflxBgArgs a) {
  const uint64_t lane = (uint64_t)blockIdx.x * kBgThreads + threadIdx.x;
  if (lane >= a.n) return;
  const double* p = a.p + lane * a.p_stride;
  double init[4];
  for (int c = 0; c < 4; ++c) init[c] = a.init[lane * 4u + c];
  InflxBgLane s;
  double n_end = __builtin_nan("");
  const double dt0 = a.fixed_dt > 0.0 ? a.fixed_dt : INFLX_BG_FIRST_DT;
  InflxBgLocated loc;
  loc.eps = __builtin_nan("");
  unsigned cursor = 0;  // (lanes with samples: the samples emitted)
  int st;
  if (a.samples) {
    SampleSink sink{a.rows + lane, a.n};
    st = inflx_bg_init_sampled(s, init, p, dt0, (a.flags & 1u) != 0, a.samples, a.n_samples, cursor, n_end, sink);
  } else {
    st = a.target ? inflx_bg_init_target(s, init, p, dt0, (a.flags & 1u) != 0, a.target[lane], n_end, loc)
                  : inflx_bg_init(s, init, p, dt0, (a.flags & 1u) != 0, n_end);
  }
  double* cy = a.carry + lane;
  for (int c = 0; c < 6; ++c) cy[(uint64_t)(INFLX_BG_CARRY_Y + c) * a.n] = s.y[c];
  cy[(uint64_t)INFLX_BG_CARRY_EPS * a.n] = loc.eps;
  cy[(uint64_t)INFLX_BG_CARRY_T * a.n] = s.t;
  cy[(uint64_t)INFLX_BG_CARRY_DT * a.n] = s.dt;
  cy[(uint64_t)INFLX_BG_CARRY_NEND * a.n] = n_end;
  cy[(uint64_t)INFLX_BG_CARRY_STATUS * a.n] = (double)st;
  cy[(uint64_t)INFLX_BG_CARRY_LAST_ROW * a.n] = (double)cursor;
  cy[(uint64_t)INFLX_BG_CARRY_PENDING * a.n] = 0.0;
  if (a.rows && !a.samples) store_row(a.rows, a.n, 0, lane, s.y, s.t, true);  // row 0 (slot 0) is the initial state
}

// A running lane with a target on N: at most a.steps accepted steps; true while it still runs.  A lane that stops keeps in its
// carry the state it stopped at -- the located state and epsilon_H there for INFLX_BG_TARGET.
template <int METHOD>
__device__ __forceinline__ bool advance_to_target(const InflxBgArgs& a, uint64_t lane, const double* p, double* cy) {
  InflxBgLane s;
  for (int c = 0; c < 6; ++c) s.y[c] = cy[(uint64_t)(INFLX_BG_CARRY_Y + c) * a.n];
  s.t = cy[(uint64_t)INFLX_BG_CARRY_T * a.n];
  s.dt = cy[(uint64_t)INFLX_BG_CARRY_DT * a.n];
  double n_end = cy[(uint64_t)INFLX_BG_CARRY_NEND * a.n];
  const double target = a.target[lane];
  const bool stop_at_end = (a.flags & 1u) != 0;
  inflx_bg_resume(s, p);
  InflxBgLocated loc;
  int status = INFLX_BG_RUNNING;
  for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i)
    status = inflx_bg_step_target<METHOD>(s, p, a.max_err, a.fixed_dt, stop_at_end, target, n_end, loc);
  const bool located = status == INFLX_BG_TARGET;
  for (int c = 0; c < 6; ++c) cy[(uint64_t)(INFLX_BG_CARRY_Y + c) * a.n] = located ? loc.y[c] : s.y[c];
  cy[(uint64_t)INFLX_BG_CARRY_T * a.n] = located ? loc.t : s.t;
  cy[(uint64_t)INFLX_BG_CARRY_DT * a.n] = s.dt;
  cy[(uint64_t)INFLX_BG_CARRY_NEND * a.n] = n_end;
  cy[(uint64_t)INFLX_BG_CARRY_STATUS * a.n] = (double)status;
  if (located) cy[(uint64_t)INFLX_BG_CARRY_EPS * a.n] = loc.eps;
  return status == INFLX_BG_RUNNING;
}

// A running lane with samples: at most a.steps accepted steps, every sample they pass stored; true while it still runs.  The carry
// holds the state the lane integrates from (never a located one) and, in plane LAST_ROW, the number of samples emitted.
template <int METHOD>
__device__ __forceinline__ bool advance_sampled(const InflxBgArgs& a, uint64_t lane, const double* p, double* cy) {
  InflxBgLane s;
  for (int c = 0; c < 6; ++c) s.y[c] = cy[(uint64_t)(INFLX_BG_CARRY_Y + c) * a.n];
  s.t = cy[(uint64_t)INFLX_BG_CARRY_T * a.n];
  s.dt = cy[(uint64_t)INFLX_BG_CARRY_DT * a.n];
  double n_end = cy[(uint64_t)INFLX_BG_CARRY_NEND * a.n];
  unsigned cursor = (unsigned)cy[(uint64_t)INFLX_BG_CARRY_LAST_ROW * a.n];
  const bool stop_at_end = (a.flags & 1u) != 0, sample_t = (a.flags & 2u) != 0;
  inflx_bg_resume(s, p);
  SampleSink sink{a.rows + lane, a.n};
  int status = INFLX_BG_RUNNING;
  for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i)
    status = inflx_bg_step_sampled<METHOD>(s, p, a.max_err, a.fixed_dt, stop_at_end, a.samples, a.n_samples, sample_t, cursor, n_end, sink);
  for (int c = 0; c < 6; ++c) cy[(uint64_t)(INFLX_BG_CARRY_Y + c) * a.n] = s.y[c];
  cy[(uint64_t)INFLX_BG_CARRY_T * a.n] = s.t;
  cy[(uint64_t)INFLX_BG_CARRY_DT * a.n] = s.dt;
  cy[(uint64_t)INFLX_BG_CARRY_NEND * a.n] = n_end;
  cy[(uint64_t)INFLX_BG_CARRY_STATUS * a.n] = (double)status;
  cy[(uint64_t)INFLX_BG_CARRY_LAST_ROW * a.n] = (double)cursor;
  return status == INFLX_BG_RUNNING;
}

// The accepted-step indices [step_begin, step_begin + steps) of one lane.  A running lane takes one accepted step per index; at
// the end of every row (index r*substeps - 1) row r is written: the state, or NaN once the lane has stopped -- except the row in
// which a lane ends at epsilon_H = 1, which holds the end state.  A row may span launches: nothing but the step index says where
// in a row a launch starts, and that index is the same for every lane.
// TARGET: a lane that has stopped is left as it is, and every wavefront adds its lanes that still run to *a.running (the lanes of
// a wavefront are consecutive, so its lane 0 is inside the batch whenever any of its lanes is).
template <int METHOD, bool STORE_ROWS, bool TARGET>
__device__ __forceinline__ void advance(const InflxBgArgs& a) {
  static_assert(!(TARGET && STORE_ROWS), "a target on N is a final-only mode");
  const uint64_t lane = (uint64_t)blockIdx.x * kBgThreads + threadIdx.x;
  if (lane >= a.n) return;
  const double* p = a.p + lane * a.p_stride;
  double* cy = a.carry + lane;
  if constexpr (TARGET) {
    const bool was_running = (int)cy[(uint64_t)INFLX_BG_CARRY_STATUS * a.n] == INFLX_BG_RUNNING;
    bool runs_on = false;
    if (was_running) runs_on = advance_to_target<METHOD>(a, lane, p, cy);
    const unsigned long long mask = __ballot(runs_on);
    if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
    return;
  }
  InflxBgLane s;
  for (int c = 0; c < 6; ++c) s.y[c] = cy[(uint64_t)(INFLX_BG_CARRY_Y + c) * a.n];
  s.t = cy[(uint64_t)INFLX_BG_CARRY_T * a.n];
  s.dt = cy[(uint64_t)INFLX_BG_CARRY_DT * a.n];
  double n_end = cy[(uint64_t)INFLX_BG_CARRY_NEND * a.n];
  int status = (int)cy[(uint64_t)INFLX_BG_CARRY_STATUS * a.n];
  double last_row = cy[(uint64_t)INFLX_BG_CARRY_LAST_ROW * a.n];
  bool pending = cy[(uint64_t)INFLX_BG_CARRY_PENDING * a.n] != 0.0;
  if (status == INFLX_BG_RUNNING) inflx_bg_resume(s, p);
  const bool stop_at_end = (a.flags & 1u) != 0;
  uint32_t k = (uint32_t)(a.step_begin % a.substeps);  // steps of the current row already taken
  uint64_t row = a.step_begin / a.substeps;             // the last complete row
  for (uint32_t i = 0; i < a.steps; ++i) {
    if (status == INFLX_BG_RUNNING) {
      status = inflx_bg_step<METHOD>(s, p, a.max_err, a.fixed_dt, stop_at_end, n_end);
      pending = status == INFLX_BG_ENDED;
    }
    if (++k == a.substeps) {
      k = 0;
      ++row;
      const bool valid = status == INFLX_BG_RUNNING || pending;
      if (valid) last_row = (double)row;
      if constexpr (STORE_ROWS) store_row(a.rows, a.n, (uint32_t)(row - a.row_base), lane, s.y, s.t, valid);
      pending = false;
    }
    if (!STORE_ROWS && status != INFLX_BG_RUNNING && !pending) break;
  }
  for (int c = 0; c < 6; ++c) cy[(uint64_t)(INFLX_BG_CARRY_Y + c) * a.n] = s.y[c];
  cy[(uint64_t)INFLX_BG_CARRY_T * a.n] = s.t;
  cy[(uint64_t)INFLX_BG_CARRY_DT * a.n] = s.dt;
  cy[(uint64_t)INFLX_BG_CARRY_NEND * a.n] = n_end;
  cy[(uint64_t)INFLX_BG_CARRY_STATUS * a.n] = (double)status;
  cy[(uint64_t)INFLX_BG_CARRY_LAST_ROW * a.n] = last_row;
  cy[(uint64_t)INFLX_BG_CARRY_PENDING * a.n] = pending ? 1.0 : 0.0;
}

#define INFLX_BG_KERNEL(name, METHOD, STORE, TARGET) \
  extern "C" __global__ __launch_bounds__(kBgThreads) void name(const InflxBgArgs a) { advance<METHOD, STORE, TARGET>(a); }
INFLX_BG_KERNEL(inflx_bg_advance_rk4_rows, INFLX_BG_RK4, true, false)
INFLX_BG_KERNEL(inflx_bg_advance_rk4_final, INFLX_BG_RK4, false, false)
INFLX_BG_KERNEL(inflx_bg_advance_rkf_rows, INFLX_BG_RKF, true, false)
INFLX_BG_KERNEL(inflx_bg_advance_rkf_final, INFLX_BG_RKF, false, false)
INFLX_BG_KERNEL(inflx_bg_advance_rk4_target, INFLX_BG_RK4, false, true)
INFLX_BG_KERNEL(inflx_bg_advance_rkf_target, INFLX_BG_RKF, false, true)

// *_sampled: a lane that has stopped is left as it is; every wavefront adds its lanes that still run to *a.running
template <int METHOD>
__device__ __forceinline__ void advance_samples(const InflxBgArgs& a) {
  const uint64_t lane = (uint64_t)blockIdx.x * kBgThreads + threadIdx.x;
  if (lane >= a.n) return;
  double* cy = a.carry + lane;
  const bool was_running = (int)cy[(uint64_t)INFLX_BG_CARRY_STATUS * a.n] == INFLX_BG_RUNNING;
  bool runs_on = false;
  if (was_running) runs_on = advance_sampled<METHOD>(a, lane, a.p + lane * a.p_stride, cy);
  const unsigned long long mask = __ballot(runs_on);
  if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
}
extern "C" __global__ __launch_bounds__(kBgThreads) void inflx_bg_advance_rk4_sampled(const InflxBgArgs a) { advance_samples<INFLX_BG_RK4>(a); }
extern "C" __global__ __launch_bounds__(kBgThreads) void inflx_bg_advance_rkf_sampled(const InflxBgArgs a) { advance_samples<INFLX_BG_RKF>(a); }

// One tile of 64 lanes x 8 slots per workgroup, through LDS: planes [slot][7][n] -> out_y (lanes, rows_total, 6), out_t (lanes,
// rows_total).  Grid: inflx_bg_rows_blocks(n, filled) workgroups.  Both phases: csrc/inflx_background_rows.h.
extern "C" __global__ __launch_bounds__(INFLX_BG_ROWS_THREADS) void inflx_bg_rows_transpose(const InflxBgRowsArgs a) {
  __shared__ double tile[INFLX_BG_ROWS_TILE_DOUBLES];
  inflx_bg_rows_load(a, blockIdx.x, threadIdx.x, tile);
  __syncthreads();
  inflx_bg_rows_store(a, blockIdx.x, threadIdx.x, tile);
}
