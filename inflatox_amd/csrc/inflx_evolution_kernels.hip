// Evolution kernels of one inflation model -- the spectra of a mode sampled along its evolution --, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_evolution into `<artefact>.evolution`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>"
//         -DINFLX_KIN_HEADER="<kinematics header>" -DINFLX_MASS_HEADER="<masses header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_mode_evolution).  It carries the core object's MODEL_TAG and a layout
// word of its own, INFLX_EV_ABI (csrc/inflx_evolution_abi.h); it is neither a kernel group nor part of any other companion object,
// and the modes object is not needed.
//
// The kernels of csrc/inflx_modes_kernels.hip with csrc/inflx_evolution.h's init and step in place of csrc/inflx_modes.h's: one lane
// per (trajectory, wavenumber), 256-lane workgroups, the 22-component lane state, the stage arrays handed to the out-of-line
// right-hand side in scratch (DESIGN.md section 12 has the figures).  A launch advances every running lane by at most
// INFLX_BG_STEPS_PER_LAUNCH accepted steps; between launches the state and the sample cursor live in `carry`, planes
// [INFLX_EV_CARRY_PLANES][n] (lane fastest).  A lane emits its final values once, in the step that stops it, into planes [22][n], and
// sample k from the step that passes it into planes sampled[k][6][n] -- lane fastest both, so that a wavefront's store of one plane is
// 512 contiguous bytes.  Lanes pass a sample in different steps, so such a store is usually partial; the host pre-fills both outputs
// with NaN and nothing else is ever written.
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
#ifndef INFLX_KIN_HEADER
#error "INFLX_KIN_HEADER must name the generated kinematics header"
#endif
#include INFLX_KIN_HEADER
#ifndef INFLX_MASS_HEADER
#error "INFLX_MASS_HEADER must name the generated masses header"
#endif
#include INFLX_MASS_HEADER
#include "inflx_background.h"
#include "inflx_modes.h"
#include "inflx_evolution.h"

static_assert(INFLX_DIM == 2, "the evolution kernels need a two-field model");

#include "inflx_background_abi.h"  // INFLX_BG_STEPS_PER_LAUNCH
#include "inflx_evolution_abi.h"

static_assert(INFLX_EV_OUT_PLANES == INFLX_MD_NOUT && INFLX_EV_CARRY_T == INFLX_MD_NC && INFLX_EV_SAMPLE_PLANES == INFLX_EV_NSAMPLE,
              "csrc/inflx_modes.h, csrc/inflx_evolution.h and csrc/inflx_evolution_abi.h disagree");

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_EV_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxEvArgs, the carry planes and the output planes (csrc/inflx_evolution_abi.h)
INFLX_EXPORT uint32_t INFLX_EV_ABI = INFLX_EV_ABI_VERSION;

// the outputs of one lane: the final values, and the samples (k < n_samples: the cursor of csrc/inflx_evolution.h)
struct EvolutionSink {
  double* base;     // plane 0 of the final values, at this lane
  double* sampled;  // plane 0 of sample 0, at this lane
  uint64_t n;
  __device__ __forceinline__ void operator()(const double* o) const {
#pragma unroll
    for (int c = 0; c < INFLX_EV_OUT_PLANES; ++c) base[(uint64_t)c * n] = o[c];
  }
  __device__ __forceinline__ void sample(unsigned k, const double* o) const {
    double* at = sampled + (uint64_t)k * INFLX_EV_SAMPLE_PLANES * n;
#pragma unroll
    for (int c = 0; c < INFLX_EV_SAMPLE_PLANES; ++c) at[(uint64_t)c * n] = o[INFLX_EV_SAMPLE_OF(c)];
  }
};

__device__ __forceinline__ void store_carry(double* cy, uint64_t n, const InflxMdLane& s, double n_end, int status, unsigned cursor) {
#pragma unroll
  for (int c = 0; c < INFLX_MD_NC; ++c) cy[(uint64_t)(INFLX_EV_CARRY_Y + c) * n] = s.y[c];
  cy[(uint64_t)INFLX_EV_CARRY_T * n] = s.t;
  cy[(uint64_t)INFLX_EV_CARRY_DT * n] = s.dt;
  cy[(uint64_t)INFLX_EV_CARRY_NEND * n] = n_end;
  cy[(uint64_t)INFLX_EV_CARRY_STATUS * n] = (double)status;
  cy[(uint64_t)INFLX_EV_CARRY_CURSOR * n] = (double)cursor;
}

extern "C" __global__ __launch_bounds__(INFLX_EV_THREADS) void inflx_ev_init(const InflxEvArgs a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_EV_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  const double* p = a.p + lane * a.p_stride;
  double init[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) init[c] = a.init[lane * 4u + c];
  InflxMdLane s;
  double n_end = __builtin_nan("");
  unsigned cursor = 0;
  const double dt0 = a.fixed_dt > 0.0 ? a.fixed_dt : INFLX_BG_FIRST_DT;
  EvolutionSink sink{a.out + lane, a.sampled + lane, a.n};
  const int st = inflx_ev_init(s, init, p, dt0, (a.flags & 1u) != 0, a.kappa[lane], a.n_target[lane], a.samples, a.n_samples, a.shift[lane], cursor, n_end, sink);
  store_carry(a.carry + lane, a.n, s, n_end, st, cursor);
}

// A running lane: at most a.steps accepted steps; true while it still runs.  The carry holds the state the lane integrates from
// (never a located one) and the cursor, which is at most a.n_samples: inflx_ev_init and inflx_ev_step alone write it.
template <int METHOD>
__device__ __forceinline__ bool advance_lane(const InflxEvArgs& a, uint64_t lane, const double* p, double* cy) {
  InflxMdLane s;
#pragma unroll
  for (int c = 0; c < INFLX_MD_NC; ++c) s.y[c] = cy[(uint64_t)(INFLX_EV_CARRY_Y + c) * a.n];
  s.t = cy[(uint64_t)INFLX_EV_CARRY_T * a.n];
  s.dt = cy[(uint64_t)INFLX_EV_CARRY_DT * a.n];
  s.kappa = a.kappa[lane];
  double n_end = cy[(uint64_t)INFLX_EV_CARRY_NEND * a.n];
  unsigned cursor = (unsigned)cy[(uint64_t)INFLX_EV_CARRY_CURSOR * a.n];
  const double n_target = a.n_target[lane], shift = a.shift[lane];
  const bool stop_at_end = (a.flags & 1u) != 0;
  inflx_md_resume(s, p);
  EvolutionSink sink{a.out + lane, a.sampled + lane, a.n};
  int status = INFLX_BG_RUNNING;
  for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i)
    status = inflx_ev_step<METHOD>(s, p, a.max_err, a.fixed_dt, stop_at_end, n_target, a.samples, a.n_samples, shift, cursor, n_end, sink);
  store_carry(cy, a.n, s, n_end, status, cursor);
  return status == INFLX_BG_RUNNING;
}

// a lane that has stopped is left as it is; every wavefront adds its lanes that still run to *a.running (the lanes of a wavefront are
// consecutive, so its lane 0 is inside the batch whenever any of its lanes is)
template <int METHOD>
__device__ __forceinline__ void advance(const InflxEvArgs& a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_EV_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  double* cy = a.carry + lane;
  const bool was_running = (int)cy[(uint64_t)INFLX_EV_CARRY_STATUS * a.n] == INFLX_BG_RUNNING;
  bool runs_on = false;
  if (was_running) runs_on = advance_lane<METHOD>(a, lane, a.p + lane * a.p_stride, cy);
  const unsigned long long mask = __ballot(runs_on);
  if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
}
extern "C" __global__ __launch_bounds__(INFLX_EV_THREADS) void inflx_ev_advance_rk4(const InflxEvArgs a) { advance<INFLX_BG_RK4>(a); }
extern "C" __global__ __launch_bounds__(INFLX_EV_THREADS) void inflx_ev_advance_rkf(const InflxEvArgs a) { advance<INFLX_BG_RKF>(a); }
