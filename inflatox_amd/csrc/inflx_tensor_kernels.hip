// Tensor-mode kernels of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_tensor into `<artefact>.tensor`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_mode_spectra with INFLX_MODES_TENSOR).  It carries the core object's
// MODEL_TAG and a layout word of its own, INFLX_TN_ABI (csrc/inflx_tensor_abi.h); it is neither a kernel group nor part of any other
// companion object.
//
// One lane per (trajectory, wavenumber), 256-lane workgroups, the 10-component lane state of csrc/inflx_tensor.h with the right-hand
// side inlined (DESIGN.md section 12 has the register figures).  A launch advances every running lane by at most
// INFLX_BG_STEPS_PER_LAUNCH accepted steps; between launches the state lives in `carry`, planes [INFLX_TN_CARRY_PLANES][n] (lane
// fastest).  A lane emits its outputs once, in the step that stops it, into planes [8][n] -- lane fastest, so that a wavefront's
// store of one plane is 512 contiguous bytes.  Lanes stop in different steps, so such a store is usually partial; the host pre-fills
// the planes with NaN and nothing else is ever written.
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
#include "inflx_tensor.h"

static_assert(INFLX_DIM == 2, "the tensor-mode kernels need a two-field model");

#include "inflx_background_abi.h"  // INFLX_BG_STEPS_PER_LAUNCH
#include "inflx_tensor_abi.h"

static_assert(INFLX_TN_OUT_PLANES == INFLX_TN_NOUT && INFLX_TN_CARRY_T == INFLX_TN_NC, "csrc/inflx_tensor.h and csrc/inflx_tensor_abi.h disagree");

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_TN_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxTnArgs, the carry planes and the output planes (csrc/inflx_tensor_abi.h)
INFLX_EXPORT uint32_t INFLX_TN_ABI = INFLX_TN_ABI_VERSION;

// the outputs of one lane
struct TensorSink {
  double* base;  // plane 0, at this lane
  uint64_t n;
  __device__ __forceinline__ void operator()(const double* o) const {
#pragma unroll
    for (int c = 0; c < INFLX_TN_OUT_PLANES; ++c) base[(uint64_t)c * n] = o[c];
  }
};

__device__ __forceinline__ void store_carry(double* cy, uint64_t n, const InflxTnLane& s, double n_end, int status) {
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) cy[(uint64_t)(INFLX_TN_CARRY_Y + c) * n] = s.y[c];
  cy[(uint64_t)INFLX_TN_CARRY_T * n] = s.t;
  cy[(uint64_t)INFLX_TN_CARRY_DT * n] = s.dt;
  cy[(uint64_t)INFLX_TN_CARRY_NEND * n] = n_end;
  cy[(uint64_t)INFLX_TN_CARRY_STATUS * n] = (double)status;
}

extern "C" __global__ __launch_bounds__(INFLX_TN_THREADS) void inflx_tn_init(const InflxTnArgs a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_TN_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  const double* p = a.p + lane * a.p_stride;
  double init[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) init[c] = a.init[lane * 4u + c];
  InflxTnLane s;
  double n_end = __builtin_nan("");
  const double dt0 = a.fixed_dt > 0.0 ? a.fixed_dt : INFLX_BG_FIRST_DT;
  TensorSink sink{a.out + lane, a.n};
  const int st = inflx_tn_init(s, init, p, dt0, (a.flags & 1u) != 0, a.kappa[lane], a.n_target[lane], n_end, sink);
  store_carry(a.carry + lane, a.n, s, n_end, st);
}

// A running lane: at most a.steps accepted steps; true while it still runs.  The carry holds the state the lane integrates from
// (never a located one).
template <int METHOD>
__device__ __forceinline__ bool advance_lane(const InflxTnArgs& a, uint64_t lane, const double* p, double* cy) {
  InflxTnLane s;
#pragma unroll
  for (int c = 0; c < INFLX_TN_NC; ++c) s.y[c] = cy[(uint64_t)(INFLX_TN_CARRY_Y + c) * a.n];
  s.t = cy[(uint64_t)INFLX_TN_CARRY_T * a.n];
  s.dt = cy[(uint64_t)INFLX_TN_CARRY_DT * a.n];
  s.kappa = a.kappa[lane];
  double n_end = cy[(uint64_t)INFLX_TN_CARRY_NEND * a.n];
  const double n_target = a.n_target[lane];
  const bool stop_at_end = (a.flags & 1u) != 0;
  inflx_tn_resume(s, p);
  TensorSink sink{a.out + lane, a.n};
  int status = INFLX_BG_RUNNING;
  for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i) status = inflx_tn_step<METHOD>(s, p, a.max_err, a.fixed_dt, stop_at_end, n_target, n_end, sink);
  store_carry(cy, a.n, s, n_end, status);
  return status == INFLX_BG_RUNNING;
}

// a lane that has stopped is left as it is; every wavefront adds its lanes that still run to *a.running (the lanes of a wavefront are
// consecutive, so its lane 0 is inside the batch whenever any of its lanes is)
template <int METHOD>
__device__ __forceinline__ void advance(const InflxTnArgs& a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_TN_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  double* cy = a.carry + lane;
  const bool was_running = (int)cy[(uint64_t)INFLX_TN_CARRY_STATUS * a.n] == INFLX_BG_RUNNING;
  bool runs_on = false;
  if (was_running) runs_on = advance_lane<METHOD>(a, lane, a.p + lane * a.p_stride, cy);
  const unsigned long long mask = __ballot(runs_on);
  if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
}
extern "C" __global__ __launch_bounds__(INFLX_TN_THREADS) void inflx_tn_advance_rk4(const InflxTnArgs a) { advance<INFLX_BG_RK4>(a); }
extern "C" __global__ __launch_bounds__(INFLX_TN_THREADS) void inflx_tn_advance_rkf(const InflxTnArgs a) { advance<INFLX_BG_RKF>(a); }
