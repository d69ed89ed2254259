// Transfer-function kernels of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_transfer into `<artefact>.transfer`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>"
//         -DINFLX_KIN_HEADER="<kinematics header>" -DINFLX_MASS_HEADER="<masses header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_transfer_functions).  It carries the core object's MODEL_TAG and a
// layout word of its own, INFLX_TR_ABI (csrc/inflx_transfer_abi.h); it is neither a kernel group nor part of the background, the
// kinematics or the masses object, whose layouts it leaves alone.
//
// One lane per trajectory, 256-lane workgroups, the nine-component lane state in registers (csrc/inflx_transfer.h); the stage arrays
// handed to the out-of-line right-hand side live in scratch, 672 to 712 bytes per lane whatever the model.  A
// launch advances every running lane by at most INFLX_BG_STEPS_PER_LAUNCH accepted steps; between launches the state lives in `carry`,
// planes [INFLX_TR_CARRY_PLANES][n] (lane fastest).  A lane emits a sample into planes [sample][10][n]: y[0..5], t, epsilon_H, T_SS,
// T_RS -- lane fastest, so that a wavefront's store of one component of one sample is 512 contiguous bytes.  Lanes reach a sample in
// different steps, so such a store is usually partial; the host pre-fills the planes with NaN and nothing else is ever written.
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
#include "inflx_transfer.h"

static_assert(INFLX_DIM == 2, "the transfer kernels need a two-field model");

#include "inflx_background_abi.h"  // INFLX_BG_STEPS_PER_LAUNCH
#include "inflx_transfer_abi.h"

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_TR_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxTrArgs, the carry planes and the output planes (csrc/inflx_transfer_abi.h)
INFLX_EXPORT uint32_t INFLX_TR_ABI = INFLX_TR_ABI_VERSION;

// sample `k` of one lane
struct TransferSink {
  double* base;  // plane 0 of sample 0, at this lane
  uint64_t n;
  __device__ __forceinline__ void operator()(unsigned k, const InflxTrSample& smp) const {
    double* out = base + (uint64_t)k * INFLX_TR_OUT_PLANES * n;
#pragma unroll
    for (int c = 0; c < 6; ++c) out[(uint64_t)c * n] = smp.loc.y[c];
    out[6u * n] = smp.loc.t;
    out[7u * n] = smp.loc.eps;
    out[8u * n] = smp.t_ss;
    out[9u * n] = smp.t_rs;
  }
};

__device__ __forceinline__ void store_carry(double* cy, uint64_t n, const InflxTrLane& s, double n_end, int status, unsigned cursor, const double* ends) {
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) cy[(uint64_t)(INFLX_TR_CARRY_Y + c) * n] = s.y[c];
  cy[(uint64_t)INFLX_TR_CARRY_T * n] = s.t;
  cy[(uint64_t)INFLX_TR_CARRY_DT * n] = s.dt;
  cy[(uint64_t)INFLX_TR_CARRY_NEND * n] = n_end;
  cy[(uint64_t)INFLX_TR_CARRY_STATUS * n] = (double)status;
  cy[(uint64_t)INFLX_TR_CARRY_CURSOR * n] = (double)cursor;
  cy[(uint64_t)INFLX_TR_CARRY_END_SS * n] = ends[0];
  cy[(uint64_t)INFLX_TR_CARRY_END_RS * n] = ends[1];
}

extern "C" __global__ __launch_bounds__(INFLX_TR_THREADS) void inflx_tr_init(const InflxTrArgs a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_TR_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  const double* p = a.p + lane * a.p_stride;
  double init[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) init[c] = a.init[lane * 4u + c];
  InflxTrLane s;
  double n_end = __builtin_nan("");
  double ends[2] = {__builtin_nan(""), __builtin_nan("")};
  const double dt0 = a.fixed_dt > 0.0 ? a.fixed_dt : INFLX_BG_FIRST_DT;
  unsigned cursor = 0;
  TransferSink sink{a.out + lane, a.n};
  const int st = inflx_tr_init(s, init, p, dt0, (a.flags & 1u) != 0, a.dq_dn != nullptr, a.dq_dn ? a.dq_dn[lane] : 0.0, a.samples, a.n_samples, cursor, n_end,
                               ends, sink);
  double* cy = a.carry + lane;
  store_carry(cy, a.n, s, n_end, st, cursor, ends);
  cy[(uint64_t)INFLX_TR_CARRY_EPS_STAR * a.n] = s.eps_star;
}

// A running lane: at most a.steps accepted steps, every sample they pass stored; true while it still runs.  The carry holds the
// state the lane integrates from (never a located one).
template <int METHOD>
__device__ __forceinline__ bool advance_lane(const InflxTrArgs& a, uint64_t lane, const double* p, double* cy) {
  InflxTrLane s;
#pragma unroll
  for (int c = 0; c < INFLX_TR_NC; ++c) s.y[c] = cy[(uint64_t)(INFLX_TR_CARRY_Y + c) * a.n];
  s.t = cy[(uint64_t)INFLX_TR_CARRY_T * a.n];
  s.dt = cy[(uint64_t)INFLX_TR_CARRY_DT * a.n];
  s.eps_star = cy[(uint64_t)INFLX_TR_CARRY_EPS_STAR * a.n];
  double n_end = cy[(uint64_t)INFLX_TR_CARRY_NEND * a.n];
  double ends[2] = {cy[(uint64_t)INFLX_TR_CARRY_END_SS * a.n], cy[(uint64_t)INFLX_TR_CARRY_END_RS * a.n]};
  unsigned cursor = (unsigned)cy[(uint64_t)INFLX_TR_CARRY_CURSOR * a.n];
  const bool stop_at_end = (a.flags & 1u) != 0;
  inflx_tr_resume(s, p);
  TransferSink sink{a.out + lane, a.n};
  int status = INFLX_BG_RUNNING;
  for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i)
    status = inflx_tr_step_sampled<METHOD>(s, p, a.max_err, a.fixed_dt, stop_at_end, a.samples, a.n_samples, cursor, n_end, ends, sink);
  store_carry(cy, a.n, s, n_end, status, cursor, ends);
  return status == INFLX_BG_RUNNING;
}

// a lane that has stopped is left as it is; every wavefront adds its lanes that still run to *a.running (the lanes of a wavefront are
// consecutive, so its lane 0 is inside the batch whenever any of its lanes is)
template <int METHOD>
__device__ __forceinline__ void advance(const InflxTrArgs& a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_TR_THREADS + threadIdx.x;
  if (lane >= a.n) return;
  double* cy = a.carry + lane;
  const bool was_running = (int)cy[(uint64_t)INFLX_TR_CARRY_STATUS * a.n] == INFLX_BG_RUNNING;
  bool runs_on = false;
  if (was_running) runs_on = advance_lane<METHOD>(a, lane, a.p + lane * a.p_stride, cy);
  const unsigned long long mask = __ballot(runs_on);
  if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
}
extern "C" __global__ __launch_bounds__(INFLX_TR_THREADS) void inflx_tr_advance_rk4(const InflxTrArgs a) { advance<INFLX_BG_RK4>(a); }
extern "C" __global__ __launch_bounds__(INFLX_TR_THREADS) void inflx_tr_advance_rkf(const InflxTrArgs a) { advance<INFLX_BG_RKF>(a); }
