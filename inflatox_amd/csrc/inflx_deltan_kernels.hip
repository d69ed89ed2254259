// Delta-N kernels of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_deltan into `<artefact>.deltan`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_delta_n).  It carries the core object's MODEL_TAG and a layout word of
// its own, INFLX_DN_ABI (csrc/inflx_deltan_abi.h); it is neither a kernel group nor part of any other companion object.
//
// One lane per stencil member, 256-lane workgroups, the six-component lane state of csrc/inflx_background.h in registers; the stepping
// and the two event searches are csrc/inflx_deltan.h.  Lane = member * nb + stencil, so every member is one contiguous plane and the
// nine values of a stencil are nine coalesced reads for inflx_dn_reduce.  A launch advances every running lane by at most
// INFLX_BG_STEPS_PER_LAUNCH accepted steps; between launches the state lives in `carry`, planes [INFLX_DN_CARRY_PLANES][lanes].
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

static_assert(INFLX_DIM == 2, "the delta-N kernels need a two-field model");

#include "inflx_background_abi.h"  // INFLX_BG_STEPS_PER_LAUNCH
#include "inflx_deltan_abi.h"

static_assert(INFLX_DN_OUT_PLANES == INFLX_DN_NOUT, "csrc/inflx_deltan.h and csrc/inflx_deltan_abi.h disagree");

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_DN_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxDnArgs, InflxDnReduceArgs, the carry planes and the output planes (csrc/inflx_deltan_abi.h)
INFLX_EXPORT uint32_t INFLX_DN_ABI = INFLX_DN_ABI_VERSION;

__device__ __forceinline__ void store_carry(double* cy, uint64_t n, const InflxBgLane& s, int status, double result) {
#pragma unroll
  for (int c = 0; c < 6; ++c) cy[(uint64_t)(INFLX_DN_CARRY_Y + c) * n] = s.y[c];
  cy[(uint64_t)INFLX_DN_CARRY_T * n] = s.t;
  cy[(uint64_t)INFLX_DN_CARRY_DT * n] = s.dt;
  cy[(uint64_t)INFLX_DN_CARRY_STATUS * n] = (double)status;
  cy[(uint64_t)INFLX_DN_CARRY_RESULT * n] = result;
}

// every lane's initial state from its centre, the offsets and the velocity rule; phase B (members = 9) knows its surface already
extern "C" __global__ __launch_bounds__(INFLX_DN_THREADS) void inflx_dn_init(const InflxDnArgs a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_DN_THREADS + threadIdx.x, n = (uint64_t)a.members * a.nb;
  if (lane >= n) return;
  const uint64_t b = lane % a.nb;
  const bool phase_a = a.members == 1u;
  const int m = phase_a ? INFLX_DN_CENTRE : (int)(lane / a.nb);
  const double* p = a.p + b * a.p_stride;
  double centre[4], init[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) centre[c] = a.centre[b * 4u + c];
  inflx_dn_member(centre, a.h0, a.h1, m, (int)a.rule, a.vel ? a.vel + (b * INFLX_DN_MEMBERS + (uint64_t)m) * 2u : nullptr, p, init);
  InflxBgLane s;
  double result = __builtin_nan("");
  const double dt0 = a.fixed_dt > 0.0 ? a.fixed_dt : INFLX_BG_FIRST_DT;
  const int st = inflx_dn_init(s, init, p, dt0, phase_a, phase_a ? __builtin_nan("") : a.hc[b], result);
  if (phase_a && st == INFLX_DN_LOCATED) a.hc[b] = s.y[4];
  double* cy = a.carry + lane;
  store_carry(cy, n, s, st, result);
  cy[(uint64_t)INFLX_DN_CARRY_H0 * n] = s.y[4];
}

// A running lane: at most a.steps accepted steps; true while it still runs
template <int METHOD, bool PHASE_A>
__device__ __forceinline__ bool advance_lane(const InflxDnArgs& a, uint64_t n, uint64_t b, const double* p, double* cy) {
  InflxBgLane s;
#pragma unroll
  for (int c = 0; c < 6; ++c) s.y[c] = cy[(uint64_t)(INFLX_DN_CARRY_Y + c) * n];
  s.t = cy[(uint64_t)INFLX_DN_CARRY_T * n];
  s.dt = cy[(uint64_t)INFLX_DN_CARRY_DT * n];
  double result = cy[(uint64_t)INFLX_DN_CARRY_RESULT * n];
  inflx_bg_resume(s, p);
  int status = INFLX_BG_RUNNING;
  if constexpr (PHASE_A) {
    double h_c = 0.0;
    for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i) status = inflx_dn_step_end<METHOD>(s, p, a.max_err, a.fixed_dt, h_c, result);
    if (status == INFLX_DN_LOCATED) a.hc[b] = h_c;
  } else {
    const double h_c = a.hc[b];
    for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i) status = inflx_dn_step_surface<METHOD>(s, p, a.max_err, a.fixed_dt, h_c, result);
  }
  store_carry(cy, n, s, status, result);
  return status == INFLX_BG_RUNNING;
}

// a lane that has stopped is left as it is; every wavefront adds its lanes that still run to *a.running (the lanes of a wavefront are
// consecutive, so its lane 0 is inside the pass whenever any of its lanes is)
template <int METHOD, bool PHASE_A>
__device__ __forceinline__ void advance(const InflxDnArgs& a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_DN_THREADS + threadIdx.x, n = (uint64_t)a.members * a.nb;
  if (lane >= n) return;
  const uint64_t b = lane % a.nb;
  double* cy = a.carry + lane;
  const bool was_running = (int)cy[(uint64_t)INFLX_DN_CARRY_STATUS * n] == INFLX_BG_RUNNING;
  bool runs_on = false;
  if (was_running) runs_on = advance_lane<METHOD, PHASE_A>(a, n, b, a.p + b * a.p_stride, cy);
  const unsigned long long mask = __ballot(runs_on);
  if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
}
extern "C" __global__ __launch_bounds__(INFLX_DN_THREADS) void inflx_dn_end_rk4(const InflxDnArgs a) { advance<INFLX_BG_RK4, true>(a); }
extern "C" __global__ __launch_bounds__(INFLX_DN_THREADS) void inflx_dn_end_rkf(const InflxDnArgs a) { advance<INFLX_BG_RKF, true>(a); }
extern "C" __global__ __launch_bounds__(INFLX_DN_THREADS) void inflx_dn_surface_rk4(const InflxDnArgs a) { advance<INFLX_BG_RK4, false>(a); }
extern "C" __global__ __launch_bounds__(INFLX_DN_THREADS) void inflx_dn_surface_rkf(const InflxDnArgs a) { advance<INFLX_BG_RKF, false>(a); }

// one thread per stencil: the nine N and statuses (plane m of the phase-B carry at lane m * nb + b), reduced by inflx_dn_reduce
extern "C" __global__ __launch_bounds__(INFLX_DN_THREADS) void inflx_dn_reduce(const InflxDnReduceArgs a) {
  const uint64_t b = (uint64_t)blockIdx.x * INFLX_DN_THREADS + threadIdx.x;
  if (b >= a.nb) return;
  const uint64_t n = (uint64_t)INFLX_DN_MEMBERS * a.nb;
  double n9[INFLX_DN_MEMBERS];
  int st9[INFLX_DN_MEMBERS];
#pragma unroll
  for (int m = 0; m < INFLX_DN_MEMBERS; ++m) {
    const uint64_t lane = (uint64_t)m * a.nb + b;
    n9[m] = a.carry[(uint64_t)INFLX_DN_CARRY_RESULT * n + lane];
    st9[m] = (int)a.carry[(uint64_t)INFLX_DN_CARRY_STATUS * n + lane];
  }
  const double h_star = a.carry[(uint64_t)INFLX_DN_CARRY_H0 * n + (uint64_t)INFLX_DN_CENTRE * a.nb + b];
  const int status_a = a.status_a ? (int)a.status_a[b] : INFLX_DN_LOCATED;
  const double x[2] = {a.centre[b * 4u], a.centre[b * 4u + 1u]};
  double out[INFLX_DN_NOUT];
  inflx_dn_reduce(n9, st9, status_a, x, a.h0, a.h1, h_star, a.p + b * a.p_stride, out);
#pragma unroll
  for (int c = 0; c < INFLX_DN_NOUT; ++c) a.out[(uint64_t)c * a.nb + b] = out[c];
}
