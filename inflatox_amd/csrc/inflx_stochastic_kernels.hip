// Stochastic e-fold kernels of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_stochastic into `<artefact>.stochastic`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>"
//         -DINFLX_NOISE_HEADER="<noise header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_stochastic_efolds).  It carries the core object's MODEL_TAG and a layout
// word of its own, INFLX_ST_ABI (csrc/inflx_stochastic_abi.h); it is neither a kernel group nor part of any other companion object.
//
// One lane per realisation, lane = point * R + realisation, 256-lane workgroups, the six-component lane state of
// csrc/inflx_background.h in registers; the step, the kick and the random numbers are csrc/inflx_stochastic.h and csrc/inflx_philox.h.
// The lanes of a wavefront are realisations of one point: they read one parameter row and take similar numbers of trials.  A launch
// advances every running lane by at most INFLX_BG_STEPS_PER_LAUNCH accepted steps; between launches the state lives in `carry`,
// planes [INFLX_ST_CARRY_PLANES][lanes].  inflx_st_reduce then reduces the R results of every point in one workgroup: store and sum,
// no float atomics, a fixed order of additions.
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
#ifndef INFLX_NOISE_HEADER
#error "INFLX_NOISE_HEADER must name the generated noise header"
#endif
#include INFLX_NOISE_HEADER
#include "inflx_background.h"
#include "inflx_stochastic.h"

static_assert(INFLX_DIM == 2, "the stochastic kernels need a two-field model");

#include "inflx_background_abi.h"  // INFLX_BG_STEPS_PER_LAUNCH
#include "inflx_stochastic_abi.h"

static_assert(INFLX_ST_OUT_PLANES == INFLX_ST_NOUT, "csrc/inflx_stochastic.h and csrc/inflx_stochastic_abi.h disagree");
static_assert(INFLX_ST_OUT_COUNT_PLANE == INFLX_ST_OUT_COUNTS, "csrc/inflx_stochastic.h and csrc/inflx_stochastic_abi.h disagree");
static_assert(INFLX_ST_THREADS == 256, "inflx_st_reduce merges four wavefronts");

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_ST_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxStArgs, InflxStReduceArgs, the carry planes and the output planes (csrc/inflx_stochastic_abi.h)
INFLX_EXPORT uint32_t INFLX_ST_ABI = INFLX_ST_ABI_VERSION;

__device__ __forceinline__ void store_carry(double* cy, uint64_t n, const InflxBgLane& s, int status, double result) {
#pragma unroll
  for (int c = 0; c < 6; ++c) cy[(uint64_t)(INFLX_ST_CARRY_Y + c) * n] = s.y[c];
  cy[(uint64_t)INFLX_ST_CARRY_T * n] = s.t;
  cy[(uint64_t)INFLX_ST_CARRY_DT * n] = s.dt;
  cy[(uint64_t)INFLX_ST_CARRY_STATUS * n] = (double)status;
  cy[(uint64_t)INFLX_ST_CARRY_RESULT * n] = result;
}

// every lane's initial state: the R realisations of a point start from the same one
extern "C" __global__ __launch_bounds__(INFLX_ST_THREADS) void inflx_st_init(const InflxStArgs a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_ST_THREADS + threadIdx.x, n = a.nb * a.R;
  if (lane >= n) return;
  const uint64_t b = lane / a.R;
  const double* p = a.p + b * a.p_stride;
  double init[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) init[c] = a.init[b * 4u + c];
  InflxBgLane s;
  double n_end = __builtin_nan("");
  const int st = inflx_st_init(s, init, p, a.fixed_dt > 0.0 ? a.fixed_dt : INFLX_BG_FIRST_DT, n_end);
  store_carry(a.carry + lane, n, s, st, n_end);
}

// A running lane: the accepted-step indices [step_begin, step_begin + steps); true while it still runs
template <int METHOD>
__device__ __forceinline__ bool advance_lane(const InflxStArgs& a, uint64_t n, const InflxStNoise& nz, const double* p, double* cy) {
  InflxBgLane s;
#pragma unroll
  for (int c = 0; c < 6; ++c) s.y[c] = cy[(uint64_t)(INFLX_ST_CARRY_Y + c) * n];
  s.t = cy[(uint64_t)INFLX_ST_CARRY_T * n];
  s.dt = cy[(uint64_t)INFLX_ST_CARRY_DT * n];
  double n_end = cy[(uint64_t)INFLX_ST_CARRY_RESULT * n];
  inflx_st_resume(s, p);
  int status = INFLX_BG_RUNNING;
  for (uint32_t i = 0; i < a.steps && status == INFLX_BG_RUNNING; ++i)
    status = inflx_st_step<METHOD>(s, p, a.max_err, a.fixed_dt, a.dn_max, a.n_stop, nz, a.step_begin + i, n_end);
  store_carry(cy, n, s, status, n_end);
  return status == INFLX_BG_RUNNING;
}

// a lane that has stopped is left as it is; every wavefront adds its lanes that still run to *a.running (the lanes of a wavefront are
// consecutive, so its lane 0 is inside the pass whenever any of its lanes is)
template <int METHOD>
__device__ __forceinline__ void advance(const InflxStArgs& a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_ST_THREADS + threadIdx.x, n = a.nb * a.R;
  if (lane >= n) return;
  const uint64_t b = lane / a.R;
  double* cy = a.carry + lane;
  const bool was_running = (int)cy[(uint64_t)INFLX_ST_CARRY_STATUS * n] == INFLX_BG_RUNNING;
  bool runs_on = false;
  if (was_running) {
    const InflxStNoise nz = {a.seed, (uint32_t)(lane - b * a.R), a.streams[b], a.noise_scale};
    runs_on = advance_lane<METHOD>(a, n, nz, a.p + b * a.p_stride, cy);
  }
  const unsigned long long mask = __ballot(runs_on);
  if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
}
extern "C" __global__ __launch_bounds__(INFLX_ST_THREADS) void inflx_st_advance_rk4(const InflxStArgs a) { advance<INFLX_BG_RK4>(a); }
extern "C" __global__ __launch_bounds__(INFLX_ST_THREADS) void inflx_st_advance_rkf(const InflxStArgs a) { advance<INFLX_BG_RKF>(a); }

// One workgroup per point, two passes over its R results (N_end and status of lanes point * R ..: contiguous, coalesced): thread t takes
// the realisations t, t + 256, ...; the 64 partial results of a wavefront merge in a __shfl_xor butterfly (offsets 32, 16, .., 1;
// lane 0's result is used), the four wavefronts' through LDS in the order 0, 1, 2, 3.  Pass 1: count and sum of the ENDED lanes, the
// mean.  Pass 2: the central moments about it, the extremes and the lanes per status.
extern "C" __global__ __launch_bounds__(INFLX_ST_THREADS) void inflx_st_reduce(const InflxStReduceArgs a) {
  __shared__ double sums[4][3];
  __shared__ InflxStMoments parts[4];
  const uint64_t b = blockIdx.x, n = a.nb * a.R;
  if (b >= a.nb) return;  // (uniform across the workgroup)
  const double* result = a.carry + (uint64_t)INFLX_ST_CARRY_RESULT * n + b * a.R;
  const double* status = a.carry + (uint64_t)INFLX_ST_CARRY_STATUS * n + b * a.R;
  const unsigned t = threadIdx.x, wave = t >> 6;

  InflxStSum acc;
  inflx_st_sum_clear(acc);
  for (uint32_t r = t; r < a.R; r += INFLX_ST_THREADS) inflx_st_sum_add(acc, result[r], (int)status[r]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o_sum = __shfl_xor(acc.sum, off), o_comp = __shfl_xor(acc.comp, off), o_count = __shfl_xor(acc.count, off);
    inflx_st_sum_merge(acc, o_sum, o_comp, o_count);
  }
  if ((t & 63u) == 0u) {
    sums[wave][0] = acc.sum;
    sums[wave][1] = acc.comp;
    sums[wave][2] = acc.count;
  }
  __syncthreads();
  InflxStSum total = {sums[0][0], sums[0][1], sums[0][2]};
  for (int w = 1; w < 4; ++w) inflx_st_sum_merge(total, sums[w][0], sums[w][1], sums[w][2]);
  const double mean = inflx_st_sum_mean(total);  // (NaN when no lane ended: inflx_st_finish does not use it then)

  InflxStMoments m;
  inflx_st_moments_clear(m);
  for (uint32_t r = t; r < a.R; r += INFLX_ST_THREADS) inflx_st_moments_add(m, result[r], (int)status[r], mean);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    InflxStMoments o;
    o.d1 = __shfl_xor(m.d1, off);
    o.d2 = __shfl_xor(m.d2, off);
    o.d3 = __shfl_xor(m.d3, off);
    o.d4 = __shfl_xor(m.d4, off);
    o.lo = __shfl_xor(m.lo, off);
    o.hi = __shfl_xor(m.hi, off);
#pragma unroll
    for (int k = 0; k < INFLX_ST_STATUSES; ++k) o.counts[k] = __shfl_xor(m.counts[k], off);
    inflx_st_moments_merge(m, o);
  }
  if ((t & 63u) == 0u) parts[wave] = m;
  __syncthreads();
  if (t != 0u) return;
  InflxStMoments all = parts[0];
  for (int w = 1; w < 4; ++w) inflx_st_moments_merge(all, parts[w]);
  double out[INFLX_ST_NOUT];
  inflx_st_finish(mean, all, out);
#pragma unroll
  for (int c = 0; c < INFLX_ST_NOUT; ++c) a.out[(uint64_t)c * a.nb + b] = out[c];
}
