// First-passage histogram kernels of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_distribution into `<artefact>.distribution`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>"
//         -DINFLX_NOISE_HEADER="<noise header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_stochastic_distribution).  It carries the core object's MODEL_TAG and a
// layout word of its own, INFLX_PD_ABI (csrc/inflx_distribution_abi.h); it is neither a kernel group nor part of any other companion
// object, and the stochastic object is not involved.
//
// L lanes per point, lane = point * L + j, L a multiple of 64: the lanes of a wavefront are realisations of one point, read one
// parameter row and one pair of bins.  Workgroups have 256 lanes and may straddle points.  A lane runs realisation after realisation
// (csrc/inflx_distribution.h inflx_pd_window): the step, the kick and the random numbers are those of the stochastic kernels
// (csrc/inflx_stochastic.h, csrc/inflx_philox.h).  A finished realisation costs one integer atomicAdd on the point's row of counts
// when it ENDED, one on the point's six status counters and one 64-bit fetch-add on the point's ticket: vector atomics at device
// scope, relaxed -- the host reads them after the stream has been synchronised.  No float atomics, so the counts do not depend on
// which lane ran which realisation.  Between launches a lane lives in the planes `carry` and `words`.
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
#include "inflx_distribution.h"

static_assert(INFLX_DIM == 2, "the distribution kernels need a two-field model");

#include "inflx_background_abi.h"  // INFLX_BG_STEPS_PER_LAUNCH
#include "inflx_distribution_abi.h"

static_assert(INFLX_PD_STATUSES == INFLX_ST_STATUSES, "csrc/inflx_stochastic.h and csrc/inflx_distribution_abi.h disagree");
static_assert(INFLX_PD_THREADS % INFLX_PD_WAVE == 0, "a workgroup is whole wavefronts");

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_PD_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxPdArgs, the carry planes and the rows of counts (csrc/inflx_distribution_abi.h)
INFLX_EXPORT uint32_t INFLX_PD_ABI = INFLX_PD_ABI_VERSION;

__device__ __forceinline__ void store_carry(double* cy, uint64_t* wd, uint64_t n, const InflxBgLane& s, const InflxPdCarry& c) {
#pragma unroll
  for (int k = 0; k < 6; ++k) cy[(uint64_t)(INFLX_PD_CARRY_Y + k) * n] = s.y[k];
  cy[(uint64_t)INFLX_PD_CARRY_T * n] = s.t;
  cy[(uint64_t)INFLX_PD_CARRY_DT * n] = s.dt;
  cy[(uint64_t)INFLX_PD_CARRY_RESULT * n] = c.n_end;
  wd[(uint64_t)INFLX_PD_WORD_STATUS * n] = (uint64_t)(uint32_t)c.status;
  wd[(uint64_t)INFLX_PD_WORD_STEPS * n] = c.steps;
  wd[(uint64_t)INFLX_PD_WORD_TICKET * n] = c.ticket;
}

// the lanes j < min(L, R) of a point start its realisations 0 .. from the point's initial state; the others are retired
extern "C" __global__ __launch_bounds__(INFLX_PD_THREADS) void inflx_pd_init(const InflxPdArgs a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_PD_THREADS + threadIdx.x, n = a.nb * a.L;
  if (lane >= n) return;
  const uint64_t b = lane / a.L, j = lane - b * a.L;
  const uint32_t first_tickets = a.R < a.L ? a.R : a.L;
  if (j == 0u) a.tickets[b] = first_tickets;
  InflxBgLane s;
  InflxPdCarry c = {__builtin_nan(""), 0u, ~UINT64_C(0), INFLX_BG_RUNNING};
  if (j < first_tickets) {
    double init[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) init[k] = a.init[b * 4u + k];
    c.ticket = j;
    c.status = inflx_st_init(s, init, a.p + b * a.p_stride, a.fixed_dt > 0.0 ? a.fixed_dt : INFLX_BG_FIRST_DT, c.n_end);
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) s.y[k] = 0.0;
    s.t = s.dt = 0.0;
  }
  store_carry(a.carry + lane, a.words + lane, n, s, c);
}

// what a finished realisation costs: the counts of its point, and the next ticket
struct PdSink {
  uint32_t* hist;    // the point's row [below, bin 0 .. bins - 1, above]
  uint32_t* counts;  // the point's six status counters
  uint64_t* ticket;
  double lo, scale;
  uint32_t bins;
  __device__ __forceinline__ void report(int status, double n_end) {
    if (status == INFLX_BG_ENDED) atomicAdd(hist + inflx_pd_slot(n_end, lo, scale, bins), 1u);
    if ((unsigned)status < (unsigned)INFLX_PD_STATUSES) atomicAdd(counts + status, 1u);
  }
  __device__ __forceinline__ uint64_t draw() { return atomicAdd(reinterpret_cast<unsigned long long*>(ticket), 1ull); }
};

// a retired lane is left as it is; every wavefront adds its lanes not retired to *a.running (n is a multiple of 64: a wavefront is
// inside the pass with all its lanes or with none)
template <int METHOD>
__device__ __forceinline__ void advance(const InflxPdArgs& a) {
  const uint64_t lane = (uint64_t)blockIdx.x * INFLX_PD_THREADS + threadIdx.x, n = a.nb * a.L;
  if (lane >= n) return;
  const uint64_t b = lane / a.L;
  double* cy = a.carry + lane;
  uint64_t* wd = a.words + lane;
  InflxPdCarry c;
  c.ticket = wd[(uint64_t)INFLX_PD_WORD_TICKET * n];
  bool live = c.ticket < a.R;
  if (live) {
    const double* p = a.p + b * a.p_stride;
    InflxBgLane s;
#pragma unroll
    for (int k = 0; k < 6; ++k) s.y[k] = cy[(uint64_t)(INFLX_PD_CARRY_Y + k) * n];
    s.t = cy[(uint64_t)INFLX_PD_CARRY_T * n];
    s.dt = cy[(uint64_t)INFLX_PD_CARRY_DT * n];
    c.n_end = cy[(uint64_t)INFLX_PD_CARRY_RESULT * n];
    c.status = (int)wd[(uint64_t)INFLX_PD_WORD_STATUS * n];
    c.steps = wd[(uint64_t)INFLX_PD_WORD_STEPS * n];
    double init[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) init[k] = a.init[b * 4u + k];
    if (c.status == INFLX_BG_RUNNING) inflx_st_resume(s, p);
    const InflxPdPoint q = {a.seed, a.first, a.R, a.max_steps, a.streams[b], a.noise_scale, a.dn_max, a.max_err, a.fixed_dt};
    PdSink sink = {a.hist + b * ((uint64_t)a.bins + 2u), a.counts + b * INFLX_PD_STATUSES, a.tickets + b, a.bin[2u * b], a.bin[2u * b + 1u], a.bins};
    live = inflx_pd_window<METHOD>(s, c, q, init, p, a.steps, sink);
    store_carry(cy, wd, n, s, c);
  }
  const unsigned long long mask = __ballot(live);
  if ((threadIdx.x & 63u) == 0u && mask != 0ull) atomicAdd(a.running, (uint32_t)__popcll(mask));
}
extern "C" __global__ __launch_bounds__(INFLX_PD_THREADS) void inflx_pd_advance_rk4(const InflxPdArgs a) { advance<INFLX_BG_RK4>(a); }
extern "C" __global__ __launch_bounds__(INFLX_PD_THREADS) void inflx_pd_advance_rkf(const InflxPdArgs a) { advance<INFLX_BG_RKF>(a); }
