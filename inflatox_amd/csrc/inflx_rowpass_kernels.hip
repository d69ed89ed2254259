// The row pass of the row-broadcast path, gfx950 only: the per-row evaluation that feeds inflx_sweep_rowstream6 / _planes, as a
// code object of its own beside a row-only model's core object (`<artefact>.rowpass`, CompilationArtifact.ensure_rowpass; the core
// object and its content tag stay as they are).  It writes the table inflx_sweep_rowvals_* writes, bit for bit, in less time.
//
// Launched alone, the time of inflx_sweep_rowvals_* is the TABLE WRITE (64 rows x 32 replicas are 128 KiB, 16 MiB for 8192 rows),
// not the ~750-instruction chain per lane, which takes about a microsecond (profiles/rowvals_breakdown.txt): one wavefront per
// workgroup writing it takes 7 us of the kernel's 10.  Here a workgroup has 256 threads: its first wavefront evaluates the 64 rows,
// all four write, and gridDim.z workgroups -- each evaluates the same rows again, which costs nothing while CUs are idle -- share
// the rows' table region, 4 KiB pieces dealt round-robin.  The parameter rows of a single-batch sweep arrive in the kernel
// arguments (inflx_rowpass_abi.h).
//
// The model, the stages, the per-point operations and the summary come from the sweep kernels' source, none of whose entry points
// is emitted here.
#define INFLX_KERNEL_GROUPS 0u
#include "inflx_sweep_kernels.hip"

#include "inflx_rowpass_abi.h"

INFLX_EXPORT uint32_t INFLX_ROWPASS_ABI = INFLX_ROWPASS_ABI_VERSION;

// eval_row (inflx_sweep_kernels.hip) with the parameter row in `A`: the same calls in the same order
template <int OP>
__device__ __forceinline__ void rowpass_eval(const InflxSweepArgs& a, const double* A, uint64_t row, double* o) {
  double U[kNU], R[kNR], C[kNC];
  inflx_stage_uniform(A, U);
  const double x0 = inflx_coord(a.row_begin + row, a.dx0, a.x0a);
  inflx_stage_row(x0, A, U, R);
  InflxModelValues mv;
  inflx_stage_point(x0, a.x1a, A, U, R, C, mv);
  fill_v01<OP>(mv, x0, a.x1a, A);
  apply_op<OP>(mv, o, a.accuracy);
}

// Constant indices and a uniform select per row, so that the argument array stays in SGPRs.
__device__ __forceinline__ void rowpass_params(const InflxRowPassArgs& ra, unsigned p, double* A) {
  if (ra.a.params) return load_params(ra.a.params, p, A);
  constexpr int kInlineRows = INFLX_INLINE_PARAMS / kNP;
#pragma unroll
  for (int k = 0; k < kNP; ++k) A[k] = 0.0;
#pragma unroll
  for (int q = 0; q < kInlineRows; ++q) {
#pragma unroll
    for (int k = 0; k < INFLX_N_PARAMETERS; ++k) A[k] = p == (unsigned)q ? ra.params_inline[q * INFLX_N_PARAMETERS + k] : A[k];
  }
}

template <int OP, bool STATS = false>
__device__ __forceinline__ void rowpass(const InflxRowPassArgs& ra) {
  const InflxSweepArgs& a = ra.a;
  __shared__ __attribute__((aligned(16))) double vals[kWave][8];
  const unsigned tid = threadIdx.x;
  const uint64_t row0 = (uint64_t)blockIdx.x * kWave;
  const unsigned p = blockIdx.y;
  if (tid < kWave) {  // (wavefront-uniform)
    double o[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    if (row0 + tid < a.row_count) {
      double A[kNP];
      rowpass_params(ra, p, A);
      rowpass_eval<OP>(a, A, row0 + tid, o);
    }
    if constexpr (STATS) {
      // every point of the row has these six values: the row counts N1 times (in one write slice only)
      if (blockIdx.z == 0) {
        StatAcc acc;
        stat_init(acc);
        if (row0 + tid < a.row_count) stat_add(acc, o, a.N1);
        stat_flush(acc, a.stats);
      }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) vals[tid][k] = o[k];
  }
  if constexpr (STATS) {
    if (a.row_table == nullptr) return;  // summary-only sweep: nothing to broadcast
  }
  __syncthreads();
  // the 64 rows' table entries ([row][replica][8 doubles], replicas a power of two) are one contiguous region: coalesced 16-byte stores
  const uint64_t left = a.row_count - row0;
  const unsigned nrows = left < (uint64_t)kWave ? (unsigned)left : (unsigned)kWave;
  const unsigned shift = 31 - __builtin_clz(a.table_replicas * 4);  // log2(units per row)
  const unsigned units = nrows << shift;
  inflx_d2* dst = reinterpret_cast<inflx_d2*>(a.row_table + ((uint64_t)p * a.row_count + row0) * a.table_replicas * 8);
  for (unsigned q = blockIdx.z * blockDim.x + tid; q < units; q += gridDim.z * blockDim.x) {
    const unsigned r = q >> shift, part = q & 3;
    dst[q] = *reinterpret_cast<const inflx_d2*>(&vals[r][2 * part]);
  }
}

#define INFLX_DEFINE_ROWPASS(NAME, OP)                                                                      \
  extern "C" __global__ __launch_bounds__(kThreads) void inflx_rowpass_##NAME(const InflxRowPassArgs ra) { \
    if constexpr ((INFLX_OUT_MASK & 2) == 0) rowpass<OP>(ra);                                             \
  }
INFLX_DEFINE_ROWPASS(complete, INFLX_OP_COMPLETE)
INFLX_DEFINE_ROWPASS(consistency, INFLX_OP_CONSISTENCY)
INFLX_DEFINE_ROWPASS(rapidturn, INFLX_OP_RAPIDTURN)
INFLX_DEFINE_ROWPASS(epsilon_v, INFLX_OP_EPSILON_V)
INFLX_DEFINE_ROWPASS(raw, INFLX_OP_RAW)
INFLX_DEFINE_ROWPASS(hesse, INFLX_OP_HESSE)
extern "C" __global__ __launch_bounds__(kThreads) void inflx_rowpass_complete_stats(const InflxRowPassArgs ra) {
  if constexpr ((INFLX_OUT_MASK & 2) == 0) rowpass<INFLX_OP_COMPLETE, true>(ra);
}
