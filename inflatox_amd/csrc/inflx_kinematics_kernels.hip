// Trajectory-kinematics kernel of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_kinematics into `<artefact>.kinematics`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>"
//         -DINFLX_KIN_HEADER="<kinematics header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_kinematics).  It carries the core object's MODEL_TAG and a layout
// word of its own, INFLX_KIN_ABI (csrc/inflx_kinematics_abi.h); it is neither a kernel group nor part of the background object,
// whose layout it leaves alone.
//
// A post-pass over states: one lane per state, 256-lane workgroups, everything in registers (csrc/inflx_kinematics.h).
//
// The read.  Lane i reads five doubles at y + i * ld: 40 (ld = 5) or 48 (ld = 6) bytes between lanes, so one load instruction of
// a wavefront touches 20 or 24 cache lines of 128 bytes and uses 8 bytes of every 40 or 48.  The five loads of a lane are issued
// back to back and together use every byte of those lines (ld = 5) or 40 of every 48 (ld = 6: the sixth column, N, shares the
// lines and would be fetched by any scheme).  So HBM need deliver the states only once: a line that the first load brought
// in serves the other four from the CU's 32 KiB vector cache, or -- a wavefront's footprint is 2.5 or 3 KiB, and at this kernel's
// 8 wavefronts per SIMD a CU's wavefronts together can exceed the cache -- from the XCD's L2, whose bandwidth is about five times
// HBM's: even if every re-read went there (5 x 40 B per state from L2 against 88-96 B per state from and to HBM) the kernel would
// stay bound by HBM.  The price of the stride is paid in cache requests (five instructions of 20-24 lines instead of five of 4),
// not in memory bytes.  An LDS-staged tile in the manner of csrc/inflx_background_rows.h would turn those into coalesced loads at
// the cost of a barrier, 10-12 KiB of LDS per workgroup and an LDS round trip for every value (2-way bank conflicts at ld = 6: a
// 48-byte stride maps 32 lanes onto 16 bank pairs): plain per-lane loads it is, and profiles/background_kinematics.json holds the
// kernel's time beside a device-to-device copy of the same bytes.  The six stores are 512 contiguous bytes per wavefront each.
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
#include "inflx_kinematics.h"

static_assert(INFLX_DIM == 2, "the kinematics kernel needs a two-field model");

#include "inflx_kinematics_abi.h"
static_assert(INFLX_KIN_PLANES == INFLX_KIN_QUANTITIES, "one output plane per quantity of inflx_kin_eval");

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_KIN_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxKinArgs and the output planes (csrc/inflx_kinematics_abi.h)
INFLX_EXPORT uint32_t INFLX_KIN_ABI = INFLX_KIN_ABI_VERSION;

extern "C" __global__ __launch_bounds__(INFLX_KIN_THREADS) void inflx_kin_states(const InflxKinArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * INFLX_KIN_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const double* src = a.y + i * a.ld;
  double y[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) y[c] = src[c];
  // (one row for all: no 64-bit division per lane)
  const double* p = a.p_stride ? a.p + ((a.first + i) / a.traj_len) * a.p_stride : a.p;
  double out[INFLX_KIN_PLANES];
  inflx_kin_eval(y, p, out);
#pragma unroll
  for (int q = 0; q < INFLX_KIN_PLANES; ++q) a.out[(uint64_t)q * a.n + i] = out[q];
}
