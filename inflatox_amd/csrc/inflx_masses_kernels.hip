// Entropic-mass kernel of one inflation model, gfx950 (MI355X / CDNA4) only.
//
// Built on first use by inflatox_amd.CompilationArtifact.ensure_masses into `<artefact>.masses`:
//   hipcc <the core object's options> -DINFLX_MODEL_HEADER="<core header>" -DINFLX_EOM_HEADER="<eom header>"
//         -DINFLX_KIN_HEADER="<kinematics header>" -DINFLX_MASS_HEADER="<masses header>" this_file
// and loaded by libinflx_hip.so beside the core object (inflx_masses).  It carries the core object's MODEL_TAG and a layout word
// of its own, INFLX_MASS_ABI (csrc/inflx_masses_abi.h); it is neither a kernel group nor part of the background or the kinematics
// object, whose layouts it leaves alone.
//
// A post-pass over states: one lane per state, 256-lane workgroups, everything in registers (csrc/inflx_masses.h).
//
// The read is inflx_kin_states' (csrc/inflx_kinematics_kernels.hip), for the same reasons.  Lane i reads five doubles at y + i * ld:
// 40 (ld = 5) or 48 (ld = 6) bytes between lanes, so one load instruction of a wavefront touches 20 or 24 cache lines of 128 bytes.
// The five loads of a lane are issued back to back and together use every byte of those lines (ld = 5) or 40 of every 48 (ld = 6),
// so HBM need deliver the states only once; the re-reads of a line are served by the CU's vector cache or by L2.  The stride is paid
// in cache requests, not in memory bytes, and this kernel has more arithmetic per state than the kinematics kernel (the Hesse
// matrix, the connection and the curvature) to hide them behind and two more planes to write (104-112 B per state from and to HBM
// against 88-96 B), so an LDS-staged tile -- a barrier, 10-12 KiB of LDS per workgroup, an LDS round trip per value -- has even less
// to offer here than there: plain per-lane loads, no LDS.  The eight stores are 512 contiguous bytes per wavefront each.
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
#include "inflx_masses.h"

static_assert(INFLX_DIM == 2, "the masses kernel needs a two-field model");

#include "inflx_masses_abi.h"
static_assert(INFLX_MASS_PLANES == INFLX_MASS_QUANTITIES, "one output plane per quantity of inflx_mass_eval");

#define INFLX_EXPORT extern "C" __device__ __attribute__((used, visibility("default")))
#ifndef INFLX_ABI_VERSION_MAJOR
#define INFLX_ABI_VERSION_MAJOR INFLX_MASS_DEFAULT_ABI_MAJOR
#endif
INFLX_EXPORT uint16_t VERSION[3] = {INFLX_ABI_VERSION_MAJOR, 0, 0};
// which model this is: the content tag of the core object it belongs to
#ifndef INFLX_MODEL_TAG
#define INFLX_MODEL_TAG ""
#endif
INFLX_EXPORT char MODEL_TAG[] = INFLX_MODEL_TAG;
// layout version of InflxMassArgs and the output planes (csrc/inflx_masses_abi.h)
INFLX_EXPORT uint32_t INFLX_MASS_ABI = INFLX_MASS_ABI_VERSION;

extern "C" __global__ __launch_bounds__(INFLX_MASS_THREADS) void inflx_mass_states(const InflxMassArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * INFLX_MASS_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const double* src = a.y + i * a.ld;
  double y[5];
#pragma unroll
  for (int c = 0; c < 5; ++c) y[c] = src[c];
  // (one row for all: no 64-bit division per lane)
  const double* p = a.p_stride ? a.p + ((a.first + i) / a.traj_len) * a.p_stride : a.p;
  double out[INFLX_MASS_PLANES];
  inflx_mass_eval(y, p, out);
#pragma unroll
  for (int q = 0; q < INFLX_MASS_PLANES; ++q) a.out[(uint64_t)q * a.n + i] = out[q];
}
