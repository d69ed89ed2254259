// Rows of the background solver in the caller's layout: the two phases of inflx_bg_rows_transpose (csrc/inflx_background_kernels.hip)
// and the plan of a call's lane passes (csrc/inflx_hip.cpp).  Plain C++ without a HIP header: the kernel, the host library and the
// CPU program tests/background_rows_twin.cpp, which runs every thread of every block through both phases, all include this file.
//
// The advance kernels write rows lane fastest, planes [slot][7][n] (a wavefront's store of one component is 512 contiguous bytes);
// inflx_solve_eom promises states (B, rows, 6) and t (B, rows).  A workgroup of 256 threads moves one tile of 64 lanes x 8 slots
// through LDS so that both sides are contiguous:
//   load   wavefront w takes the segments w, w + 4, ... of the tile's 8 x 7 (slot, component) segments; a segment is the component of
//          64 consecutive lanes, 512 contiguous bytes of the planes.  Lane l puts y[c] of slot r at tile[l * 49 + r * 6 + c] and t at
//          tile[64 * 49 + l * 9 + r].
//   store  a lane's 8 rows x 6 components are 48 consecutive doubles of out_y (384 B): thread e of the tile's 64 x 48 elements
//          (e = 256 k + thread) writes element e % 48 of lane e / 48, so consecutive threads write consecutive doubles; likewise the
//          64 x 8 elements of out_t.
// The pitches 49 and 9 are odd on purpose.  The LDS banks a 64-bit store over 32 dword banks in groups of 16 consecutive lanes: with
// a pitch of P doubles lane l starts at dword 2 P l, and for odd P the 16 lanes of a group cover the 32 banks once (even P: 2-way at
// best, P = 48: 16-way).  It banks a 64-bit load over 64 dword banks in halves of 32 lanes: thread e reads double e + e / 48, so the
// 32 threads of a half read 32 doubles out of 33 consecutive ones -- the 64 banks once, or one bank twice where a lane ends.
// A ragged tile (n % 64 lanes, filled % 8 slots) masks lanes and slots in both phases; LDS that load did not write is not read.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "inflx_background_abi.h"

#if defined(__HIPCC__)
#define INFLX_BG_ROWS_FN __host__ __device__ __forceinline__
#else
#define INFLX_BG_ROWS_FN inline
#endif

#define INFLX_BG_ROWS_THREADS 256u
#define INFLX_BG_ROWS_TILE_LANES 64u
#define INFLX_BG_ROWS_TILE_ROWS 8u
#define INFLX_BG_ROWS_PITCH_Y 49u  // doubles per lane: 8 rows x 6 components, + 1
#define INFLX_BG_ROWS_PITCH_T 9u   // doubles per lane: 8 rows, + 1
#define INFLX_BG_ROWS_TILE_DOUBLES (INFLX_BG_ROWS_TILE_LANES * (INFLX_BG_ROWS_PITCH_Y + INFLX_BG_ROWS_PITCH_T))  // 29 696 bytes

// workgroups of one launch: lane tiles x row tiles, lane tiles fastest (a one-dimensional grid)
INFLX_BG_ROWS_FN uint64_t inflx_bg_rows_blocks(uint64_t n, uint64_t filled) {
  return ((n + INFLX_BG_ROWS_TILE_LANES - 1) / INFLX_BG_ROWS_TILE_LANES) * ((filled + INFLX_BG_ROWS_TILE_ROWS - 1) / INFLX_BG_ROWS_TILE_ROWS);
}

// the tile of workgroup `block`: its first lane and slot, and how many of its lanes and slots lie inside the window
struct InflxBgRowsTile {
  uint64_t lane0, slot0;
  unsigned lanes, slots;
};
INFLX_BG_ROWS_FN InflxBgRowsTile inflx_bg_rows_tile(const InflxBgRowsArgs& a, uint64_t block) {
  const uint64_t lane_tiles = (a.n + INFLX_BG_ROWS_TILE_LANES - 1) / INFLX_BG_ROWS_TILE_LANES;
  InflxBgRowsTile t;
  t.lane0 = (block % lane_tiles) * INFLX_BG_ROWS_TILE_LANES;
  t.slot0 = (block / lane_tiles) * INFLX_BG_ROWS_TILE_ROWS;
  const uint64_t lanes = a.n - t.lane0, slots = t.slot0 < a.filled ? a.filled - t.slot0 : 0;
  t.lanes = lanes < INFLX_BG_ROWS_TILE_LANES ? (unsigned)lanes : INFLX_BG_ROWS_TILE_LANES;
  t.slots = slots < INFLX_BG_ROWS_TILE_ROWS ? (unsigned)slots : INFLX_BG_ROWS_TILE_ROWS;
  return t;
}

// phase 1 of thread `thread` of workgroup `block`: planes -> tile
INFLX_BG_ROWS_FN void inflx_bg_rows_load(const InflxBgRowsArgs& a, uint64_t block, unsigned thread, double* tile) {
  const InflxBgRowsTile t = inflx_bg_rows_tile(a, block);
  const unsigned l = thread % INFLX_BG_ROWS_TILE_LANES, w = thread / INFLX_BG_ROWS_TILE_LANES;
  if (l >= t.lanes) return;
  const double* src = a.rows + t.slot0 * 7u * a.n + t.lane0 + l;
  constexpr unsigned kWaves = INFLX_BG_ROWS_THREADS / INFLX_BG_ROWS_TILE_LANES, kSegments = INFLX_BG_ROWS_TILE_ROWS * 7u;
  static_assert(kSegments % kWaves == 0, "every wavefront takes the same number of segments");
  // (all loads first, so that they are in flight together; then the tile)
  double v[kSegments / kWaves];
#pragma unroll
  for (unsigned k = 0; k < kSegments / kWaves; ++k) {
    const unsigned seg = w + k * kWaves;
    v[k] = seg / 7u < t.slots ? src[(uint64_t)seg * a.n] : 0.0;
  }
#pragma unroll
  for (unsigned k = 0; k < kSegments / kWaves; ++k) {
    const unsigned seg = w + k * kWaves, r = seg / 7u, c = seg % 7u;
    if (r >= t.slots) continue;
    if (c < 6u)
      tile[l * INFLX_BG_ROWS_PITCH_Y + r * 6u + c] = v[k];
    else
      tile[INFLX_BG_ROWS_TILE_LANES * INFLX_BG_ROWS_PITCH_Y + l * INFLX_BG_ROWS_PITCH_T + r] = v[k];
  }
}

// phase 2, after every thread of the workgroup has finished phase 1: tile -> out_y, out_t
INFLX_BG_ROWS_FN void inflx_bg_rows_store(const InflxBgRowsArgs& a, uint64_t block, unsigned thread, const double* tile) {
  const InflxBgRowsTile t = inflx_bg_rows_tile(a, block);
  const uint64_t row0 = a.row_base + t.slot0, traj0 = a.lane_off + t.lane0;
  if (a.out_y) {
    constexpr unsigned kRun = INFLX_BG_ROWS_TILE_ROWS * 6u;
    static_assert(INFLX_BG_ROWS_TILE_LANES * kRun % INFLX_BG_ROWS_THREADS == 0, "every thread takes the same number of elements");
#pragma unroll
    for (unsigned k = 0; k < INFLX_BG_ROWS_TILE_LANES * kRun / INFLX_BG_ROWS_THREADS; ++k) {
      const unsigned e = k * INFLX_BG_ROWS_THREADS + thread, l = e / kRun, j = e % kRun;
      if (l < t.lanes && j < t.slots * 6u) a.out_y[((traj0 + l) * a.rows_total + row0) * 6u + j] = tile[l * INFLX_BG_ROWS_PITCH_Y + j];
    }
  }
  if (a.out_t) {
    static_assert(INFLX_BG_ROWS_TILE_LANES * INFLX_BG_ROWS_TILE_ROWS % INFLX_BG_ROWS_THREADS == 0, "every thread takes the same number of elements");
#pragma unroll
    for (unsigned k = 0; k < INFLX_BG_ROWS_TILE_LANES * INFLX_BG_ROWS_TILE_ROWS / INFLX_BG_ROWS_THREADS; ++k) {
      const unsigned e = k * INFLX_BG_ROWS_THREADS + thread, l = e / INFLX_BG_ROWS_TILE_ROWS, r = e % INFLX_BG_ROWS_TILE_ROWS;
      if (l < t.lanes && r < t.slots)
        a.out_t[(traj0 + l) * a.rows_total + row0 + r] = tile[INFLX_BG_ROWS_TILE_LANES * INFLX_BG_ROWS_PITCH_Y + l * INFLX_BG_ROWS_PITCH_T + r];
    }
  }
}

// ---- the passes of one call (host) -------------------------------------------------------------------------------------------
// bounds of one call's passes: lanes per chunk, bytes of the device row buffer (the steps of one launch: INFLX_BG_STEPS_PER_LAUNCH)
constexpr size_t kBgMaxLanes = size_t(1) << 20;
constexpr size_t kBgRowBytes = size_t(256) << 20;
// A host-result call transposes a pass of lanes into a device array of the pass's whole result, rows x 56 bytes per lane, and copies
// that out with two contiguous copies.  Both figures are design constants, not measurements: 2 GiB is what a call may hold on the
// device for that array, and below 2^14 lanes per pass (rows >= 2341) the passes become too many and too small to be worth it --
// such a call scatters on the host as before.
constexpr size_t kBgPassBytes = size_t(2) << 30;
constexpr size_t kBgMinPassLanes = size_t(1) << 14;

struct InflxBgRowsPlan {
  size_t lanes_per_pass;  // lanes of every pass but the last
  bool transposed;        // rows go through inflx_bg_rows_transpose; false: the host scatters the planes
};

// How a call of B trajectories x `rows` rows that stores rows is split.  `device_result`: the caller's arrays are on the device, so
// no array of a pass's result exists and nothing bounds a pass but kBgMaxLanes.  `force_scatter`: INFLX_EOM_HOST_SCATTER.
inline InflxBgRowsPlan inflx_bg_rows_plan(size_t B, size_t rows, bool force_scatter, bool device_result = false) {
  const size_t chunk = B < kBgMaxLanes ? B : kBgMaxLanes;
  if (rows < 1) rows = 1;
  if (device_result) return {chunk, true};
  const size_t row_bytes = 7 * sizeof(double);
  const size_t fit = rows <= kBgPassBytes / row_bytes ? kBgPassBytes / (rows * row_bytes) : 0;
  if (force_scatter || fit < kBgMinPassLanes) return {chunk, false};
  return {chunk < fit ? chunk : fit, true};
}
