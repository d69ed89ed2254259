// The lanes of one pass of a host-result call of the background solver whose device buffer holds a whole lane's result (the sampled,
// transfer and mode-function calls of csrc/inflx_hip.cpp).  Plain C++ without a HIP header: the host library and the CPU program
// tests/background_rows_twin.cpp include this file.  (It stands beside csrc/inflx_background_rows.h, not in it: that file is a
// source of the background object, whose bytes and cache key this rule has no part in.)
#pragma once
#include "inflx_background_rows.h"

// Lanes reach their results in different launches, so the buffer of kBgRowBytes holds everything a pass's lanes return,
// `bytes_per_lane` each: as many lanes as fit, at least one, in whole workgroups of `threads` where more than one workgroup fits, and
// no more than the call's B lanes or kBgMaxLanes.
inline size_t inflx_bg_lanes_per_pass(size_t B, size_t bytes_per_lane, size_t threads) {
  size_t lanes = kBgRowBytes / bytes_per_lane;
  if (lanes < 1) lanes = 1;
  if (lanes > threads) lanes -= lanes % threads;
  if (lanes > kBgMaxLanes) lanes = kBgMaxLanes;
  return lanes < B ? lanes : B;
}
