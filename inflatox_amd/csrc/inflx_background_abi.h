// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_solve_eom) and the background kernels
// (csrc/inflx_background_kernels.hip): the kernels' argument blocks and the carry planes.  Both sides include this header; the
// background object exports INFLX_BG_ABI, and the host refuses an object whose value differs from its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_BG_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_BG_ABI_VERSION
#define INFLX_BG_ABI_VERSION 5
#endif
// the artefact ABI major a background object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there
// and here with -DINFLX_ABI_VERSION_MAJOR, which the background object is built with whenever the core object is)
#define INFLX_BG_DEFAULT_ABI_MAJOR 5

// carry planes [plane][lane] between launches
enum InflxBgCarry {
  INFLX_BG_CARRY_Y = 0,         // 0..5: phi^0, phi^1, chi^0, chi^1, H, N
  INFLX_BG_CARRY_T = 6,
  INFLX_BG_CARRY_DT = 7,
  INFLX_BG_CARRY_NEND = 8,      // N at epsilon_H = 1 (NaN until the lane ends there)
  INFLX_BG_CARRY_STATUS = 9,
  INFLX_BG_CARRY_LAST_ROW = 10, // index of the last row that holds a state (*_sampled kernels: the number of samples emitted)
  INFLX_BG_CARRY_PENDING = 11,  // 1: the lane ended inside a row that has not been written yet (that row holds the end state)
  INFLX_BG_CARRY_ROW_PLANES = 12,  // the planes inflx_solve_eom reads back
  INFLX_BG_CARRY_EPS = 12,      // epsilon_H at the located state of a lane that reached its target on N (NaN otherwise)
  INFLX_BG_CARRY_PLANES = 13,
};

// Argument block of inflx_bg_init and inflx_bg_advance_*.  A launch of the advance kernels processes the accepted-step indices
// [step_begin, step_begin + steps) of every lane -- the same indices for all lanes, whether they still run or not --, and row r is
// complete after step index r*substeps - 1; it goes to slot r - row_base of `rows`.  The *_target kernels (final-only, substeps = 1)
// stop a lane at its target on N as well: the lane's carry then holds the located state (planes Y, T, EPS).  They skip a lane that
// has stopped, and add the number of lanes still running after the launch to *running.  So do the *_sampled kernels (final-only,
// substeps = 1), whose lanes emit the state at every point of `samples` that an accepted step passes into `rows`, here planes
// [sample][8][n]: y[0..5], t, epsilon_H; the lane's cursor into `samples` is its carry plane LAST_ROW.  The host fills `rows` with NaN
// first: a sample that a lane never reaches stays NaN.
struct InflxBgArgs {
  const double* p;       // parameter rows of lane 0 of this launch
  uint64_t p_stride;     // doubles between the parameter rows of two lanes (0: one row for all)
  const double* init;    // (n, 4): phi^0, phi^1, chi^0, chi^1 (init kernel)
  double* carry;         // [INFLX_BG_CARRY_PLANES][n]
  double* rows;          // [slot][7][n]: y[0..5], t -- or NULL (*_sampled kernels: [sample][8][n], with epsilon_H)
  uint64_t n;            // lanes
  uint64_t step_begin;   // first accepted-step index of this launch
  uint64_t row_base;     // row held by slot 0 of `rows`
  uint32_t steps;        // accepted-step indices this launch processes (at most INFLX_BG_STEPS_PER_LAUNCH)
  uint32_t substeps;     // accepted steps per row
  uint32_t flags;        // bit 0: stop at epsilon_H = 1; bit 1: `samples` are times, not e-fold counts
  uint32_t n_samples;    // points in `samples`
  double max_err;
  double fixed_dt;       // > 0: fixed step
  const double* target;  // (n,): the target on N of every lane (init and *_target kernels) -- or NULL
  uint32_t* running;     // *_target and *_sampled kernels: one word, += the lanes still running when the launch ends
  const double* samples; // (n_samples,): the sample points of all lanes, strictly increasing (init and *_sampled kernels) -- or NULL
};
static_assert(sizeof(InflxBgArgs) == 120, "InflxBgArgs layout");
static_assert(offsetof(InflxBgArgs, step_begin) == 48 && offsetof(InflxBgArgs, steps) == 64 && offsetof(InflxBgArgs, max_err) == 80 &&
                  offsetof(InflxBgArgs, n_samples) == 76 && offsetof(InflxBgArgs, target) == 96 && offsetof(InflxBgArgs, running) == 104 &&
                  offsetof(InflxBgArgs, samples) == 112,
              "InflxBgArgs layout");

// bound of one launch: accepted steps per lane (each of at most 50 trials)
#define INFLX_BG_STEPS_PER_LAUNCH 256u

// Argument block of inflx_bg_rows_transpose (csrc/inflx_background_rows.h): one window of row planes -- the slots [0, filled) of
// `rows`, which hold the rows [row_base, row_base + filled) of n lanes -- into the trajectory-major arrays of inflx_solve_eom:
//   out_y[((lane_off + lane) * rows_total + row) * 6 + c], c = 0..5        out_t[(lane_off + lane) * rows_total + row]
// Nothing else of out_y / out_t is written; either may be NULL.
struct InflxBgRowsArgs {
  const double* rows;   // [slot][7][n]: y[0..5], t
  double* out_y;        // (lanes, rows_total, 6) -- or NULL
  double* out_t;        // (lanes, rows_total) -- or NULL
  uint64_t n;           // lanes of the planes
  uint64_t lane_off;    // trajectory of lane 0 in out_y / out_t
  uint64_t rows_total;  // rows per trajectory in out_y / out_t
  uint64_t row_base;    // row held by slot 0
  uint64_t filled;      // slots of the window
};
static_assert(sizeof(InflxBgRowsArgs) == 64, "InflxBgRowsArgs layout");
static_assert(offsetof(InflxBgRowsArgs, out_y) == 8 && offsetof(InflxBgRowsArgs, out_t) == 16 && offsetof(InflxBgRowsArgs, n) == 24 &&
                  offsetof(InflxBgRowsArgs, lane_off) == 32 && offsetof(InflxBgRowsArgs, rows_total) == 40 &&
                  offsetof(InflxBgRowsArgs, row_base) == 48 && offsetof(InflxBgRowsArgs, filled) == 56,
              "InflxBgRowsArgs layout");
