// Layout shared by libinflx_hip.so (csrc/inflx_hip.cpp, inflx_stochastic_distribution) and the distribution kernels
// (csrc/inflx_distribution_kernels.hip): the kernels' argument block, the carry planes and the rows of counts.  Both sides include
// this header; the distribution object exports INFLX_PD_ABI, and the host refuses an object whose value differs from its own.  The
// layout word is the distribution object's own: no other companion object's is involved (the stochastic object's INFLX_ST_ABI least
// of all: that object is neither loaded nor changed by this one).
#pragma once
#include <stddef.h>
#include <stdint.h>

// (overridable with -DINFLX_PD_ABI_VERSION=<n> so that a test can build an object of another layout version and see it refused)
#ifndef INFLX_PD_ABI_VERSION
#define INFLX_PD_ABI_VERSION 1
#endif

// the artefact ABI major a distribution object reports by default: the core object's (csrc/inflx_sweep_kernels.hip, overridable there
// and here with -DINFLX_ABI_VERSION_MAJOR, which the distribution object is built with whenever the core object is)
#define INFLX_PD_DEFAULT_ABI_MAJOR 5

#define INFLX_PD_THREADS 256
#define INFLX_PD_WAVE 64                         // lanes_per_point is a multiple of it: a wavefront's lanes belong to one point
#define INFLX_PD_MAX_LANES_PER_POINT (1u << 20)  // ... and at most this
#define INFLX_PD_MAX_BINS (1u << 20)
#define INFLX_PD_STATUSES 6  // InflxBgStatus 0..5

// carry planes [plane][lane] between launches, every plane of 8-byte words; lane = point * L + the lane's index within the point
enum InflxPdCarryPlane {
  INFLX_PD_CARRY_Y = 0,  // 0..5: phi^0, phi^1, chi^0, chi^1, H, N (double)
  INFLX_PD_CARRY_T = 6,
  INFLX_PD_CARRY_DT = 7,
  INFLX_PD_CARRY_RESULT = 8,  // N_end of the lane's realisation once it is INFLX_BG_ENDED (NaN until then)
  INFLX_PD_CARRY_DOUBLES = 9,
};
// ... and the planes of `words`, uint64_t
enum InflxPdWordPlane {
  INFLX_PD_WORD_STATUS = 0,  // of the lane's realisation
  INFLX_PD_WORD_STEPS = 1,   // its accepted steps so far: the Philox step index of its next kick
  INFLX_PD_WORD_TICKET = 2,  // its index among the R realisations of the call; >= R: the lane is retired
  INFLX_PD_CARRY_WORDS = 3,
};
#define INFLX_PD_CARRY_BYTES ((INFLX_PD_CARRY_DOUBLES + INFLX_PD_CARRY_WORDS) * 8)

// Argument block of inflx_pd_init and inflx_pd_advance_*.  A pass holds nb points of L lanes, lane = point * L + j.  Point b reads the
// parameter row p + b * p_stride, the initial state init[4 b .. 4 b + 3], its stream id streams[b] and its bins (lo, scale) =
// bin[2 b], bin[2 b + 1], and owns the ticket counter tickets[b], the row hist[b (bins + 2) ..] = [below, bin 0 .. bins - 1, above] and
// the status counts counts[6 b ..].  inflx_pd_init gives the lanes j < min(L, R) the tickets j, retires the others and sets tickets[b] =
// min(L, R); hist and counts are cleared by the host.  A launch of the advance kernels gives every lane that is not retired `steps`
// units (csrc/inflx_distribution.h inflx_pd_window) and adds the number of lanes not retired after it to *running.
struct InflxPdArgs {
  const double* p;          // parameter rows of point 0 of this pass
  uint64_t p_stride;        // doubles between the parameter rows of two points (0: one row for all)
  const double* init;       // (nb, 4): phi^0, phi^1, chi^0, chi^1
  const uint32_t* streams;  // (nb,): the points' stream ids
  const double* bin;        // (nb, 2): lo and scale = bins / (hi - lo) of every point
  double* carry;            // [INFLX_PD_CARRY_DOUBLES][nb * L]
  uint64_t* words;          // [INFLX_PD_CARRY_WORDS][nb * L]
  uint64_t* tickets;        // (nb,): the next ticket of every point
  uint32_t* hist;           // (nb, bins + 2)
  uint32_t* counts;         // (nb, INFLX_PD_STATUSES)
  uint32_t* running;        // one word, += the lanes not retired when the launch ends
  uint64_t nb;              // points of this pass
  uint64_t seed;            // the Philox key
  uint64_t first;           // first_realisation: ticket t is realisation first + t (first + R <= 2^32)
  uint64_t max_steps;       // accepted steps a realisation may take
  uint32_t R;               // realisations (tickets) per point
  uint32_t L;               // lanes per point, a multiple of INFLX_PD_WAVE
  uint32_t bins;
  uint32_t steps;           // units of a lane in this launch (at most INFLX_BG_STEPS_PER_LAUNCH)
  double noise_scale;
  double dn_max;            // adaptive runs: no step is tried that is longer than dn_max / H
  double max_err;
  double fixed_dt;          // > 0: fixed step
};
static_assert(sizeof(InflxPdArgs) == 168, "InflxPdArgs layout");
static_assert(offsetof(InflxPdArgs, p_stride) == 8 && offsetof(InflxPdArgs, init) == 16 && offsetof(InflxPdArgs, streams) == 24 &&
                  offsetof(InflxPdArgs, bin) == 32 && offsetof(InflxPdArgs, carry) == 40 && offsetof(InflxPdArgs, words) == 48 &&
                  offsetof(InflxPdArgs, tickets) == 56 && offsetof(InflxPdArgs, hist) == 64 && offsetof(InflxPdArgs, counts) == 72 &&
                  offsetof(InflxPdArgs, running) == 80 && offsetof(InflxPdArgs, nb) == 88 && offsetof(InflxPdArgs, seed) == 96 &&
                  offsetof(InflxPdArgs, first) == 104 && offsetof(InflxPdArgs, max_steps) == 112 && offsetof(InflxPdArgs, R) == 120 &&
                  offsetof(InflxPdArgs, L) == 124 && offsetof(InflxPdArgs, bins) == 128 && offsetof(InflxPdArgs, steps) == 132 &&
                  offsetof(InflxPdArgs, noise_scale) == 136 && offsetof(InflxPdArgs, dn_max) == 144 && offsetof(InflxPdArgs, max_err) == 152 &&
                  offsetof(InflxPdArgs, fixed_dt) == 160,
              "InflxPdArgs layout");
