// Host twin of the first-passage histogram kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion and noise headers and the code the kernels run
// (csrc/inflx_distribution.h over csrc/inflx_stochastic.h, csrc/inflx_philox.h and csrc/inflx_background.h) for the CPU, and drives the
// L lanes of every point the way inflx_stochastic_distribution drives them: the lanes j < min(L, R) start with the tickets j, the others
// are retired; launches of `window` units per lane until every lane has retired.  The lanes of a launch are served one after the other,
// in the order `order` gives (a permutation of 0 .. L - 1, or none: 0, 1, ..), and share the point's ticket: reports and draws are plain
// additions here where the kernels use atomics.  Never used by the product.  With DISTRIBUTION_TWIN_MAIN it is a stand-alone program
// (for a sanitizer build of the host code).
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#define INFLX_HOST_TWIN 1
#define INFLX_FN static inline
using std::atan;
using std::cos;
using std::cosh;
using std::exp;
using std::fabs;
using std::floor;
using std::fmax;
using std::isfinite;
using std::lgamma;
using std::log;
using std::log1p;
using std::pow;
using std::sin;
using std::sinh;
using std::sqrt;
using std::tan;
using std::tanh;
using std::tgamma;

#include "inflx_device_math.h"
#include "inflx_kernel_abi.h"
#include "inflx_ops.h"
#include INFLX_MODEL_HEADER
#include INFLX_EOM_HEADER
#include INFLX_NOISE_HEADER
#include "inflx_background.h"
#include "inflx_distribution.h"

namespace {

struct SerialSink {
  uint32_t* hist;    // the point's row [below, bin 0 .. bins - 1, above]
  uint32_t* counts;  // the point's six status counters
  uint64_t* ticket;
  double lo, scale;
  uint32_t bins;
  void report(int status, double n_end) {
    if (status == INFLX_BG_ENDED) hist[inflx_pd_slot(n_end, lo, scale, bins)] += 1u;
    if ((unsigned)status < 6u) counts[status] += 1u;
  }
  uint64_t draw() { return (*ticket)++; }
};

struct Lane {
  InflxBgLane s;
  InflxPdCarry c;
};

}  // namespace

extern "C" {

// the slots of n values under (lo, scale, bins)
void twin_slots(const double* values, size_t n, double lo, double scale, uint32_t bins, uint32_t* out) {
  for (size_t i = 0; i < n; ++i) out[i] = inflx_pd_slot(values[i], lo, scale, bins);
}

// B points, the realisations first .. first + R - 1 of each on L lanes.  p: row b at p + b * p_stride; init (B, 4); streams (B,);
// bin (B, 2): lo and scale; order (L,) or NULL; hist (B, bins + 2) and counts (B, 6), cleared here.  Returns the launches of the
// slowest point, or -1 when a point went past launch_limit.
long twin_distribution(const double* p, size_t p_stride, const double* init, size_t B, uint64_t R, uint64_t first, size_t L, const uint32_t* streams, uint64_t seed,
                       double noise_scale, double dn_max, uint64_t max_steps, int method, double max_err, double dt, uint32_t bins, const double* bin,
                       uint32_t window, const uint32_t* order, long launch_limit, uint32_t* hist, uint32_t* counts) {
  long worst = 0;
  std::vector<Lane> lanes(L);
  for (size_t b = 0; b < B; ++b) {
    const double* pb = p + b * p_stride;
    const double* start = init + 4 * b;
    uint32_t* row = hist + b * ((size_t)bins + 2);
    uint32_t* cnt = counts + 6 * b;
    for (size_t k = 0; k < (size_t)bins + 2; ++k) row[k] = 0;
    for (int k = 0; k < 6; ++k) cnt[k] = 0;
    const uint64_t first_tickets = R < L ? R : L;
    uint64_t ticket = first_tickets;
    for (size_t j = 0; j < L; ++j) {
      Lane& l = lanes[j];
      l.c = InflxPdCarry{NAN, 0, ~UINT64_C(0), INFLX_BG_RUNNING};
      if (j < first_tickets) {
        l.c.ticket = j;
        l.c.status = inflx_st_init(l.s, start, pb, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, l.c.n_end);
      }
    }
    const InflxPdPoint q = {seed, first, R, max_steps, streams[b], noise_scale, dn_max, max_err, dt};
    SerialSink sink = {row, cnt, &ticket, bin[2 * b], bin[2 * b + 1], bins};
    long launches = 0;
    for (size_t running = 1; running != 0; ++launches) {
      if (launches >= launch_limit) return -1;
      running = 0;
      for (size_t k = 0; k < L; ++k) {
        Lane& l = lanes[order ? order[k] : k];
        if (!(l.c.ticket < R)) continue;
        // (a launch resumes from the carried y, t and dt: f and kin are recomputed, as the kernel recomputes them)
        if (l.c.status == INFLX_BG_RUNNING) inflx_st_resume(l.s, pb);
        const bool live = method == INFLX_BG_RKF ? inflx_pd_window<INFLX_BG_RKF>(l.s, l.c, q, start, pb, window, sink)
                                                 : inflx_pd_window<INFLX_BG_RK4>(l.s, l.c, q, start, pb, window, sink);
        running += live ? 1 : 0;
      }
    }
    worst = launches > worst ? launches : worst;
  }
  return worst;
}
}

#ifdef DISTRIBUTION_TWIN_MAIN
#include <cstdio>
#include <cstdlib>

// argv[1..]: the parameter row.  Two points x 150 realisations from (3, 0.2) and (2.5, -0.1) with the velocity (-0.3, 1e-3) on 64 lanes
// (150 is no multiple of 64: every lane is used again, and 42 lanes retire before the others), both steppers, adaptive and at a fixed dt
// with a max_steps that leaves some realisations unfinished; 16 bins.
int main(int argc, char** argv) {
  std::vector<double> p;
  for (int i = 1; i < argc; ++i) p.push_back(atof(argv[i]));
  const double init[8] = {3, 0.2, -0.3, 1e-3, 2.5, -0.1, -0.3, 1e-3};
  const uint32_t streams[2] = {7, 0xffffffffu};
  const size_t B = 2, L = 64;
  const uint64_t R = 150;
  const uint32_t bins = 16;
  const double bin[4] = {0.0, bins / 8.0, 0.0, bins / 8.0};
  std::vector<uint32_t> hist(B * (bins + 2)), counts(B * 6);
  for (int method = 0; method < 2; ++method)
    for (int fixed = 0; fixed < 2; ++fixed) {
      const long launches = twin_distribution(p.data(), 0, init, B, R, 5, L, streams, 0x123456789abcdef0ull, 1.0, 1.0 / 32.0, fixed ? 40 : 100000, method, 1e-8,
                                              fixed ? 1e-2 : 0.0, bins, bin, 256, nullptr, 1000000, hist.data(), counts.data());
      for (size_t b = 0; b < B; ++b) {
        unsigned long inside = 0, all = 0;
        for (uint32_t k = 1; k <= bins; ++k) inside += hist[b * (bins + 2) + k];
        for (int k = 0; k < 6; ++k) all += counts[6 * b + k];
        printf("method %d fixed %d point %zu: launches %ld, realisations %lu, ended %u, running %u, below %u, inside %lu, above %u\n", method, fixed, b, launches, all,
               counts[6 * b + 1], counts[6 * b], hist[b * (bins + 2)], inside, hist[b * (bins + 2) + bins + 1]);
      }
    }
  return 0;
}
#endif
