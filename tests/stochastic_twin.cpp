// Host twin of the stochastic e-fold kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion and noise headers and the code the kernels run
// (csrc/inflx_stochastic.h and csrc/inflx_philox.h over csrc/inflx_background.h) for the CPU, and drives every lane the way
// inflx_stochastic_efolds drives it: lane = point * R + realisation, one accepted step and its kick per step index, then the reduction
// of every point in the order of inflx_st_reduce (256 strided partial results, a butterfly over 64, four wavefronts in order).  Never
// used by the product.  With STOCHASTIC_TWIN_MAIN it is a stand-alone program (for a sanitizer build of the host code).
#include <cmath>
#include <cstddef>
#include <cstdint>

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
#include "inflx_stochastic.h"

extern "C" {

void twin_philox(const uint32_t* counter, uint32_t k0, uint32_t k1, uint32_t* out) { inflx_philox4x32_10(counter, k0, k1, out); }

double twin_uniform(uint32_t hi, uint32_t lo) { return inflx_philox_uniform(hi, lo); }

// xi (n, 2) of the steps step_begin .. step_begin + n - 1 of realisation r of stream `stream`
void twin_normals(uint64_t seed, uint64_t step_begin, size_t n, uint32_t r, uint32_t stream, double* xi) {
  for (size_t i = 0; i < n; ++i) inflx_philox_normals(seed, step_begin + i, r, stream, xi + 2 * i);
}

// inflx_noise_point at n points pts (n, 2): out (n, 5)
void twin_noise_point(const double* p, const double* pts, size_t n, double* out) {
  for (size_t i = 0; i < n; ++i) inflx_noise_point(pts[2 * i], pts[2 * i + 1], p, out + 5 * i);
}

// B points x R realisations.  p: row b at p + b * p_stride; init (B, 4); streams (B,).  samples (7, B R) as inflx_stochastic_efolds';
// accepted (B R,): the step indices every lane went through
void twin_stochastic(const double* p, size_t p_stride, const double* init, size_t B, size_t R, const uint32_t* streams, uint64_t seed, double noise_scale,
                     double dn_max, double n_stop, size_t max_steps, int method, double max_err, double dt, double* samples, double* accepted) {
  const size_t total = B * R;
  for (size_t lane = 0; lane < total; ++lane) {
    const size_t b = lane / R;
    const double* pb = p + b * p_stride;
    const InflxStNoise nz = {seed, (uint32_t)(lane - b * R), streams[b], noise_scale};
    InflxBgLane s;
    double n_end = NAN;
    int st = inflx_st_init(s, init + 4 * b, pb, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, n_end);
    size_t k = 0;
    for (; k < max_steps && st == INFLX_BG_RUNNING; ++k)
      st = method == INFLX_BG_RKF ? inflx_st_step<INFLX_BG_RKF>(s, pb, max_err, dt, dn_max, n_stop, nz, k, n_end)
                                  : inflx_st_step<INFLX_BG_RK4>(s, pb, max_err, dt, dn_max, n_stop, nz, k, n_end);
    samples[lane] = st == INFLX_BG_ENDED ? n_end : s.y[5];
    for (int c = 0; c < 5; ++c) samples[(size_t)(1 + c) * total + lane] = s.y[c];
    samples[6 * total + lane] = st;
    accepted[lane] = (double)k;
  }
}

// the reduction of one point in inflx_st_reduce's order: result and status (R,), out (12,)
void twin_moments(const double* result, const double* status, size_t R, double* out) {
  InflxStSum acc[256];
  for (size_t t = 0; t < 256; ++t) {
    inflx_st_sum_clear(acc[t]);
    for (size_t r = t; r < R; r += 256) inflx_st_sum_add(acc[t], result[r], (int)status[r]);
  }
  for (int off = 32; off > 0; off >>= 1) {
    InflxStSum next[256];
    for (size_t t = 0; t < 256; ++t) {
      const InflxStSum& o = acc[(t & ~(size_t)63) | ((t & 63) ^ (size_t)off)];
      next[t] = acc[t];
      inflx_st_sum_merge(next[t], o.sum, o.comp, o.count);
    }
    for (size_t t = 0; t < 256; ++t) acc[t] = next[t];
  }
  InflxStSum total = acc[0];
  for (int w = 1; w < 4; ++w) inflx_st_sum_merge(total, acc[64 * w].sum, acc[64 * w].comp, acc[64 * w].count);
  const double mean = inflx_st_sum_mean(total);
  static InflxStMoments m[256], next[256];
  for (size_t t = 0; t < 256; ++t) {
    inflx_st_moments_clear(m[t]);
    for (size_t r = t; r < R; r += 256) inflx_st_moments_add(m[t], result[r], (int)status[r], mean);
  }
  for (int off = 32; off > 0; off >>= 1) {
    for (size_t t = 0; t < 256; ++t) {
      next[t] = m[t];
      inflx_st_moments_merge(next[t], m[(t & ~(size_t)63) | ((t & 63) ^ (size_t)off)]);
    }
    for (size_t t = 0; t < 256; ++t) m[t] = next[t];
  }
  InflxStMoments all = m[0];
  for (int w = 1; w < 4; ++w) inflx_st_moments_merge(all, m[64 * w]);
  inflx_st_finish(mean, all, out);
}
}

#ifdef STOCHASTIC_TWIN_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>

// argv[1..]: the parameter row.  Two points x 70 realisations from (3, 0.2) and (2.5, -0.1) with the velocity (-0.3, 1e-3), both steppers,
// adaptive to the end of inflation and with a stop after a quarter of an e-fold at a fixed dt; then the reduction of every point.
int main(int argc, char** argv) {
  std::vector<double> p;
  for (int i = 1; i < argc; ++i) p.push_back(atof(argv[i]));
  const double init[8] = {3, 0.2, -0.3, 1e-3, 2.5, -0.1, -0.3, 1e-3};
  const uint32_t streams[2] = {7, 0xffffffffu};
  const size_t B = 2, R = 70;
  std::vector<double> samples(7 * B * R), accepted(B * R);
  double out[12];
  for (int method = 0; method < 2; ++method)
    for (int stop = 0; stop < 2; ++stop) {
      twin_stochastic(p.data(), 0, init, B, R, streams, 0x123456789abcdef0ull, 1.0, stop ? INFINITY : 1.0 / 32.0, stop ? 0.25 : NAN, 100000, method, 1e-8,
                      stop ? 1e-2 : 0.0, samples.data(), accepted.data());
      for (size_t b = 0; b < B; ++b) {
        twin_moments(samples.data() + b * R, samples.data() + 6 * B * R + b * R, R, out);
        printf("method %d stop %d point %zu: status of lane 0 %g, mean %.17g, m2 %.17g, ended %g, target %g\n", method, stop, b, samples[6 * B * R + b * R], out[0], out[1],
               out[7], out[11]);
      }
    }
  uint32_t c[4] = {0, 0, 0, 0}, w[4];
  twin_philox(c, 0, 0, w);
  printf("philox(0; 0) = %08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
  return 0;
}
#endif
