// Host twin of the crossing kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion header and the code the kernels run
// (csrc/inflx_crossing.h over csrc/inflx_background.h and csrc/inflx_deltan.h) for the CPU, and drives one trajectory the way
// inflx_hx_advance_* and inflx_hx_end_* drive a lane: init, then accepted steps until the lane stops or the steps run out.  Never used
// by the product.  With CROSSING_TWIN_MAIN it is a stand-alone program (for a sanitizer build of the host code).
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
#include "inflx_background.h"
#include "inflx_deltan.h"
#include "inflx_crossing.h"

extern "C" {

// what the kernels' sink does, into out (S, 8): y[0..5], t, epsilon_H of every sample; `step_of` (S): the accepted step that emitted it
struct TwinSink {
  double* out;
  double* step_of;
  double accepted;
  void operator()(unsigned k, const InflxBgLocated& loc) const {
    for (int c = 0; c < 6; ++c) out[k * 8 + c] = loc.y[c];
    out[k * 8 + 6] = loc.t;
    out[k * 8 + 7] = loc.eps;
    step_of[k] = accepted;
  }
};

// One trajectory at the crossings offset + samples (S).  out (S, 8) and step_of (S) are NaN where a sample was not emitted (step_of:
// 0 = in init, k = in the k-th accepted step); meta = status, N_end, accepted steps, samples emitted, samples before the start
void twin_solve_crossings(const double* p, const double* init, double offset, const double* samples, unsigned S, size_t max_steps, int method, double max_err,
                          double dt, int stop_at_end, double* out, double* step_of, double* meta) {
  for (unsigned k = 0; k < S; ++k) {
    for (int c = 0; c < 8; ++c) out[k * 8 + c] = NAN;
    step_of[k] = NAN;
  }
  InflxBgLane s;
  TwinSink sink{out, step_of, 0.0};
  double n_end = NAN, accepted = 0.0;
  unsigned cursor = 0, n_before = 0;
  int status = inflx_hx_init_crossings(s, init, p, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, stop_at_end != 0, offset, samples, S, cursor, n_before, n_end, sink);
  for (size_t k = 0; k < max_steps && status == INFLX_BG_RUNNING; ++k) {
    sink.accepted = accepted + 1.0;  // (the step about to be taken)
    status = method == INFLX_BG_RKF ? inflx_hx_step_crossings<INFLX_BG_RKF>(s, p, max_err, dt, stop_at_end != 0, offset, samples, S, cursor, n_end, sink)
                                    : inflx_hx_step_crossings<INFLX_BG_RK4>(s, p, max_err, dt, stop_at_end != 0, offset, samples, S, cursor, n_end, sink);
    if (status == INFLX_BG_RUNNING || status == INFLX_BG_ENDED || status == INFLX_BG_TARGET) accepted += 1.0;
  }
  meta[0] = status;
  meta[1] = n_end;
  meta[2] = accepted;
  meta[3] = cursor - n_before;
  meta[4] = n_before;
}

// One trajectory to the located end of inflation.  out (8): y[0..5], t, epsilon_H there (NaN unless the lane ENDED); meta = status,
// accepted steps
void twin_inflation_end(const double* p, const double* init, size_t max_steps, int method, double max_err, double dt, double* out, double* meta) {
  for (int c = 0; c < 8; ++c) out[c] = NAN;
  InflxBgLane s;
  InflxBgLocated loc;
  double accepted = 0.0;
  int status = inflx_hx_init_end(s, init, p, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, loc);
  for (size_t k = 0; k < max_steps && status == INFLX_BG_RUNNING; ++k) {
    status = method == INFLX_BG_RKF ? inflx_hx_step_end<INFLX_BG_RKF>(s, p, max_err, dt, loc) : inflx_hx_step_end<INFLX_BG_RK4>(s, p, max_err, dt, loc);
    if (status == INFLX_BG_RUNNING || status == INFLX_BG_ENDED) accepted += 1.0;
  }
  if (status == INFLX_BG_ENDED) {
    for (int c = 0; c < 6; ++c) out[c] = loc.y[c];
    out[6] = loc.t;
    out[7] = loc.eps;
  }
  meta[0] = status;
  meta[1] = accepted;
}

// inflx_hx_locate on one step given by its ends: ends = N0, dN0, N1, dN1, H0, dH0, H1, dH1
double twin_locate(const double* ends, double h, double tau) { return inflx_hx_locate(ends[0], ends[1], ends[2], ends[3], ends[4], ends[5], ends[6], ends[7], h, tau); }
}

#ifdef CROSSING_TWIN_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>

// argv[1..]: the parameter row.  Two trajectories, from (3, 0.5) with the velocity (0, 0.1) and from (3, 0) with (5, 0), which starts past
// the end of inflation; seven targets relative to each one's own ln H_0, two of them before the start and one at it; both steppers,
// adaptive with stop_at_end and at a fixed dt with a max_steps that runs out; then the located end of inflation.
int main(int argc, char** argv) {
  std::vector<double> p;
  for (int i = 1; i < argc; ++i) p.push_back(atof(argv[i]));
  const double inits[2][4] = {{3.0, 0.5, 0.0, 0.1}, {3.0, 0.0, 5.0, 0.0}};
  const unsigned S = 7;
  const double samples[S] = {-1.0, -0.25, 0.0, 1e-3, 2e-3, 0.5, 40.0};
  std::vector<double> out(S * 8), step_of(S);
  double meta[5], end[8], emeta[2];
  for (int b = 0; b < 2; ++b) {
    InflxBgLane s;
    double n_end = 0.0;
    inflx_bg_init(s, inits[b], p.data(), 1e-3, false, n_end);
    const double l0 = log(s.y[4]);
    for (int method = 0; method < 2; ++method)
      for (int fixed = 0; fixed < 2; ++fixed) {
        twin_solve_crossings(p.data(), inits[b], l0, samples, S, fixed ? 300 : 100000, method, 1e-8, fixed ? 1e-3 : 0.0, !fixed, out.data(), step_of.data(), meta);
        twin_inflation_end(p.data(), inits[b], fixed ? 300 : 100000, method, 1e-8, fixed ? 1e-3 : 0.0, end, emeta);
        printf("trajectory %d method %d fixed %d: status %d, stored %d, before %d, accepted %d; end status %d, N_end %.6f\n", b, method, fixed, (int)meta[0], (int)meta[3],
               (int)meta[4], (int)meta[2], (int)emeta[0], end[5]);
      }
  }
  return 0;
}
#endif
