// Host twin of the sampled kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion header and the stepper the kernels run
// (csrc/inflx_background.h: inflx_bg_init_sampled, inflx_bg_step_sampled) for the CPU, and drives one trajectory the way
// inflx_bg_advance_*_sampled drive a lane: init, then accepted steps until the lane stops or the steps run out.  Never used by the
// product.
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

// One trajectory sampled at `samples` (S; times when sample_t).  out (S, 8) and step_of (S) are NaN where a sample was not emitted
// (step_of: 0 = in init, k = in the k-th accepted step); meta = status, N_end, accepted steps, samples emitted
void twin_solve_sampled(const double* p, const double* init, const double* samples, unsigned S, int sample_t, size_t max_steps, int method,
                        double max_err, double dt, int stop_at_end, double* out, double* step_of, double* meta) {
  for (unsigned k = 0; k < S; ++k) {
    for (int c = 0; c < 8; ++c) out[k * 8 + c] = NAN;
    step_of[k] = NAN;
  }
  InflxBgLane s;
  TwinSink sink{out, step_of, 0.0};
  double n_end = NAN, accepted = 0.0;
  unsigned cursor = 0;
  int status = inflx_bg_init_sampled(s, init, p, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, stop_at_end != 0, samples, S, cursor, n_end, sink);
  for (size_t k = 0; k < max_steps && status == INFLX_BG_RUNNING; ++k) {
    sink.accepted = accepted + 1.0;  // (the step about to be taken)
    status = method == INFLX_BG_RKF
                 ? inflx_bg_step_sampled<INFLX_BG_RKF>(s, p, max_err, dt, stop_at_end != 0, samples, S, sample_t != 0, cursor, n_end, sink)
                 : inflx_bg_step_sampled<INFLX_BG_RK4>(s, p, max_err, dt, stop_at_end != 0, samples, S, sample_t != 0, cursor, n_end, sink);
    if (status == INFLX_BG_RUNNING || status == INFLX_BG_ENDED || status == INFLX_BG_TARGET) accepted += 1.0;
  }
  meta[0] = status;
  meta[1] = n_end;
  meta[2] = accepted;
  meta[3] = cursor;
}
}
