// Host twin of the target-on-N kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion header and the stepper the kernels run
// (csrc/inflx_background.h: inflx_bg_init_target, inflx_bg_step_target) for the CPU, and drives one trajectory the way
// inflx_bg_advance_*_target drive a lane: init, then accepted steps until the lane stops or the steps run out.  Never used by the
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

// One trajectory to its target on N.  out (8): y[0..5], t, epsilon_H of where the lane stopped (the located state for
// INFLX_BG_TARGET; epsilon_H is NaN otherwise); meta = status, N_end, accepted steps
void twin_solve_target(const double* p, const double* init, double target, size_t max_steps, int method, double max_err, double dt, int stop_at_end,
                       double* out, double* meta) {
  InflxBgLane s;
  InflxBgLocated loc;
  loc.eps = NAN;
  double n_end = NAN, accepted = 0.0;
  int status = inflx_bg_init_target(s, init, p, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, stop_at_end != 0, target, n_end, loc);
  for (size_t k = 0; k < max_steps && status == INFLX_BG_RUNNING; ++k) {
    status = method == INFLX_BG_RKF ? inflx_bg_step_target<INFLX_BG_RKF>(s, p, max_err, dt, stop_at_end != 0, target, n_end, loc)
                                    : inflx_bg_step_target<INFLX_BG_RK4>(s, p, max_err, dt, stop_at_end != 0, target, n_end, loc);
    if (status == INFLX_BG_RUNNING || status == INFLX_BG_ENDED || status == INFLX_BG_TARGET) accepted += 1.0;
  }
  const bool located = status == INFLX_BG_TARGET;
  for (int c = 0; c < 6; ++c) out[c] = located ? loc.y[c] : s.y[c];
  out[6] = located ? loc.t : s.t;
  out[7] = located ? loc.eps : NAN;
  meta[0] = status;
  meta[1] = n_end;
  meta[2] = accepted;
}
}
