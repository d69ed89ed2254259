// Host twin of the mode-function kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion, kinematics and masses headers and the stepper the
// kernels run (csrc/inflx_modes.h over csrc/inflx_background.h) for the CPU, and drives every lane the way inflx_md_init and
// inflx_md_advance_* drive it: init, then accepted steps until the lane stops or the steps run out, outputs into planes [22][lane]
// that start out NaN.  Never used by the product.
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
#include INFLX_KIN_HEADER
#include INFLX_MASS_HEADER
#include "inflx_background.h"
#include "inflx_modes.h"

extern "C" {

struct TwinSink {
  double* base;  // plane 0, at this lane
  size_t n;
  void operator()(const double* o) const {
    for (int c = 0; c < INFLX_MD_NOUT; ++c) base[(size_t)c * n] = o[c];
  }
};

// n lanes.  p: row l at p + l * p_stride; init (n, 4); kappa (n,); n_target (n,), NaN: none.  out (22, n); lanes (n, 26): status,
// N_end, accepted steps, y[0..21] and t where the lane stopped (never a located state)
void twin_modes(const double* p, size_t p_stride, const double* init, const double* kappa, const double* n_target, size_t n, size_t max_steps, int method,
                double max_err, double dt, int stop_at_end, double* out, double* lanes) {
  for (size_t i = 0; i < (size_t)INFLX_MD_NOUT * n; ++i) out[i] = NAN;
  for (size_t l = 0; l < n; ++l) {
    const double* pl = p + l * p_stride;
    InflxMdLane s;
    TwinSink sink{out + l, n};
    double n_end = NAN, accepted = 0.0;
    int status = inflx_md_init(s, init + 4 * l, pl, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, stop_at_end != 0, kappa[l], n_target[l], n_end, sink);
    for (size_t k = 0; k < max_steps && status == INFLX_BG_RUNNING; ++k) {
      status = method == INFLX_BG_RKF ? inflx_md_step<INFLX_BG_RKF>(s, pl, max_err, dt, stop_at_end != 0, n_target[l], n_end, sink)
                                      : inflx_md_step<INFLX_BG_RK4>(s, pl, max_err, dt, stop_at_end != 0, n_target[l], n_end, sink);
      if (status == INFLX_BG_RUNNING || status == INFLX_BG_ENDED || status == INFLX_BG_TARGET) accepted += 1.0;
    }
    double* m = lanes + 26 * l;
    m[0] = status;
    m[1] = n_end;
    m[2] = accepted;
    for (int c = 0; c < INFLX_MD_NC; ++c) m[3 + c] = s.y[c];
    m[25] = s.t;
  }
}
}
