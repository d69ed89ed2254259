// Host twin of the tensor-mode kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion header and the stepper the kernels run
// (csrc/inflx_tensor.h over csrc/inflx_background.h) for the CPU, and drives every lane the way inflx_tn_init and
// inflx_tn_advance_* drive it: init, then accepted steps until the lane stops or the steps run out, outputs into planes [8][lane]
// that start out NaN.  Never used by the product.  With TENSOR_TWIN_MAIN it is a stand-alone program (for a sanitizer build of the
// host code): a few lanes of every stop rule, both steppers.
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
#include "inflx_tensor.h"

extern "C" {

struct TwinSink {
  double* base;  // plane 0, at this lane
  size_t n;
  void operator()(const double* o) const {
    for (int c = 0; c < INFLX_TN_NOUT; ++c) base[(size_t)c * n] = o[c];
  }
};

// n lanes.  p: row l at p + l * p_stride; init (n, 4); kappa (n,); n_target (n,), NaN: none.  out (8, n); lanes (n, 14): status,
// N_end, accepted steps, y[0..9] and t where the lane stopped (never a located state)
void twin_tensor(const double* p, size_t p_stride, const double* init, const double* kappa, const double* n_target, size_t n, size_t max_steps, int method,
                 double max_err, double dt, int stop_at_end, double* out, double* lanes) {
  for (size_t i = 0; i < (size_t)INFLX_TN_NOUT * n; ++i) out[i] = NAN;
  for (size_t l = 0; l < n; ++l) {
    const double* pl = p + l * p_stride;
    InflxTnLane s;
    TwinSink sink{out + l, n};
    double n_end = NAN, accepted = 0.0;
    int status = inflx_tn_init(s, init + 4 * l, pl, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, stop_at_end != 0, kappa[l], n_target[l], n_end, sink);
    for (size_t k = 0; k < max_steps && status == INFLX_BG_RUNNING; ++k) {
      status = method == INFLX_BG_RKF ? inflx_tn_step<INFLX_BG_RKF>(s, pl, max_err, dt, stop_at_end != 0, n_target[l], n_end, sink)
                                      : inflx_tn_step<INFLX_BG_RK4>(s, pl, max_err, dt, stop_at_end != 0, n_target[l], n_end, sink);
      if (status == INFLX_BG_RUNNING || status == INFLX_BG_ENDED || status == INFLX_BG_TARGET) accepted += 1.0;
    }
    double* m = lanes + 14 * l;
    m[0] = status;
    m[1] = n_end;
    m[2] = accepted;
    for (int c = 0; c < INFLX_TN_NC; ++c) m[3 + c] = s.y[c];
    m[13] = s.t;
  }
}
}

#ifdef TENSOR_TWIN_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>

// argv[1..]: the parameter row.  Four lanes from the state (3, 0.2, -0.3, 1e-3): a target, no target, a target <= 0 and a bad kappa.
int main(int argc, char** argv) {
  std::vector<double> p;
  for (int i = 1; i < argc; ++i) p.push_back(atof(argv[i]));
  const double init[16] = {3, 0.2, -0.3, 1e-3, 3, 0.2, -0.3, 1e-3, 3, 0.2, -0.3, 1e-3, 3, 0.2, -0.3, 1e-3};
  const double kappa[4] = {5.0, 5.0, 5.0, -1.0}, target[4] = {0.1, NAN, 0.0, 0.1};
  double out[8 * 4], lanes[14 * 4];
  for (int method = 0; method < 2; ++method) {
    twin_tensor(p.data(), 0, init, kappa, target, 4, 400, method, 1e-8, 0.0, 1, out, lanes);
    for (int l = 0; l < 4; ++l) printf("method %d lane %d: status %g, P_T %.17g, N %g\n", method, l, lanes[14 * l], out[l], out[5 * 4 + l]);
  }
  return 0;
}
#endif
