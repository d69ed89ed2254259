// Host twin of the transfer kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion, kinematics and masses headers and the stepper the
// kernels run (csrc/inflx_transfer.h over csrc/inflx_background.h) for the CPU, and drives every trajectory the way
// inflx_tr_init and inflx_tr_advance_* drive a lane: init, then accepted steps until the lane stops or the steps run out, samples
// into planes [sample][10][lane] that start out NaN.  Never used by the product.
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
#include "inflx_transfer.h"

extern "C" {

struct TwinSink {
  double* base;  // plane 0 of sample 0, at this lane
  size_t n;
  void operator()(unsigned k, const InflxTrSample& smp) const {
    double* out = base + (size_t)k * 10 * n;
    for (int c = 0; c < 6; ++c) out[(size_t)c * n] = smp.loc.y[c];
    out[6 * n] = smp.loc.t;
    out[7 * n] = smp.loc.eps;
    out[8 * n] = smp.t_ss;
    out[9 * n] = smp.t_rs;
  }
};

// B trajectories.  p: row l at p + l * p_stride; init (B, 4); dq_dn (B,) or NULL; samples (S,).  out (S, 10, B); lanes (B, 16):
// status, N_end, samples emitted, T_SS_end, T_RS_end, accepted steps, y[0..8] and t where the lane stopped (never a located state)
void twin_transfer(const double* p, size_t p_stride, const double* init, const double* dq_dn, size_t B, const double* samples, unsigned S, size_t max_steps,
                   int method, double max_err, double dt, int stop_at_end, double* out, double* lanes) {
  for (size_t i = 0; i < (size_t)S * 10 * B; ++i) out[i] = NAN;
  for (size_t l = 0; l < B; ++l) {
    const double* pl = p + l * p_stride;
    InflxTrLane s;
    TwinSink sink{out + l, B};
    double n_end = NAN, ends[2] = {NAN, NAN}, accepted = 0.0;
    unsigned cursor = 0;
    int status = inflx_tr_init(s, init + 4 * l, pl, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, stop_at_end != 0, dq_dn != nullptr, dq_dn ? dq_dn[l] : 0.0, samples, S,
                               cursor, n_end, ends, sink);
    for (size_t k = 0; k < max_steps && status == INFLX_BG_RUNNING; ++k) {
      status = method == INFLX_BG_RKF ? inflx_tr_step_sampled<INFLX_BG_RKF>(s, pl, max_err, dt, stop_at_end != 0, samples, S, cursor, n_end, ends, sink)
                                      : inflx_tr_step_sampled<INFLX_BG_RK4>(s, pl, max_err, dt, stop_at_end != 0, samples, S, cursor, n_end, ends, sink);
      if (status == INFLX_BG_RUNNING || status == INFLX_BG_ENDED || status == INFLX_BG_TARGET) accepted += 1.0;
    }
    double* m = lanes + 16 * l;
    m[0] = status;
    m[1] = n_end;
    m[2] = cursor;
    m[3] = ends[0];
    m[4] = ends[1];
    m[5] = accepted;
    for (int c = 0; c < INFLX_TR_NC; ++c) m[6 + c] = s.y[c];
    m[15] = s.t;
  }
}
}
