// Host twin of the background kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion header (staging.emit_eom_header) and the very
// integrator the kernels run (csrc/inflx_background.h) for the CPU, and drives one trajectory the way
// csrc/inflx_background_kernels.hip drives a lane: init, then rows of `substeps` accepted steps.  Never used by the product.
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

// out: (n, 4) -- eom^0, eom^1, V, G_ab xd^a xd^b at the points pts (n, 4) = (x0, x1, xd0, xd1)
void twin_eom(const double* p, const double* pts, size_t n, double* out) {
  for (size_t k = 0; k < n; ++k) inflx_eom_point(pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], p, out + 4 * k);
}

// the status word the model's special functions leave their domain notes in (csrc/inflx_sf.h: the host word of this library);
// reading clears it, as sf_status_take of tests/sf_host.cpp does
unsigned twin_sf_status_take() {
  const unsigned v = inflx_sf_status_host;
  inflx_sf_status_host = 0u;
  return v;
}

// One trajectory: rows (rows, 7) = y[0..5], t (NaN after the lane stopped); meta = status, N_end, last_row, accepted steps
void twin_solve(const double* p, const double* init, size_t rows, unsigned substeps, int method, double max_err, double dt, int stop_at_end,
                double* out, double* meta) {
  InflxBgLane s;
  double n_end = NAN, last_row = 0.0, accepted = 0.0;
  int status = inflx_bg_init(s, init, p, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, stop_at_end != 0, n_end);
  for (int c = 0; c < 6; ++c) out[c] = s.y[c];
  out[6] = s.t;
  for (size_t r = 1; r < rows; ++r) {
    int st = status;
    bool ended_now = false;
    if (st == INFLX_BG_RUNNING) {
      for (unsigned k = 0; k < substeps; ++k) {
        st = method == INFLX_BG_RKF ? inflx_bg_step<INFLX_BG_RKF>(s, p, max_err, dt, stop_at_end != 0, n_end)
                                    : inflx_bg_step<INFLX_BG_RK4>(s, p, max_err, dt, stop_at_end != 0, n_end);
        if (st == INFLX_BG_RUNNING || st == INFLX_BG_ENDED) accepted += 1.0;
        if (st != INFLX_BG_RUNNING) break;
      }
      ended_now = st == INFLX_BG_ENDED;
    }
    const bool valid = st == INFLX_BG_RUNNING || ended_now;
    if (valid) last_row = (double)r;
    for (int c = 0; c < 6; ++c) out[r * 7 + c] = valid ? s.y[c] : NAN;
    out[r * 7 + 6] = valid ? s.t : NAN;
    status = st;
  }
  meta[0] = status;
  meta[1] = n_end;
  meta[2] = last_row;
  meta[3] = accepted;
}
}
