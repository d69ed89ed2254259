// Host twin of the reheating kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion header and the code the kernels run
// (csrc/inflx_reheating.h over csrc/inflx_background.h) for the CPU, and drives one trajectory the way inflx_rh_init and
// inflx_rh_advance_* drive a lane: init, then accepted steps until the lane stops or the steps run out.  Never used by the product.
// With REHEATING_TWIN_MAIN it is a stand-alone program (for a sanitizer build of the host code).
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
#include "inflx_reheating.h"

#define TWIN_ROW 15  // y[0..6], f[0..6], t

extern "C" {

static void twin_row(double* rows, size_t max_rows, size_t k, const InflxRhLane& s) {
  if (!rows || k >= max_rows) return;
  for (int c = 0; c < 7; ++c) {
    rows[k * TWIN_ROW + c] = s.y[c];
    rows[k * TWIN_ROW + 7 + c] = s.f[c];
  }
  rows[k * TWIN_ROW + 14] = s.t;
}

// One trajectory.  rows (max_rows, 15) or NULL: row 0 the initial state, row k the END state of the k-th accepted step (never a
// located one) with the right-hand side there and t; out (8): y[0..6] and t as the kernels' carry holds them when the lane stops -- the
// located state of a REHEATED lane, the last state held otherwise; meta = status, accepted steps, H_0, rows written
void twin_reheating(const double* p, const double* init, double gamma, double rho_r0, double omega_r, size_t max_steps, int method, double max_err, double dt,
                    double* rows, size_t max_rows, double* out, double* meta) {
  InflxRhLane s;
  InflxRhLocated loc;
  double accepted = 0.0;
  int status = inflx_rh_init(s, init, gamma, rho_r0, p, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, omega_r, loc);
  const double h0 = s.y[4];
  twin_row(rows, max_rows, 0, s);
  size_t written = 1;
  for (size_t k = 0; k < max_steps && status == INFLX_BG_RUNNING; ++k) {
    status = method == INFLX_BG_RKF ? inflx_rh_step<INFLX_BG_RKF>(s, p, max_err, dt, omega_r, loc) : inflx_rh_step<INFLX_BG_RK4>(s, p, max_err, dt, omega_r, loc);
    if (status == INFLX_BG_RUNNING || status == INFLX_RH_REHEATED) {
      accepted += 1.0;
      twin_row(rows, max_rows, written, s);
      ++written;
    }
  }
  const bool located = status == INFLX_RH_REHEATED;
  for (int c = 0; c < 7; ++c) out[c] = located ? loc.y[c] : s.y[c];
  out[7] = located ? loc.t : s.t;
  meta[0] = status;
  meta[1] = accepted;
  meta[2] = h0;
  meta[3] = (double)(written < max_rows || !rows ? written : max_rows);
}

// the model at `n` points (phi^0, phi^1, chi^0, chi^1): eom^0, eom^1, V, G_ab chi^a chi^b
void twin_eom(const double* p, const double* pts, size_t n, double* out) {
  for (size_t k = 0; k < n; ++k) inflx_eom_point(pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], p, out + 4 * k);
}
}

#ifdef REHEATING_TWIN_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>

// argv[1..]: the parameter row.  Two lanes from (0.8, 0.5) with the velocity (-0.3, 0.1): one with Gamma = 0.5 and no radiation, one
// whose initial radiation already dominates (reheated at the start); both steppers, adaptive and at a fixed dt with a max_steps that
// runs out.
int main(int argc, char** argv) {
  std::vector<double> p;
  for (int i = 1; i < argc; ++i) p.push_back(atof(argv[i]));
  const double init[4] = {0.8, 0.5, -0.3, 0.1};
  const double rho0[2] = {0.0, 1e3};
  std::vector<double> rows(64 * TWIN_ROW);
  double out[8], meta[4];
  for (int b = 0; b < 2; ++b)
    for (int method = 0; method < 2; ++method)
      for (int fixed = 0; fixed < 2; ++fixed) {
        twin_reheating(p.data(), init, 0.5, rho0[b], 0.9, fixed ? 40 : 100000, method, 1e-8, fixed ? 1e-3 : 0.0, rows.data(), 64, out, meta);
        printf("lane %d method %d fixed %d: status %d, accepted %d, rows %d, N %.6f, Omega_r %.6f\n", b, method, fixed, (int)meta[0], (int)meta[1], (int)meta[3], out[5],
               out[6] / (3.0 * out[4] * out[4]));
      }
  return 0;
}
#endif
