// Host twin of the masses kernel -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion, kinematics and masses headers (staging.emit_eom_header,
// staging.emit_kinematics_header, staging.emit_masses_header) and the very device function the kernel runs (csrc/inflx_masses.h)
// for the CPU, and walks the states the way csrc/inflx_masses_kernels.hip does: state i at y[i * ld], its parameter row at p +
// (i / traj_len) * p_stride, the eight quantities into planes out[q * n + i].  Never used by the product.
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
#include "inflx_masses.h"

extern "C" {

// out: (8, n) planes -- V_TT, V_TN, V_NN, ricci, eps_H, omega, M_eff2, mu_s2
void twin_masses(const double* p, size_t p_stride, const double* y, size_t n, size_t ld, size_t traj_len, double* out) {
  for (size_t i = 0; i < n; ++i) {
    double q[INFLX_MASS_QUANTITIES];
    inflx_mass_eval(y + i * ld, p + (i / traj_len) * p_stride, q);
    for (int c = 0; c < INFLX_MASS_QUANTITIES; ++c) out[(size_t)c * n + i] = q[c];
  }
}

// out: (n, 4) -- inflx_mass_point's o[0..3] at the points pts (n, 4) = (x0, x1, xd0, xd1), one parameter row for all
void twin_mass_point(const double* p, const double* pts, size_t n, double* out) {
  for (size_t k = 0; k < n; ++k) inflx_mass_point(pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], p, out + 4 * k);
}
}
