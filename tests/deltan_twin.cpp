// Host twin of the delta-N kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion header and the code the kernels run (csrc/inflx_deltan.h over
// csrc/inflx_background.h) for the CPU, and drives every stencil the way inflx_delta_n drives it: phase A on the centre (unless H_end is
// given), phase B on the nine members, inflx_dn_reduce.  Never used by the product.  With DELTAN_TWIN_MAIN it is a stand-alone
// program (for a sanitizer build of the host code): one stencil per velocity rule, both steppers.
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

extern "C" {

// B stencils.  p: row b at p + b * p_stride; centre (B, 4); vel (B, 9, 2) or NULL; h_end (B,) or NULL.  out (21, B) as inflx_delta_n's;
// surface (2, B): H_c, N_c; members (B, 9, 3): status, N on the surface, accepted steps; centres (B, 3): the same of phase A (status
// INFLX_DN_LOCATED, NaN, 0 when h_end is given)
void twin_delta_n(const double* p, size_t p_stride, const double* centre, const double* vel, int rule, double h0, double h1, const double* h_end, size_t B,
                  size_t max_steps, int method, double max_err, double dt, double* out, double* surface, double* members, double* centres) {
  const double dt0 = dt > 0.0 ? dt : INFLX_BG_FIRST_DT;
  for (size_t b = 0; b < B; ++b) {
    const double* pb = p + b * p_stride;
    const double* cb = centre + 4 * b;
    double h_c = NAN, n_c = NAN, accepted = 0.0;
    int status_a = INFLX_DN_LOCATED;
    if (h_end) {
      h_c = h_end[b];
    } else {
      double init[4];
      inflx_dn_member(cb, h0, h1, INFLX_DN_CENTRE, rule, vel ? vel + (9 * b + INFLX_DN_CENTRE) * 2 : nullptr, pb, init);
      InflxBgLane s;
      status_a = inflx_dn_init(s, init, pb, dt0, true, NAN, n_c);
      if (status_a == INFLX_DN_LOCATED) h_c = s.y[4];
      for (size_t k = 0; k < max_steps && status_a == INFLX_BG_RUNNING; ++k) {
        status_a = method == INFLX_BG_RKF ? inflx_dn_step_end<INFLX_BG_RKF>(s, pb, max_err, dt, h_c, n_c) : inflx_dn_step_end<INFLX_BG_RK4>(s, pb, max_err, dt, h_c, n_c);
        if (status_a == INFLX_BG_RUNNING || status_a == INFLX_DN_LOCATED) accepted += 1.0;
      }
      if (status_a != INFLX_DN_LOCATED) h_c = n_c = NAN;
    }
    centres[3 * b] = status_a;
    centres[3 * b + 1] = n_c;
    centres[3 * b + 2] = accepted;
    surface[b] = h_c;
    surface[B + b] = n_c;
    double n9[9], h_star = NAN;
    int st9[9];
    for (int m = 0; m < 9; ++m) {
      double init[4];
      inflx_dn_member(cb, h0, h1, m, rule, vel ? vel + (9 * b + m) * 2 : nullptr, pb, init);
      InflxBgLane s;
      double result = NAN, taken = 0.0;
      int st = inflx_dn_init(s, init, pb, dt0, false, h_c, result);
      if (m == INFLX_DN_CENTRE) h_star = s.y[4];
      for (size_t k = 0; k < max_steps && st == INFLX_BG_RUNNING; ++k) {
        st = method == INFLX_BG_RKF ? inflx_dn_step_surface<INFLX_BG_RKF>(s, pb, max_err, dt, h_c, result) : inflx_dn_step_surface<INFLX_BG_RK4>(s, pb, max_err, dt, h_c, result);
        if (st == INFLX_BG_RUNNING || st == INFLX_DN_LOCATED) taken += 1.0;
      }
      n9[m] = result;
      st9[m] = st;
      double* mm = members + (9 * b + m) * 3;
      mm[0] = st;
      mm[1] = result;
      mm[2] = taken;
    }
    double o[INFLX_DN_NOUT];
    inflx_dn_reduce(n9, st9, status_a, cb, h0, h1, h_star, pb, o);
    for (int c = 0; c < INFLX_DN_NOUT; ++c) out[(size_t)c * B + b] = o[c];
  }
}

// inflx_dn_reduce alone on given planes: n9 (B, 9), st9 (B, 9), x (B, 2), h_star (B,), one parameter row; out (21, B)
void twin_reduce(const double* p, const double* n9, const int* st9, int status_a, const double* x, double h0, double h1, const double* h_star, size_t B, double* out) {
  for (size_t b = 0; b < B; ++b) {
    double o[INFLX_DN_NOUT];
    inflx_dn_reduce(n9 + 9 * b, st9 + 9 * b, status_a, x + 2 * b, h0, h1, h_star[b], p, o);
    for (int c = 0; c < INFLX_DN_NOUT; ++c) out[(size_t)c * B + b] = o[c];
  }
}
}

#ifdef DELTAN_TWIN_MAIN
#include <cstdio>
#include <cstdlib>
#include <vector>

// argv[1..]: the parameter row.  One stencil around (3, 0.2) with the velocity (-0.3, 1e-3), h = 1e-2, under each rule, both steppers.
int main(int argc, char** argv) {
  std::vector<double> p;
  for (int i = 1; i < argc; ++i) p.push_back(atof(argv[i]));
  const double centre[4] = {3, 0.2, -0.3, 1e-3};
  double vel[18];
  for (int m = 0; m < 9; ++m) {
    vel[2 * m] = -0.3;
    vel[2 * m + 1] = 1e-3 * m;
  }
  double out[21], surface[2], members[27], centres[3];
  for (int method = 0; method < 2; ++method)
    for (int rule = 0; rule < 3; ++rule) {
      twin_delta_n(p.data(), 0, centre, rule == INFLX_DN_EXPLICIT ? vel : nullptr, rule, 1e-2, 1e-2, nullptr, 1, 100000, method, 1e-8, 0.0, out, surface, members, centres);
      printf("method %d rule %d: status %g, N %.17g, H_c %.17g, f_NL %.17g\n", method, rule, out[20], out[4], surface[0], out[18]);
    }
  return 0;
}
#endif
