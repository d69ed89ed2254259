// Host twin of the evolution kernels -- TEST INFRASTRUCTURE.
//
// Compiles the generated model header, the generated equations-of-motion, kinematics and masses headers and the lane the kernels
// run (csrc/inflx_evolution.h over csrc/inflx_modes.h over csrc/inflx_background.h) for the CPU, and drives every lane the way
// inflx_ev_init and inflx_ev_advance_* drive it: init, then accepted steps until the lane stops or the steps run out, final values
// into planes [22][lane] and samples into planes [sample][6][lane] that start out NaN.  Never used by the product.
//
// With -DEVOLUTION_TWIN_MAIN it is a stand-alone program (for a build with -fsanitize=address,undefined): `evolution_twin FILE` reads
// the numbers n, n_par, S, max_steps, method, stop_at_end, max_err, dt and then the arrays p (n, n_par), init (n, 4), kappa (n,),
// n_target (n,; "nan": none), shift (n,), samples (S,) from the text file FILE, runs twin_evolution and prints status, cursor and the
// 6 S sample values of every lane, one lane per line, with 17 significant digits.
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
#include "inflx_evolution.h"

extern "C" {

struct TwinSink {
  double* base;     // plane 0 of the final values, at this lane
  double* sampled;  // plane 0 of sample 0, at this lane
  size_t n;
  unsigned* step_of;  // the accepted step (0: init) that emitted each sample of this lane
  unsigned step;
  void operator()(const double* o) const {
    for (int c = 0; c < INFLX_MD_NOUT; ++c) base[(size_t)c * n] = o[c];
  }
  void sample(unsigned k, const double* o) const {
    for (int c = 0; c < INFLX_EV_NSAMPLE; ++c) sampled[((size_t)k * INFLX_EV_NSAMPLE + c) * n] = o[INFLX_EV_SAMPLE_OF(c)];
    step_of[k] = step;
  }
};

// n lanes.  p: row l at p + l * p_stride; init (n, 4); kappa, n_target (NaN: none), shift (n,); samples (S,).  out (22, n); sampled
// (S, 6, n); lanes (n, 27): status, N_end, accepted steps, y[0..21] and t where the lane stopped (never a located state), cursor;
// step_of (n, S): the accepted step that emitted each sample (0: the initial state), untouched for a sample not emitted
void twin_evolution(const double* p, size_t p_stride, const double* init, const double* kappa, const double* n_target, const double* shift, const double* samples,
                    size_t S, size_t n, size_t max_steps, int method, double max_err, double dt, int stop_at_end, double* out, double* sampled, double* lanes,
                    unsigned* step_of) {
  for (size_t i = 0; i < (size_t)INFLX_MD_NOUT * n; ++i) out[i] = NAN;
  for (size_t i = 0; i < S * INFLX_EV_NSAMPLE * n; ++i) sampled[i] = NAN;
  for (size_t l = 0; l < n; ++l) {
    const double* pl = p + l * p_stride;
    InflxMdLane s;
    TwinSink sink{out + l, sampled + l, n, step_of + l * S, 0u};
    double n_end = NAN, accepted = 0.0;
    unsigned cursor = 0;
    int status = inflx_ev_init(s, init + 4 * l, pl, dt > 0.0 ? dt : INFLX_BG_FIRST_DT, stop_at_end != 0, kappa[l], n_target[l], samples, (unsigned)S, shift[l], cursor,
                               n_end, sink);
    for (size_t k = 0; k < max_steps && status == INFLX_BG_RUNNING; ++k) {
      sink.step = (unsigned)k + 1u;
      status = method == INFLX_BG_RKF
                   ? inflx_ev_step<INFLX_BG_RKF>(s, pl, max_err, dt, stop_at_end != 0, n_target[l], samples, (unsigned)S, shift[l], cursor, n_end, sink)
                   : inflx_ev_step<INFLX_BG_RK4>(s, pl, max_err, dt, stop_at_end != 0, n_target[l], samples, (unsigned)S, shift[l], cursor, n_end, sink);
      if (status == INFLX_BG_RUNNING || status == INFLX_BG_ENDED || status == INFLX_BG_TARGET) accepted += 1.0;
    }
    double* m = lanes + 27 * l;
    m[0] = status;
    m[1] = n_end;
    m[2] = accepted;
    for (int c = 0; c < INFLX_MD_NC; ++c) m[3 + c] = s.y[c];
    m[25] = s.t;
    m[26] = cursor;
  }
}
}

#ifdef EVOLUTION_TWIN_MAIN
#include <cstdio>
#include <vector>

static bool read_doubles(FILE* fh, std::vector<double>& v, size_t count) {
  v.resize(count);
  for (size_t i = 0; i < count; ++i)
    if (fscanf(fh, "%lf", &v[i]) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s FILE\n", argv[0]);
    return 2;
  }
  FILE* fh = fopen(argv[1], "r");
  if (!fh) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  unsigned long n = 0, n_par = 0, S = 0, max_steps = 0;
  int method = 0, stop_at_end = 0;
  double max_err = 0.0, dt = 0.0;
  std::vector<double> p, init, kappa, target, shift, samples;
  const bool ok = fscanf(fh, "%lu %lu %lu %lu %d %d %lf %lf", &n, &n_par, &S, &max_steps, &method, &stop_at_end, &max_err, &dt) == 8 && read_doubles(fh, p, n * n_par) &&
                  read_doubles(fh, init, n * 4) && read_doubles(fh, kappa, n) && read_doubles(fh, target, n) && read_doubles(fh, shift, n) && read_doubles(fh, samples, S);
  fclose(fh);
  if (!ok) {
    fprintf(stderr, "%s is incomplete\n", argv[1]);
    return 2;
  }
  std::vector<double> out(22 * n), sampled(S * INFLX_EV_NSAMPLE * n), lanes(27 * n);
  std::vector<unsigned> step_of(n * S, 0u);
  twin_evolution(p.data(), n_par, init.data(), kappa.data(), target.data(), shift.data(), samples.data(), S, n, max_steps, method, max_err, dt, stop_at_end, out.data(),
                 sampled.data(), lanes.data(), step_of.data());
  for (size_t l = 0; l < n; ++l) {
    printf("%d %u", (int)lanes[27 * l], (unsigned)lanes[27 * l + 26]);
    for (size_t i = 0; i < S * INFLX_EV_NSAMPLE; ++i) printf(" %.17g", sampled[i * n + l]);
    printf("\n");
  }
  return 0;
}
#endif
