// TEST INFRASTRUCTURE: the power rewrites and the fast divisions of csrc/inflx_device_math.h on the device, against the operations
// they replace -- OCML's pow (class and sign of the result at edge arguments), powl on the host (values, with a derived
// allowance) and the compiler's own a / b (bit for bit).  usage: device_math_probe [log2 of the random operands per helper, default 20]
// Prints counts, worst ratios and the first offending operands; exit status 1 on any mismatch, 2 on a HIP error.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>
#include "inflx_device_math.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static double from_bits(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
static uint64_t to_bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
static double random_significand(int exponent, bool negative) { return from_bits((rnd() & 0x000FFFFFFFFFFFFFull) | ((uint64_t)(1023 + exponent) << 52) | ((uint64_t)negative << 63)); }
static double next_up(double x, int steps) { return from_bits(to_bits(x) + (int64_t)steps); }  // (in magnitude; x != 0, finite)

// =====================================================================================================================
// powers
// =====================================================================================================================
// the four forms staging.py:_print_Pow emits: inflx_ipow<n>(x), (1.0/inflx_ipow<n>(x)), inflx_hpow<n>(x), (1.0/inflx_hpow<n>(x));
// the stand-alone x**(-1/2) is the last one with n = 1
enum { IPOW = 0, RIPOW = 1, HPOW = 2, RHPOW = 3 };
struct PowForm { int kind, n; double e; };  // e: the exponent of the reference's pow call

#define INFLX_IP(N) case N: return inflx_ipow<N>(x);
#define INFLX_HP(N) case N: return inflx_hpow<N>(x);
#define INFLX_HC(N) case N: return inflx_hpow_checked<N>(x, ok);
__device__ double ipow_n(int n, double x) {
  switch (n) { INFLX_IP(2) INFLX_IP(3) INFLX_IP(4) INFLX_IP(5) INFLX_IP(6) INFLX_IP(7) INFLX_IP(8) INFLX_IP(9) INFLX_IP(10) INFLX_IP(11) INFLX_IP(12) INFLX_IP(13) INFLX_IP(14) INFLX_IP(15) INFLX_IP(16) }
  return 0.0;
}
__device__ double hpow_n(int n, double x) {
  switch (n) { INFLX_HP(1) INFLX_HP(3) INFLX_HP(5) INFLX_HP(7) INFLX_HP(9) INFLX_HP(11) INFLX_HP(13) INFLX_HP(15) INFLX_HP(17) INFLX_HP(19) INFLX_HP(21) INFLX_HP(23) INFLX_HP(25) INFLX_HP(27) INFLX_HP(29) INFLX_HP(31) }
  return 0.0;
}
__device__ double hpow_checked_n(int n, double x, bool& ok) {
  switch (n) { INFLX_HC(1) INFLX_HC(3) INFLX_HC(5) INFLX_HC(7) INFLX_HC(9) INFLX_HC(11) INFLX_HC(13) INFLX_HC(15) INFLX_HC(17) INFLX_HC(19) INFLX_HC(21) INFLX_HC(23) INFLX_HC(25) INFLX_HC(27) INFLX_HC(29) INFLX_HC(31) }
  return 0.0;
}
// OCML's general pow.  The exponent arrives from memory, so the compiler cannot turn the call into something else (pow(x, 2.0) -> x*x).
__device__ __noinline__ double ocml_pow(double x, double e) { return pow(x, e); }

// item i: base x[i], form f[i].  got = our spelling, ref = OCML pow(x, e) in the same kernel; for the half powers also the quick
// variant (inflx_hpow_checked) and whether its guard accepted the argument.
__global__ void power_probe(const double* x, const int* f, const PowForm* forms, size_t n, double* got, double* ref, double* quick, unsigned char* quick_ok) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PowForm form = forms[f[i]];
  const double v = x[i];
  double g;
  if (form.kind == IPOW) g = ipow_n(form.n, v);
  else if (form.kind == RIPOW) g = (1.0/ipow_n(form.n, v));
  else if (form.kind == HPOW) g = hpow_n(form.n, v);
  else g = (1.0/hpow_n(form.n, v));
  got[i] = g;
  ref[i] = ocml_pow(v, form.e);
  bool ok = true;
  quick[i] = (form.kind == HPOW || form.kind == RHPOW) ? hpow_checked_n(form.n, v, ok) : 0.0;
  quick_ok[i] = ok;
}

static int value_class(double v) { return v != v ? 0 : std::isinf(v) ? 1 : v == 0.0 ? 2 : 3; }  // NaN, inf, zero, finite
// 2^k as a long double (a literal beyond double's range does not pass the device half of the compilation, where long double is double)
static long double two_to(int k) { return ldexpl(1.0L, k); }
static bool is_normal_ld(long double v) { v = fabsl(v); return v >= 0x1p-1022L && v <= (long double)DBL_MAX; }
static bool same_bits(double a, double b) { return to_bits(a) == to_bits(b) || (a != a && b != b); }

struct PowerStats {
  double worst_ratio = 0.0; size_t judged_normal = 0, judged_other = 0, value_bad = 0;
  size_t class_judged = 0, class_bad = 0, class_boundary = 0;
  size_t quick_accepted = 0, quick_bad = 0, guard_bad = 0;
};

static int run_powers(int log2_random) {
  std::vector<PowForm> forms;
  for (int n = 2; n <= 16; ++n) { forms.push_back({IPOW, n, (double)n}); forms.push_back({RIPOW, n, (double)-n}); }
  for (int n = 3; n <= 31; n += 2) { forms.push_back({HPOW, n, n / 2.0}); forms.push_back({RHPOW, n, -n / 2.0}); }
  forms.push_back({RHPOW, 1, -1 / 2.0});  // the stand-alone x**(-1/2): (1.0/inflx_hpow<1>(x))
  const int F = (int)forms.size();
  // ---- class and sign: every form at every edge argument -------------------------------------------------------------
  std::vector<double> edge = {0.0, INFINITY, NAN, 5e-324, 0x1p-1022, DBL_MAX, 1.0, 2.0, 0.5, 3.0, 1e10, 1e-10, 0x1.fffffffffffffp-1, 0x1.0000000000001p+0, 1e-310, 1e300, 1e-200, 1e200};
  for (int k : {1, 31, 35, 64, 69, 100, 128, 300, 520, 1000, 1022})  // bases whose power overflows / underflows for some of the exponents
    for (double m : {1.0, 1.5}) { edge.push_back(std::ldexp(m, k)); edge.push_back(std::ldexp(m, -k)); }
  { const size_t half = edge.size(); for (size_t i = 0; i < half; ++i) edge.push_back(-edge[i]); }
  std::vector<double> x; std::vector<int> f; std::vector<char> is_edge;
  for (double v : edge) for (int k = 0; k < F; ++k) { x.push_back(v); f.push_back(k); is_edge.push_back(1); }
  const size_t n_edge = x.size();
  // ---- values: random bases over the range of each form in which the result is finite --------------------------------
  // |x|^|e| = 2^t with t uniform: down into the denormals for the plain forms; for the reciprocal forms the chain itself
  // must stay finite (where x^n overflows, 1.0/chain is 0 and pow(x, -n) a denormal: accepted, staging.py MAX_INT_POW)
  const size_t per_kind = (size_t)1 << (log2_random - 1);
  for (int kind = 0; kind < 4; ++kind) {
    std::vector<int> mine;
    for (int k = 0; k < F; ++k) if (forms[k].kind == kind) mine.push_back(k);
    for (size_t i = 0; i < per_kind; ++i) {
      const int k = mine[rnd() % mine.size()];
      const long double ae = fabsl((long double)forms[k].e);
      const bool reciprocal = kind == RIPOW || kind == RHPOW;
      const long double lo = reciprocal ? -1023.0L : -1074.0L, hi = 1023.0L;
      const long double t = lo + (hi - lo) * ((long double)(rnd() >> 11) * 0x1p-53L);
      double v = (double)exp2l(t / ae);
      if (powl((long double)v, ae) >= two_to(1023)) v = next_up(v, -4);
      if ((kind == IPOW || kind == RIPOW) && (rnd() & 1)) v = -v;  // negative bases for the integer powers
      x.push_back(v); f.push_back(k); is_edge.push_back(0);
    }
  }
  const size_t n = x.size();
  // the reference values, once: the same power in long double
  std::vector<long double> want(n), chain(n), inner(n);
  for (size_t i = 0; i < n; ++i) {
    const PowForm& fm = forms[f[i]];
    const long double xl = x[i], ae = fabsl((long double)fm.e);
    chain[i] = powl(xl, ae);                                                    // what the chain (times the root) computes
    inner[i] = (fm.kind == HPOW || fm.kind == RHPOW) ? powl(xl, (fm.n - 1) / 2) : chain[i];  // the integer part of a half power
    want[i] = powl(xl, (long double)fm.e);
  }
  double *d_x, *d_got, *d_ref, *d_quick; int* d_f; PowForm* d_forms; unsigned char* d_ok;
  CK(hipMalloc(&d_x, n * 8)); CK(hipMalloc(&d_got, n * 8)); CK(hipMalloc(&d_ref, n * 8)); CK(hipMalloc(&d_quick, n * 8));
  CK(hipMalloc(&d_f, n * 4)); CK(hipMalloc(&d_forms, F * sizeof(PowForm))); CK(hipMalloc(&d_ok, n));
  CK(hipMemcpy(d_forms, forms.data(), F * sizeof(PowForm), hipMemcpyHostToDevice));
  std::vector<size_t> order(n);
  std::iota(order.begin(), order.end(), (size_t)0);
  std::vector<PowerStats> stats(F);
  size_t printed = 0;
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0) {  // random order: neighbouring lanes evaluate different forms
      for (size_t i = n - 1; i > 0; --i) std::swap(order[i], order[rnd() % (i + 1)]);
    } else {  // sorted by form and argument: wave-uniform
      std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return f[a] != f[b] ? f[a] < f[b] : to_bits(x[a]) < to_bits(x[b]); });
    }
    std::vector<double> hx(n), got(n), ref(n), quick(n); std::vector<int> hf(n); std::vector<unsigned char> qok(n);
    for (size_t j = 0; j < n; ++j) { hx[j] = x[order[j]]; hf[j] = f[order[j]]; }
    CK(hipMemcpy(d_x, hx.data(), n * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_f, hf.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemset(d_got, 0, n * 8)); CK(hipMemset(d_ref, 0, n * 8)); CK(hipMemset(d_quick, 0, n * 8)); CK(hipMemset(d_ok, 0, n));
    power_probe<<<(unsigned)((n + 255) / 256), 256>>>(d_x, d_f, d_forms, n, d_got, d_ref, d_quick, d_ok);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    CK(hipMemcpy(got.data(), d_got, n * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(ref.data(), d_ref, n * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(quick.data(), d_quick, n * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(qok.data(), d_ok, n, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < n; ++j) {
      const size_t i = order[j];
      const PowForm& fm = forms[f[i]];
      PowerStats& s = stats[f[i]];
      const bool reciprocal = fm.kind == RIPOW || fm.kind == RHPOW, half = fm.kind == HPOW || fm.kind == RHPOW;
      const double v = x[i], g = got[j], r = ref[j];
      const long double w = want[i], aw = fabsl(w), ac = fabsl(chain[i]);
      // -- class and sign against OCML's pow, at every argument.  Not judged: results within a factor of four of the smallest
      // denormal or of the overflow threshold, where the two spellings may round to different sides, and the reciprocal
      // forms where the chain overflows while pow(x, -n) still is a denormal (the documented difference, counted).
      const bool at_threshold = (aw > two_to(-1077) && aw < two_to(-1072)) || (aw > two_to(1023) && aw < two_to(1025)) || (ac > two_to(-1077) && ac < two_to(-1072)) || (ac > two_to(1023) && ac < two_to(1025));
      const bool documented = reciprocal && ac >= two_to(1025) && ac < two_to(1077);
      if (w == w && (at_threshold || documented)) {
        ++s.class_boundary;
      } else {
        ++s.class_judged;
        const bool same = value_class(g) == value_class(r) && (g != g || std::signbit(g) == std::signbit(r));
        if (!same) { ++s.class_bad; if (printed++ < 20) printf("  CLASS kind %d n %d: x=%a pow(x, %g)=%a ours=%a\n", fm.kind, fm.n, v, fm.e, r, g); }
      }
      // -- values against powl
      if (w == w && aw <= (long double)DBL_MAX && !(w == 0.0L) && !at_threshold && !documented && std::isfinite(v)) {
        const int steps = fm.kind == IPOW || fm.kind == RIPOW ? fm.n - 1 : (fm.n - 1) / 2 + 1;  // roundings on the way, each <= u relative
        const long double u = 0x1p-53L, allowed = (steps + (reciprocal ? 1 : 0)) * u * (1.0L + 0x1p-10L);
        const long double err = fabsl((long double)g - w);
        const bool normal = is_normal_ld(w) && is_normal_ld(chain[i]) && is_normal_ld(inner[i]) && is_normal_ld((long double)v);
        bool fine;
        if (normal) {
          ++s.judged_normal;
          const double ratio = (double)(err / (allowed * aw));
          s.worst_ratio = std::max(s.worst_ratio, ratio);
          fine = ratio <= 1.0;
        } else {
          ++s.judged_other;
          fine = err <= 1e-10L * aw || err <= fm.n * two_to(-1074);
        }
        if (!fine || g != g) { ++s.value_bad; if (printed++ < 20) printf("  VALUE kind %d n %d: x=%a powl=%La ours=%a (%s)\n", fm.kind, fm.n, v, w, g, normal ? "normal" : "denormal on the way"); }
      }
      // -- the quick variant: refuses zeros, denormals, infinities and NaN; accepts at least the mid range 2^-500 <= |x| <= 2^500
      // (that of the quotients' guards; where between the two its guard ends is its own business); accepted => the bits of inflx_hpow<n>
      if (half) {
        const double av = std::fabs(v);
        const bool must_refuse = !(av >= 0x1p-1022 && av < INFINITY), must_accept = av >= 0x1p-500 && av <= 0x1p500;
        if ((qok[j] && must_refuse) || (!qok[j] && must_accept)) { ++s.guard_bad; if (printed++ < 20) printf("  GUARD n %d: x=%a accepted=%d\n", fm.n, v, (int)qok[j]); }
        if (qok[j]) {
          ++s.quick_accepted;
          const double plain = reciprocal ? 1.0 / quick[j] : quick[j];
          if (!same_bits(plain, g)) { ++s.quick_bad; if (printed++ < 20) printf("  QUICK n %d: x=%a inflx_hpow=%a inflx_hpow_checked=%a\n", fm.n, v, g, plain); }
        }
      }
    }
  }
  size_t bad = 0, accepted = 0, boundary = 0;
  const char* names[4] = {"inflx_ipow<%d>", "1.0/inflx_ipow<%d>", "inflx_hpow<%d>", "1.0/inflx_hpow<%d>"};
  printf("powers: %zu edge and %zu random (argument, form) pairs, each in random order and sorted\n", n_edge, n - n_edge);
  for (int k = 0; k < F; ++k) {
    const PowerStats& s = stats[k];
    char name[40]; snprintf(name, sizeof name, names[forms[k].kind], forms[k].n);
    printf("  %-20s worst ratio to the allowance %.3f over %zu values (%zu more with a denormal on the way), value mismatches %zu; class/sign judged %zu, mismatches %zu, at a threshold %zu",
           name, s.worst_ratio, s.judged_normal, s.judged_other, s.value_bad, s.class_judged, s.class_bad, s.class_boundary);
    if (forms[k].kind >= HPOW) printf("; quick variant accepted %zu, mismatches %zu, guard errors %zu", s.quick_accepted, s.quick_bad, s.guard_bad);
    printf("\n");
    bad += s.value_bad + s.class_bad + s.quick_bad + s.guard_bad + (s.judged_normal == 0);
    accepted += s.quick_accepted; boundary += s.class_boundary;
  }
  printf("powers: %zu mismatches; quick half powers accepted %zu; %zu class comparisons not judged (at a rounding threshold, or 1.0/chain = 0 where pow is a denormal)\n", bad, accepted, boundary);
  if (accepted == 0) ++bad;
  CK(hipFree(d_x)); CK(hipFree(d_got)); CK(hipFree(d_ref)); CK(hipFree(d_quick)); CK(hipFree(d_f)); CK(hipFree(d_forms)); CK(hipFree(d_ok));
  return bad ? 1 : 0;
}

// =====================================================================================================================
// divisions
// =====================================================================================================================
enum { H_HOISTED = 0, H_SHARED = 1, H_INLINE = 2, H_IN_RANGE = 3, N_HELPERS = 4 };
enum { C_PAIRS = 0, C_ACCEPTED = 1, C_MISMATCH = 2, C_WRONGLY_ACCEPTED = 3, N_COUNTS = 4 };
constexpr int N_SETS = 9;
static const char* set_names[N_SETS] = {"random significands, exponents +-32", "all bit patterns", "pairs of special values", "significands next to 1 and 2", "|b| around 2^+-500",
                                        "|a/b| in 2^-402..2^-398", "a*y overflowing", "zero and denormal numerators", "factors around 2^+-160, |b| around 2^+-500"};

__device__ bool irregular(double v) { const double m = __builtin_fabs(v); return !(m >= 0x1p-1022 && m < __builtin_inf()); }  // zero, denormal, infinite, NaN
__device__ bool same_bits_d(double a, double b) { return __double_as_longlong(a) == __double_as_longlong(b) || (a != a && b != b); }
// (mismatches only: the pair and accepted counts are summed per lane first)
__device__ void report(unsigned long long* counts, double* first, int helper, int set, int what, double a, double b, double got, double want) {
  if (atomicAdd(counts + (helper * N_SETS + set) * N_COUNTS + what, 1ull) == 0) {
    double* o = first + ((helper * N_SETS + set) * 2 + (what - C_MISMATCH)) * 4;
    o[0] = a; o[1] = b; o[2] = got; o[3] = want;
  }
}

// lane i divides four numerators a[k * n + i] by b[i] (several numerators per denominator, as D5 has them); all four are of b's operand set
__global__ void division_probe(const double* a_, const double* b_, const unsigned char* set_, size_t n, unsigned long long* counts, double* first) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double b = b_[i];
  const int set = set_[i];
  const double num[4] = {a_[i], a_[n + i], a_[2 * n + i], a_[3 * n + i]};
  const double mb = __builtin_fabs(b);
  const bool b_in_recip_guard = mb >= 0x1p-500 && mb <= 0x1p500;  // inflx_recip: inclusive 2^500
  const bool b_in_shared_guard = mb >= 0x1p-500 && mb < 0x1p501;  // exponent field 523 .. 1523
  const double y = inflx_recip(b);
  bool shared_ok = true;
  const double ys = inflx_shared_reciprocal(b, shared_ok);
  unsigned pairs[N_HELPERS] = {0, 0, 0, 0}, accepted[N_HELPERS] = {0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) {
    const double a = num[k];
    const double want = a / b;
    const bool special = irregular(a) || irregular(b) || irregular(want);
    {  // inflx_div_by_hoisted
      bool ok = true;
      const double q = inflx_div_by_hoisted(a, b, y, ok);
      ++pairs[H_HOISTED];
      if (ok) {
        ++accepted[H_HOISTED];
        if (!same_bits_d(q, want)) report(counts, first, H_HOISTED, set, C_MISMATCH, a, b, q, want);
        if (special || !b_in_recip_guard) report(counts, first, H_HOISTED, set, C_WRONGLY_ACCEPTED, a, b, q, want);
      }
    }
    {  // inflx_shared_reciprocal + inflx_div_by_shared
      bool ok = shared_ok;
      const double q = inflx_div_by_shared(a, b, ys, ok);
      ++pairs[H_SHARED];
      if (ok) {
        ++accepted[H_SHARED];
        if (!same_bits_d(q, want)) report(counts, first, H_SHARED, set, C_MISMATCH, a, b, q, want);
        if (special || !b_in_shared_guard) report(counts, first, H_SHARED, set, C_WRONGLY_ACCEPTED, a, b, q, want);
      }
    }
    {  // inflx_div_by_hoisted_inline: a / b always, whatever the other lanes hold
      const double q = inflx_div_by_hoisted_inline(a, b, y);
      ++pairs[H_INLINE];
      ++accepted[H_INLINE];
      if (!same_bits_d(q, want)) report(counts, first, H_INLINE, set, C_MISMATCH, a, b, q, want);
    }
  }
  // inflx_div_by_hoisted_in_range: numerators that are products of one, two and three factors with clean <160> flags, a denominator
  // with a clean <500> flag -- no comparison at all, the bits of the division
  if (inflx_out_of_range<500>(b) == 0.0) {
    double product = 1.0, flags = 0.0;
    for (int k = 0; k < 3; ++k) {
      flags += inflx_out_of_range<160>(num[k]);
      product = k == 0 ? num[0] : product * num[k];
      ++pairs[H_IN_RANGE];
      if (flags != 0.0) continue;
      const double want = product / b;
      const double q = inflx_div_by_hoisted_in_range(product, b, y);
      ++accepted[H_IN_RANGE];
      if (!same_bits_d(q, want)) report(counts, first, H_IN_RANGE, set, C_MISMATCH, product, b, q, want);
      if (irregular(want) || irregular(product)) report(counts, first, H_IN_RANGE, set, C_WRONGLY_ACCEPTED, product, b, q, want);
    }
  }
  for (int h = 0; h < N_HELPERS; ++h) {
    if (pairs[h]) atomicAdd(counts + (h * N_SETS + set) * N_COUNTS + C_PAIRS, (unsigned long long)pairs[h]);
    if (accepted[h]) atomicAdd(counts + (h * N_SETS + set) * N_COUNTS + C_ACCEPTED, (unsigned long long)accepted[h]);
  }
}

static int run_divisions(int log2_random) {
  std::vector<double> a, b; std::vector<unsigned char> set;
  auto add = [&](int s, double x, double y) { a.push_back(x); b.push_back(y); set.push_back((unsigned char)s); };
  const size_t N = (size_t)1 << log2_random;
  // 0: random significands, moderate exponents (tests/div_hoisted_host.cpp): |q| >= 2^-65, every pair must be accepted
  for (size_t i = 0; i < N; ++i) add(0, random_significand((int)(rnd() % 64) - 32, rnd() & 1), random_significand((int)(rnd() % 64) - 32, rnd() & 1));
  // 1: all bit patterns
  for (size_t i = 0; i < N / 2; ++i) add(1, from_bits(rnd()), from_bits(rnd()));
  // 2: every pair of special values
  const double sp[] = {0.0, -0.0, 1.0, -1.0, INFINITY, -INFINITY, NAN, 5e-324, -5e-324, 2.2250738585072014e-308, DBL_MAX, -DBL_MAX, 1e-310, 3.0, 1.0 / 3.0, 0x1.fffffffffffffp0, 0x1.0000000000001p0, 0x1.fffffffffffffp-1, 0x1p-500, 0x1p500, 0x1p501, 0x1p-400, 0x1p-901, 0x1p1023};
  for (double p : sp) for (double q : sp) add(2, p, q);
  // 3: significands near all-ones and near powers of two
  for (size_t i = 0; i < N / 8; ++i) {
    const uint64_t k = rnd() % 64, l = rnd() % 64;
    const double p = std::ldexp((double)((1ull << 53) - 1 - k), (int)(rnd() % 40) - 20 - 52), q = std::ldexp((double)((1ull << 53) - 1 - l), (int)(rnd() % 40) - 20 - 52), c = std::ldexp((double)((1ull << 52) + k), -52);
    add(3, p, q); add(3, q, p); add(3, p, c); add(3, c, q);
  }
  // 4: |b| at the two guards' ends and one ulp either side, numerators over a wide range
  for (int e : {-501, -500, -499, 499, 500, 501})
    for (int ulp : {-1, 0, 1})
      for (int sign : {1, -1})
        for (int i = 0; i < 512; ++i) {
          const double den = sign * next_up(std::ldexp(1.0, e), ulp);
          add(4, random_significand((int)(rnd() % 64) - 32, rnd() & 1), den);
          add(4, random_significand(e + (int)(rnd() % 64) - 32, rnd() & 1), den);   // quotient of moderate size
          add(4, random_significand((int)(rnd() % 2000) - 1000, rnd() & 1), den);   // anything
        }
  // 5: quotients around the acceptance bound 2^-400
  for (size_t i = 0; i < N / 16; ++i) {
    const int eb = (i & 1) ? (int)(rnd() % 64) - 32 : (int)(rnd() % 900) - 450;
    const double den = random_significand(eb, rnd() & 1);
    add(5, random_significand(eb - 402 + (int)(rnd() % 5), rnd() & 1), den);
  }
  for (int ulp = -2; ulp <= 2; ++ulp) for (double den : {1.0, 3.0, 0x1.fffffffffffffp0, 0x1p100}) add(5, next_up(0x1p-400, ulp) * den, den);
  // 6: a * y overflows while the denominator is inside the guards; quotients next to the overflow threshold
  for (size_t i = 0; i < N / 64; ++i) {
    add(6, random_significand(1020 + (int)(rnd() % 4), rnd() & 1), random_significand(-500 + (int)(rnd() % 4), rnd() & 1));
    add(6, random_significand(1023, rnd() & 1), random_significand(-1 + (int)(rnd() % 3), rnd() & 1));
    add(6, next_up(DBL_MAX, -(int)(rnd() % 8)), next_up(1.0, -(int)(rnd() % 8) - 1));
    // a / b = 2^1024 (or an ulp or two less): a * y may round to a finite q0 while the quotient rounds to infinity, and the last
    // step then overflows -- the reason for the upper end of the acceptance test
    const double den = random_significand(-1, rnd() & 1);
    add(6, next_up(std::ldexp(den, 1024), -(int)(rnd() % 3)), den);  // (|den| < 1: the numerator is finite)
  }
  // 7: zero and denormal numerators
  for (size_t i = 0; i < N / 64; ++i) {
    const double den = random_significand((i & 1) ? (int)(rnd() % 64) - 32 : (int)(rnd() % 1000) - 500, rnd() & 1);
    add(7, (i % 8 == 0) ? ((rnd() & 1) ? 0.0 : -0.0) : from_bits((rnd() & 0x8000000000000000ull) | ((rnd() & 0x000FFFFFFFFFFFFFull) >> (rnd() % 52))), den);
  }
  // 8: factors over the whole range the <160> flag admits (its ends and one ulp outside included), denominators over that of the <500> flag
  for (size_t i = 0; i < N / 4; ++i) {
    const unsigned r = (unsigned)(rnd() % 16);
    const int ea = r == 0 ? 160 : r == 1 ? -160 : r == 2 ? 159 : (int)(rnd() % 321) - 160;
    const int eb = (rnd() % 4 == 0) ? ((rnd() & 1) ? 499 : -500) : (int)(rnd() % 1001) - 500;
    double p = ea == 160 ? std::ldexp(1.0, 160) : random_significand(ea, rnd() & 1);
    if (r == 3) p = next_up(0x1p160, 1);
    if (r == 4) p = next_up(0x1p-160, -1);
    add(8, p, (rnd() % 8 == 0) ? std::ldexp(1.0, eb >= 0 ? eb + 1 : eb) : random_significand(eb, rnd() & 1));
  }
  const size_t n = a.size();
  // three more numerators per denominator: those of the next pairs of the same set
  std::vector<std::vector<size_t>> members(N_SETS);
  for (size_t i = 0; i < n; ++i) members[set[i]].push_back(i);
  std::vector<double> more(3 * n);
  for (const auto& m : members)
    for (size_t j = 0; j < m.size(); ++j)
      for (int k = 1; k < 4; ++k) more[(k - 1) * n + m[j]] = a[m[(j + k) % m.size()]];
  double *d_a, *d_b, *d_first; unsigned char* d_set; unsigned long long* d_counts;
  const size_t n_counts = N_HELPERS * N_SETS * N_COUNTS, n_first = N_HELPERS * N_SETS * 2 * 4;
  CK(hipMalloc(&d_a, 4 * n * 8)); CK(hipMalloc(&d_b, n * 8)); CK(hipMalloc(&d_set, n)); CK(hipMalloc(&d_counts, n_counts * 8)); CK(hipMalloc(&d_first, n_first * 8));
  std::vector<size_t> order(n);
  std::iota(order.begin(), order.end(), (size_t)0);
  std::vector<unsigned long long> total(n_counts, 0);
  size_t bad = 0;
  const char* helper_names[N_HELPERS] = {"inflx_div_by_hoisted", "inflx_div_by_shared", "inflx_div_by_hoisted_inline", "inflx_div_by_hoisted_in_range"};
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0) {  // random order: every wavefront mixes regular and irregular pairs
      for (size_t i = n - 1; i > 0; --i) std::swap(order[i], order[rnd() % (i + 1)]);
    } else {  // sorted by operand class: wavefronts whose lanes are all regular, or all irregular (the ballot branch of the inline quotient)
      std::vector<int> key(n);
      for (size_t i = 0; i < n; ++i) {
        const double q = a[i] / b[i], m = std::fabs(b[i]);
        const bool regular = std::isnormal(a[i]) && std::isnormal(q) && std::fabs(q) >= 0x1p-400 && m >= 0x1p-500 && m <= 0x1p500;
        key[i] = (regular ? 0 : 1 + value_class(q)) * 16 + set[i];
      }
      std::stable_sort(order.begin(), order.end(), [&](size_t p, size_t q) { return key[p] < key[q]; });
    }
    std::vector<double> ha(4 * n), hb(n); std::vector<unsigned char> hs(n);
    for (size_t j = 0; j < n; ++j) {
      ha[j] = a[order[j]]; hb[j] = b[order[j]]; hs[j] = set[order[j]];
      for (int k = 1; k < 4; ++k) ha[k * n + j] = more[(k - 1) * n + order[j]];
    }
    CK(hipMemcpy(d_a, ha.data(), 4 * n * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_b, hb.data(), n * 8, hipMemcpyHostToDevice)); CK(hipMemcpy(d_set, hs.data(), n, hipMemcpyHostToDevice));
    CK(hipMemset(d_counts, 0, n_counts * 8)); CK(hipMemset(d_first, 0, n_first * 8));
    division_probe<<<(unsigned)((n + 255) / 256), 256>>>(d_a, d_b, d_set, n, d_counts, d_first);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    std::vector<unsigned long long> counts(n_counts); std::vector<double> first(n_first);
    CK(hipMemcpy(counts.data(), d_counts, n_counts * 8, hipMemcpyDeviceToHost)); CK(hipMemcpy(first.data(), d_first, n_first * 8, hipMemcpyDeviceToHost));
    for (int h = 0; h < N_HELPERS; ++h)
      for (int s = 0; s < N_SETS; ++s) {
        const unsigned long long* c = &counts[(h * N_SETS + s) * N_COUNTS];
        for (int w = 0; w < N_COUNTS; ++w) total[(h * N_SETS + s) * N_COUNTS + w] += c[w];
        for (int w = C_MISMATCH; w <= C_WRONGLY_ACCEPTED; ++w)
          if (c[w]) {
            const double* o = &first[((h * N_SETS + s) * 2 + (w - C_MISMATCH)) * 4];
            printf("  %s, %s, %s order: %llu %s, first a=%a b=%a got=%a a/b=%a\n", helper_names[h], set_names[s], pass ? "sorted" : "random", c[w], w == C_MISMATCH ? "MISMATCHES" : "WRONGLY ACCEPTED", o[0], o[1], o[2], o[3]);
            bad += c[w];
          }
        // a condition, not a measurement: |q| >= 2^-65 in the +-32 set, so every pair of it is accepted
        if (s == 0 && h != H_IN_RANGE && c[C_ACCEPTED] != c[C_PAIRS]) { printf("  %s: %llu pairs of the +-32 set not accepted (%s order)\n", helper_names[h], c[C_PAIRS] - c[C_ACCEPTED], pass ? "sorted" : "random"); ++bad; }
      }
  }
  printf("divisions: %zu operand pairs, four numerators per denominator, each in random order and sorted by operand class\n", n);
  for (int h = 0; h < N_HELPERS; ++h) {
    unsigned long long pairs = 0, accepted = 0, mism = 0, wrong = 0;
    for (int s = 0; s < N_SETS; ++s) {
      const unsigned long long* c = &total[(h * N_SETS + s) * N_COUNTS];
      pairs += c[C_PAIRS]; accepted += c[C_ACCEPTED]; mism += c[C_MISMATCH]; wrong += c[C_WRONGLY_ACCEPTED];
      printf("  %-30s %-45s quotients %10llu accepted %10llu mismatches %llu wrongly accepted %llu\n", helper_names[h], set_names[s], c[C_PAIRS], c[C_ACCEPTED], c[C_MISMATCH], c[C_WRONGLY_ACCEPTED]);
    }
    printf("  %-30s %-45s quotients %10llu accepted %10llu mismatches %llu wrongly accepted %llu\n", helper_names[h], "all sets", pairs, accepted, mism, wrong);
    if (accepted == 0) ++bad;
  }
  printf("divisions: %zu mismatches\n", bad);
  CK(hipFree(d_a)); CK(hipFree(d_b)); CK(hipFree(d_set)); CK(hipFree(d_counts)); CK(hipFree(d_first));
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  const int log2_random = argc > 1 ? atoi(argv[1]) : 20;
  if (log2_random < 8 || log2_random > 24) { printf("usage: device_math_probe [log2 of the random operands per helper, 8..24]\n"); return 2; }
  const int powers = run_powers(log2_random);
  const int divisions = run_divisions(log2_random);
  printf("device_math_probe: %s\n", (powers || divisions) ? "FAILED" : "ok");
  return (powers || divisions) ? 1 : 0;
}
