// TEST INFRASTRUCTURE: csrc/inflx_sf.h on the device, the counterpart of tests/sf_host.cpp.  A stand-alone program built with
// the kernels' own compiler flags (tests/test_special_edges_gpu.py).  usage: sf_probe CASES
// CASES (written by tests/special_cases.py's table): the number of cases, then one line per case,
//     function  integer-order  p0 p1 p2  x  group        (doubles as 16 hex digits of their bit pattern)
// Every group is one kernel launch, one lane per case, and runs twice: in table order (waves mostly uniform in function and
// branch) and in a fixed shuffled order (every wave mixes functions and branches through the noinline calls).  After each
// launch the status word INFLX_SF_STATUS is read, cleared and read again.  Output:
//     R index bits-in-table-order bits-shuffled
//     S group status next-read status-shuffled next-read-shuffled
//     DIFFERENCES n
// exit status 1 when the two passes differ in any bit, 2 on a HIP error or a malformed case file.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "inflx_device_math.h"
#include "inflx_sf.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

struct ProbeCase {
  int fn, n;
  double p[3], x;
};
enum { JN, YN, IN, KN, JL, YL, JNU, YNU, INU, KNU, F01, F11, F21, F20, N_FUNCTIONS };

__global__ void sf_probe(const ProbeCase* cases, int n, unsigned long long* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ProbeCase c = cases[i];
  double v = 0.0;
  switch (c.fn) {
    case JN: v = inflx_sf_bessel_Jn(c.n, c.x); break;
    case YN: v = inflx_sf_bessel_Yn(c.n, c.x); break;
    case IN: v = inflx_sf_bessel_In(c.n, c.x); break;
    case KN: v = inflx_sf_bessel_Kn(c.n, c.x); break;
    case JL: v = inflx_sf_bessel_jl(c.n, c.x); break;
    case YL: v = inflx_sf_bessel_yl(c.n, c.x); break;
    case JNU: v = inflx_sf_bessel_Jnu(c.p[0], c.x); break;
    case YNU: v = inflx_sf_bessel_Ynu(c.p[0], c.x); break;
    case INU: v = inflx_sf_bessel_Inu(c.p[0], c.x); break;
    case KNU: v = inflx_sf_bessel_Knu(c.p[0], c.x); break;
    case F01: v = inflx_sf_hyperg_0F1(c.p[0], c.x); break;
    case F11: v = inflx_sf_hyperg_1F1(c.p[0], c.p[1], c.x); break;
    case F21: v = inflx_sf_hyperg_2F1(c.p[0], c.p[1], c.p[2], c.x); break;
    case F20: v = inflx_sf_hyperg_2F0(c.p[0], c.p[1], c.x); break;
  }
  out[i] = (unsigned long long)__double_as_longlong(v);
}

static double from_bits(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }

int main(int argc, char** argv) {
  if (argc != 2) { printf("usage: sf_probe CASES\n"); return 2; }
  FILE* f = fopen(argv[1], "r");
  if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
  int n_cases = 0;
  if (fscanf(f, "%d", &n_cases) != 1 || n_cases < 1 || n_cases > (1 << 20)) { printf("malformed case file\n"); return 2; }
  std::vector<ProbeCase> cases(n_cases);
  std::vector<int> group(n_cases);
  int n_groups = 0;
  for (int i = 0; i < n_cases; ++i) {
    unsigned long long b[4];
    ProbeCase& c = cases[i];
    if (fscanf(f, "%d %d %llx %llx %llx %llx %d", &c.fn, &c.n, &b[0], &b[1], &b[2], &b[3], &group[i]) != 7 || c.fn < 0 || c.fn >= N_FUNCTIONS || group[i] < 0 || group[i] >= n_cases) {
      printf("malformed case %d\n", i);
      return 2;
    }
    for (int k = 0; k < 3; ++k) c.p[k] = from_bits(b[k]);
    c.x = from_bits(b[3]);
    n_groups = std::max(n_groups, group[i] + 1);
  }
  fclose(f);
  std::vector<std::vector<int>> members(n_groups);
  for (int i = 0; i < n_cases; ++i) members[group[i]].push_back(i);
  size_t largest = 1;
  for (const auto& m : members) largest = std::max(largest, m.size());
  ProbeCase* d_cases;
  unsigned long long* d_out;
  CK(hipMalloc(&d_cases, largest * sizeof(ProbeCase)));
  CK(hipMalloc(&d_out, largest * 8));
  std::vector<unsigned long long> bits[2] = {std::vector<unsigned long long>(n_cases, 0), std::vector<unsigned long long>(n_cases, 0)};
  std::vector<unsigned> status[2] = {std::vector<unsigned>(2 * n_groups, 0), std::vector<unsigned>(2 * n_groups, 0)};
  const unsigned zero = 0u;
  for (int g = 0; g < n_groups; ++g) {
    std::vector<int> order = members[g];
    const int n = (int)order.size();
    if (n == 0) continue;
    for (int pass = 0; pass < 2; ++pass) {
      if (pass == 1)
        for (int i = n - 1; i > 0; --i) std::swap(order[i], order[rnd() % (uint64_t)(i + 1)]);
      std::vector<ProbeCase> h(n);
      std::vector<unsigned long long> got(n);
      for (int j = 0; j < n; ++j) h[j] = cases[order[j]];
      CK(hipMemcpy(d_cases, h.data(), n * sizeof(ProbeCase), hipMemcpyHostToDevice));
      CK(hipMemset(d_out, 0, n * 8));
      CK(hipMemcpyToSymbol(HIP_SYMBOL(INFLX_SF_STATUS), &zero, sizeof zero));
      sf_probe<<<(n + 63) / 64, 64>>>(d_cases, n, d_out);
      CK(hipGetLastError());
      CK(hipDeviceSynchronize());
      CK(hipMemcpy(got.data(), d_out, n * 8, hipMemcpyDeviceToHost));
      for (int j = 0; j < n; ++j) bits[pass][order[j]] = got[j];
      unsigned word = 0u;
      CK(hipMemcpyFromSymbol(&word, HIP_SYMBOL(INFLX_SF_STATUS), sizeof word));
      status[pass][2 * g] = word;
      CK(hipMemcpyToSymbol(HIP_SYMBOL(INFLX_SF_STATUS), &zero, sizeof zero));
      CK(hipMemcpyFromSymbol(&word, HIP_SYMBOL(INFLX_SF_STATUS), sizeof word));
      status[pass][2 * g + 1] = word;
    }
  }
  CK(hipFree(d_cases));
  CK(hipFree(d_out));
  size_t differences = 0;
  for (int i = 0; i < n_cases; ++i) {
    printf("R %d %016llx %016llx\n", i, bits[0][i], bits[1][i]);
    differences += bits[0][i] != bits[1][i];
  }
  for (int g = 0; g < n_groups; ++g) {
    printf("S %d %u %u %u %u\n", g, status[0][2 * g], status[0][2 * g + 1], status[1][2 * g], status[1][2 * g + 1]);
    differences += status[0][2 * g] != status[1][2 * g] || status[0][2 * g + 1] != status[1][2 * g + 1];
  }
  printf("DIFFERENCES %zu\n", differences);
  return differences ? 1 : 0;
}
