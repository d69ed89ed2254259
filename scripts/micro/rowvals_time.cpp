// What the per-row evaluation of the row-broadcast path costs, and what that time is made of: inflx_sweep_rowvals_complete of a
// core object, or inflx_rowpass_complete of a row-pass object (`<tag>.rp<hash>.hsaco`, csrc/inflx_rowpass_kernels.hip).
//
//   hipcc -O2 -I inflatox_amd/csrc scripts/micro/rowvals_time.cpp -o scripts/micro/rowvals_time.bin
//   scripts/micro/rowvals_time.bin LABEL CODE_OBJECT ROWS [p0 p1 ...]
//
// CODE_OBJECT is a model's core object or row-pass object (inflatox_amd/_jit_cache/...).  A core object knows one shape only: 64
// threads, one slice, parameters behind the pointer.  For every launch shape (threads per workgroup 64 / 256, write slices = grid.z, parameters behind a device
// pointer / in the kernel arguments) three figures, HIP event pairs on one stream, microseconds:
//   warm  -- 200 launches back to back between one pair of events: code and table lines resident, launch overhead overlapped
//   lone  -- one launch on an idle stream between a pair of events, median of 41: what a lone call waits for
//   cold  -- the same launch behind a 1 GiB fill of other memory on the same stream (what the store stream of the sweep
//            before it leaves of the caches), median of 21
// One line per shape on stdout.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "inflx_rowpass_abi.h"

#define CK(x)                                                                                \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) {                                                                  \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));      \
      return 1;                                                                              \
    }                                                                                        \
  } while (0)

static float median(std::vector<float> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: %s LABEL CODE_OBJECT ROWS [parameters ...]\n", argv[0]);
    return 2;
  }
  const char* label = argv[1];
  const size_t rows = strtoull(argv[3], nullptr, 10);
  std::vector<double> par;
  for (int k = 4; k < argc; ++k) par.push_back(atof(argv[k]));
  if (rows == 0 || rows > (1u << 20) || par.empty() || par.size() > INFLX_INLINE_PARAMS) {
    fprintf(stderr, "rows in [1, 2^20], 1 to %d parameters\n", INFLX_INLINE_PARAMS);
    return 2;
  }
  hipModule_t mod;
  hipFunction_t f;
  CK(hipModuleLoad(&mod, argv[2]));
  const bool old_abi = hipModuleGetFunction(&f, mod, "inflx_rowpass_complete") != hipSuccess;  // a core object
  if (old_abi) {
    (void)hipGetLastError();
    CK(hipModuleGetFunction(&f, mod, "inflx_sweep_rowvals_complete"));
  }
  hipStream_t s;
  CK(hipStreamCreate(&s));
  const unsigned replicas = 32;
  double *table = nullptr, *d_par = nullptr;
  char* filler = nullptr;
  const size_t table_bytes = rows * replicas * 64, fill_bytes = size_t(1) << 30;
  CK(hipMalloc(reinterpret_cast<void**>(&table), table_bytes));
  CK(hipMalloc(reinterpret_cast<void**>(&d_par), par.size() * sizeof(double)));
  CK(hipMalloc(reinterpret_cast<void**>(&filler), fill_bytes));
  CK(hipMemcpy(d_par, par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));

  InflxRowPassArgs ra;  // (a core object's kernel reads the InflxSweepArgs at its head)
  memset(&ra, 0, sizeof ra);
  InflxSweepArgs& a = ra.a;
  a.x0a = -1.0;
  a.dx0 = 2.0 / (double)rows;
  a.x1a = 0.0;
  a.dx1 = 1.0;
  a.N1 = rows;
  a.row_count = rows;
  a.P = 1;
  a.col_chunks = 1;
  a.row_table = table;
  a.table_replicas = replicas;
  a.stream_planes = 6;
  for (size_t k = 0; k < par.size(); ++k) ra.params_inline[k] = par[k];
  void* params[] = {&ra};
  const unsigned gx = (unsigned)((rows + 63) / 64);

  struct Shape { unsigned block, slices; int inline_params; };
  const Shape shapes[] = {{64, 1, 0}, {256, 1, 0}, {256, 1, 1}, {256, 2, 1}, {256, 4, 1}, {256, 8, 1}, {256, 16, 1}};
  for (const Shape& sh : shapes) {
    {
      if (old_abi && (sh.block != 64 || sh.slices != 1 || sh.inline_params)) continue;
      const unsigned block = sh.block;
      const int inline_params = sh.inline_params;
      a.params = inline_params ? nullptr : d_par;
      auto launch = [&] { return hipModuleLaunchKernel(f, gx, 1, sh.slices, block, 1, 1, 0, s, params, nullptr); };
      for (int k = 0; k < 5; ++k) CK(launch());
      CK(hipStreamSynchronize(s));
      float ms = 0.f;
      const int reps = 200;
      CK(hipEventRecord(e0, s));
      for (int k = 0; k < reps; ++k) CK(launch());
      CK(hipEventRecord(e1, s));
      CK(hipEventSynchronize(e1));
      CK(hipEventElapsedTime(&ms, e0, e1));
      const float warm = ms / reps * 1e3f;
      std::vector<float> lone, cold;
      for (int k = 0; k < 41; ++k) {
        CK(hipStreamSynchronize(s));
        CK(hipEventRecord(e0, s));
        CK(launch());
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        lone.push_back(ms * 1e3f);
      }
      for (int k = 0; k < 21; ++k) {
        CK(hipMemsetAsync(filler, k, fill_bytes, s));
        CK(hipEventRecord(e0, s));
        CK(launch());
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        cold.push_back(ms * 1e3f);
      }
      printf("%-14s rows %zu  block %3u  slices %2u  params %-7s  warm %6.2f us  lone %6.2f us (min %6.2f)  cold %6.2f us (min %6.2f)\n", label, rows, block, sh.slices,
             inline_params ? "inline" : "pointer", warm, median(lone), *std::min_element(lone.begin(), lone.end()), median(cold),
             *std::min_element(cold.begin(), cold.end()));
      fflush(stdout);
    }
  }
  // an empty event pair: what the two records themselves contribute to `lone`
  std::vector<float> empty;
  for (int k = 0; k < 41; ++k) {
    float ms = 0.f;
    CK(hipStreamSynchronize(s));
    CK(hipEventRecord(e0, s));
    CK(hipEventRecord(e1, s));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    empty.push_back(ms * 1e3f);
  }
  printf("%-14s empty event pair %6.2f us\n", label, median(empty));
  CK(hipFree(table));
  CK(hipFree(d_par));
  CK(hipFree(filler));
  CK(hipModuleUnload(mod));
  return 0;
}
