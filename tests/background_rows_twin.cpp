// The row transpose on the CPU (csrc/inflx_background_rows.h): every thread of every workgroup of a launch through the load phase,
// then every thread through the store phase -- what inflx_bg_rows_transpose does around its __syncthreads() --, on heap blocks of
// exactly the sizes the kernel is promised, so that an AddressSanitizer build sees any access outside them; and the plan of a
// call's lane passes, with the lanes of a pass whose buffer holds whole lanes (csrc/inflx_background_passes.h).  Built and run by
// tests/test_background_rows.py.  Exit status 0: every check passed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "inflx_background_passes.h"
#include "inflx_background_rows.h"

namespace {

int g_failures = 0;
#define CHECK(cond, ...)                     \
  do {                                       \
    if (!(cond)) {                           \
      if (++g_failures <= 20) {              \
        std::fprintf(stderr, "FAILED %s: ", #cond); \
        std::fprintf(stderr, __VA_ARGS__);   \
        std::fprintf(stderr, "\n");          \
      }                                      \
    }                                        \
  } while (0)

constexpr uint64_t kSentinel = UINT64_C(0xDEADBEEFCAFEF00D);

uint64_t bits_of(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof b);
  return b;
}
double from_bits(uint64_t b) {
  double v;
  std::memcpy(&v, &b, sizeof v);
  return v;
}

// element i of the source: distinct values, among them NaNs with a payload and -0.0 (only one element is -0.0: i = 5)
uint64_t source_bits(uint64_t i) {
  if (i % 11 == 3) return UINT64_C(0x7FF8000000000000) | (i + 1);  // quiet NaN, payload i + 1
  if (i % 13 == 6) return UINT64_C(0xFFF4000000000000) | (i + 1);  // a signalling pattern with the sign set
  if (i == 5) return UINT64_C(0x8000000000000000);                  // -0.0
  return bits_of(1.0 + (double)i);
}

// one launch: n lanes, `filled` slots holding rows row_base.., into arrays of (n + 4) trajectories x rows_total rows at lane_off
void run_launch(uint64_t n, uint64_t filled, bool want_y, bool want_t) {
  const uint64_t rows_total = filled + 5, row_base = 3, lane_off = 2, lanes_out = n + 4;
  const size_t n_src = (size_t)(filled * 7 * n), n_y = (size_t)(lanes_out * rows_total * 6), n_t = (size_t)(lanes_out * rows_total);
  double* src = static_cast<double*>(std::malloc(n_src * sizeof(double)));
  double* out_y = static_cast<double*>(std::malloc(n_y * sizeof(double)));
  double* out_t = static_cast<double*>(std::malloc(n_t * sizeof(double)));
  double* tile = static_cast<double*>(std::malloc(INFLX_BG_ROWS_TILE_DOUBLES * sizeof(double)));
  if (!src || !out_y || !out_t || !tile) std::abort();
  for (size_t i = 0; i < n_src; ++i) src[i] = from_bits(source_bits(i));
  for (size_t i = 0; i < n_y; ++i) out_y[i] = from_bits(kSentinel);
  for (size_t i = 0; i < n_t; ++i) out_t[i] = from_bits(kSentinel);

  InflxBgRowsArgs a;
  std::memset(&a, 0, sizeof a);
  a.rows = src;
  a.out_y = want_y ? out_y : nullptr;
  a.out_t = want_t ? out_t : nullptr;
  a.n = n;
  a.lane_off = lane_off;
  a.rows_total = rows_total;
  a.row_base = row_base;
  a.filled = filled;
  const uint64_t blocks = inflx_bg_rows_blocks(n, filled);
  CHECK(blocks == ((n + 63) / 64) * ((filled + 7) / 8), "blocks %llu", (unsigned long long)blocks);
  for (uint64_t b = 0; b < blocks; ++b) {
    for (size_t i = 0; i < INFLX_BG_ROWS_TILE_DOUBLES; ++i) tile[i] = from_bits(kSentinel);  // (LDS is not cleared between workgroups)
    for (unsigned th = 0; th < INFLX_BG_ROWS_THREADS; ++th) inflx_bg_rows_load(a, b, th, tile);
    for (unsigned th = 0; th < INFLX_BG_ROWS_THREADS; ++th) inflx_bg_rows_store(a, b, th, tile);
  }

  // every destination element: the source bits inside the window, the sentinel outside
  for (uint64_t traj = 0; traj < lanes_out; ++traj)
    for (uint64_t row = 0; row < rows_total; ++row) {
      const bool inside = traj >= lane_off && traj < lane_off + n && row >= row_base && row < row_base + filled;
      const uint64_t lane = traj - lane_off, slot = row - row_base;
      for (unsigned c = 0; c < 7; ++c) {
        const uint64_t got = bits_of(c < 6 ? out_y[(traj * rows_total + row) * 6 + c] : out_t[traj * rows_total + row]);
        const bool written = inside && (c < 6 ? want_y : want_t);
        const uint64_t want = written ? source_bits((slot * 7 + c) * n + lane) : kSentinel;
        CHECK(got == want, "n %llu filled %llu: trajectory %llu row %llu component %u holds %016llx, expected %016llx", (unsigned long long)n,
              (unsigned long long)filled, (unsigned long long)traj, (unsigned long long)row, c, (unsigned long long)got, (unsigned long long)want);
      }
    }
  std::free(tile);
  std::free(out_t);
  std::free(out_y);
  std::free(src);
}

void check_plan(size_t B, size_t rows, bool force, bool transposed, size_t lanes) {
  const InflxBgRowsPlan p = inflx_bg_rows_plan(B, rows, force);
  CHECK(p.transposed == transposed && p.lanes_per_pass == lanes, "plan(B %zu, rows %zu, force %d) = {%zu lanes, transposed %d}, expected {%zu, %d}", B, rows,
        (int)force, p.lanes_per_pass, (int)p.transposed, lanes, (int)transposed);
}

void check_lanes(size_t B, size_t bytes_per_lane, size_t threads, size_t lanes) {
  const size_t got = inflx_bg_lanes_per_pass(B, bytes_per_lane, threads);
  CHECK(got == lanes, "lanes_per_pass(B %zu, %zu bytes per lane, %zu threads) = %zu, expected %zu", B, bytes_per_lane, threads, got, lanes);
}

}  // namespace

int main() {
  static_assert(INFLX_BG_ROWS_TILE_LANES == 64 && INFLX_BG_ROWS_THREADS == 256, "a wavefront reads one segment of 64 lanes");
  static_assert(INFLX_BG_ROWS_PITCH_Y % 2 == 1 && INFLX_BG_ROWS_PITCH_T % 2 == 1, "odd pitches: see the banking rule in the header");
  const uint64_t tr = INFLX_BG_ROWS_TILE_ROWS;
  const uint64_t lanes[] = {1, 63, 64, 65, 257}, slots[] = {1, tr - 1, tr, tr + 1, 2 * tr + 3};
  unsigned launches = 0;
  for (uint64_t n : lanes)
    for (uint64_t filled : slots) {
      run_launch(n, filled, true, true);
      ++launches;
    }
  // one output only: the other array is not touched
  run_launch(65, tr + 1, true, false);
  run_launch(65, tr + 1, false, true);

  const size_t M = size_t(1) << 20;
  check_plan(size_t(1) << 17, 256, false, true, size_t(1) << 17);  // one pass
  check_plan(M + 3, 3, false, true, M);                            // passes of 2^20 and 3 lanes
  check_plan(M, 60, false, true, 639132);                          // floor(2 GiB / (60 x 56 B))
  check_plan(8, 2340, false, true, 8);
  check_plan(8, 2341, false, false, 8);
  check_plan(1, 1, false, true, 1);
  check_plan(size_t(1) << 17, 256, true, false, size_t(1) << 17);  // with the flag: scatter, today's chunks
  check_plan(M + 3, 3, true, false, M);
  check_plan(1, 1, true, false, 1);
  check_plan(8, 2341, true, false, 8);
  {  // the passes of 2^20 + 3 lanes
    const InflxBgRowsPlan p = inflx_bg_rows_plan(M + 3, 3, false);
    std::vector<size_t> passes;
    for (size_t c0 = 0; c0 < M + 3; c0 += p.lanes_per_pass) passes.push_back(p.lanes_per_pass < M + 3 - c0 ? p.lanes_per_pass : M + 3 - c0);
    CHECK(passes.size() == 2 && passes[0] == M && passes[1] == 3, "%zu passes", passes.size());
  }
  // a device-resident result has no staging array: nothing but the lane chunk bounds a pass, whatever the rows
  {
    const InflxBgRowsPlan p = inflx_bg_rows_plan(M + 3, 5000, false, true);
    CHECK(p.transposed && p.lanes_per_pass == M, "device plan {%zu, %d}", p.lanes_per_pass, (int)p.transposed);
  }
  // a staged pass fits 2 GiB
  for (size_t rows : {size_t(1), size_t(60), size_t(256), size_t(2340)}) {
    const InflxBgRowsPlan p = inflx_bg_rows_plan(M, rows, false);
    CHECK(p.transposed && p.lanes_per_pass * rows * 56 <= (size_t(2) << 30), "rows %zu: %zu lanes", rows, p.lanes_per_pass);
  }
  // the lanes of a pass whose 256 MiB buffer holds `bytes_per_lane` of every lane: whole workgroups where more than one fits
  const size_t big = 10000000;
  check_lanes(65541, 4096, 256, 65536);                // S = 64 samples of 8 doubles: two passes
  check_lanes(big, 5120, 256, 52224);                  // floor(2^28 / 5120) = 52 428, whole workgroups
  check_lanes(big, size_t(1) << 29, 256, 1);           // a lane larger than the buffer: one at a time
  check_lanes(big, 894784, 256, 256);                  // quotient 300
  check_lanes(big, 1342177, 256, 200);                 // quotient 200, below one workgroup: not rounded
  check_lanes(5, 4096, 256, 5);                        // no more than the call has
  check_lanes(M + 257, 176, 256, M);                   // no more than kBgMaxLanes
  if (g_failures) {
    std::fprintf(stderr, "%d checks failed\n", g_failures);
    return 1;
  }
  std::printf("ok: %u launches, tile %u x %u, LDS %zu bytes\n", launches + 2, (unsigned)INFLX_BG_ROWS_TILE_LANES, (unsigned)INFLX_BG_ROWS_TILE_ROWS,
              (size_t)INFLX_BG_ROWS_TILE_DOUBLES * sizeof(double));
  return 0;
}
