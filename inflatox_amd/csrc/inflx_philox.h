// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), a counter-based generator: four
// 32-bit words from a 128-bit counter and a 64-bit key, ten rounds.  No state: a word depends on (counter, key) alone, so a lane
// draws what it needs from where it is (csrc/inflx_stochastic.h) and nothing has to be carried, skipped or seeded per thread.
//     round:   (hi0, lo0) = M0 * c0,  (hi1, lo1) = M1 * c2;   c <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
//     between rounds:  k0 += W0,  k1 += W1
// with the multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57 and the Weyl constants W0 = 0x9E3779B9, W1 = 0xBB67AE85.
//
// INFLX_FN code in plain C++ (a 32 x 32 -> 64 bit product is v_mul_lo_u32 + v_mul_hi_u32 on the device), so that
// tests/stochastic_twin.cpp compiles the very same generator for the host.
#pragma once
#include <stdint.h>

#define INFLX_PHILOX_M0 0xD2511F53u
#define INFLX_PHILOX_M1 0xCD9E8D57u
#define INFLX_PHILOX_W0 0x9E3779B9u
#define INFLX_PHILOX_W1 0xBB67AE85u

// out[0..3] = Philox4x32-10 of the counter c[0..3] under the key (k0, k1)
INFLX_FN void inflx_philox4x32_10(const uint32_t* c, uint32_t k0, uint32_t k1, uint32_t* out) {
  uint32_t c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)INFLX_PHILOX_M0 * c0, p1 = (uint64_t)INFLX_PHILOX_M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += INFLX_PHILOX_W0;
    k1 += INFLX_PHILOX_W1;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

// u in (0, 1) from two words: the 52 bits (hi, top 20 bits of lo) plus one half, times 2^-52 -- exact in binary64, never 0 and never 1
INFLX_FN double inflx_philox_uniform(uint32_t hi, uint32_t lo) {
  const uint64_t k = ((uint64_t)hi << 20) | (uint64_t)(lo >> 12);
  return ((double)k + 0.5) * 0x1p-52;
}

// Two independent standard normals of one Philox call (Box-Muller): the key is the 64-bit seed, the counter (step lo, step hi, r,
// stream) -- the lane's accepted-step index, its realisation and its point's stream id.
INFLX_FN void inflx_philox_normals(uint64_t seed, uint64_t step, uint32_t r, uint32_t stream, double* xi) {
  const uint32_t c[4] = {(uint32_t)step, (uint32_t)(step >> 32), r, stream};
  uint32_t w[4];
  inflx_philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  const double u1 = inflx_philox_uniform(w[0], w[1]), u2 = inflx_philox_uniform(w[2], w[3]);
  const double two_pi = 6.283185307179586476925286766559;
  const double rad = sqrt(-2.0 * log(u1)), ang = two_pi * u2;
  xi[0] = rad * cos(ang);
  xi[1] = rad * sin(ang);
}
