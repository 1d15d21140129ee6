// The counter-based N(0,1) field of the tile-level degradation: a pure function of (seed, channel, row, column) of the
// full-size HR image, so a tile's noise does not depend on which tile is cut, on the batch, or on the launch.
//
//   words   = Philox4x32-10(counter = (column >> 2, row, channel, 0), key = (seed, 0))          [Salmon et al., SC'11]
//   u_i     = (float(words[i] >> 8) + 0.5f) * 2^-24      in fp32; the sum is exact below 2^23 and rounds to even above
//                                                         (a 25-bit value), so u lies in (0, 1] and is never 0
//   pair p  = (u_{2p}, u_{2p+1}),  p = 0, 1:   radius = sqrtf(-2 logf(u_{2p})),  angle = 2 pi u_{2p+1}
//   pixel (channel, row, column) takes normal number m = column & 3 of the call:  m = 0: radius_0 cos(angle_0),
//   m = 1: radius_0 sin(angle_0),  m = 2: radius_1 cos(angle_1),  m = 3: radius_1 sin(angle_1)
//
// i.e. words 0, 1 feed the columns 4q and 4q + 1, words 2, 3 the columns 4q + 2 and 4q + 3.  logf / cosf / sinf are the
// precise library functions (degrade.normal_field_host states the same map in numpy, normals in float64).  This map is part
// of the interface (include/sisr_hip.h): a seeded run depends on it.
#pragma once
#include "sisr_common.h"

__host__ __device__ __forceinline__ void sisr_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                            unsigned k1, unsigned* out) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out[3] = c3;
}

__host__ __device__ __forceinline__ float sisr_word_to_uniform(unsigned word) {
  return ((float)(word >> 8) + 0.5f) * 5.9604644775390625e-8f;  // 2^-24
}

// the N(0,1) value of pixel (channel, row, column) under `seed`
__device__ __forceinline__ float sisr_normal_at(unsigned seed, int channel, int row, int column) {
  unsigned w[4];
  sisr_philox4x32_10((unsigned)column >> 2, (unsigned)row, (unsigned)channel, 0u, seed, 0u, w);
  const int pair = (column >> 1) & 1;
  const float ua = sisr_word_to_uniform(pair ? w[2] : w[0]), ub = sisr_word_to_uniform(pair ? w[3] : w[1]);
  const float radius = sqrtf(-2.0f * logf(ua)), angle = 6.283185307179586f * ub;
  return radius * ((column & 1) ? sinf(angle) : cosf(angle));
}
