// Pillow's 8-bit bicubic up-sampling of a 32 x 32 output block held in LDS, shared by the whole-image kernel (interp.hip) and
// the tile kernel (interp_tiles.hip): both must give the same bytes for the same output pixel, so the staging of the
// coefficient tables, the two fixed-point passes, ToTensor's division and the colour conversion live here once.
#pragma once
#include "sisr_common.h"

#define UT 32  // output tile edge
#define UH 40  // most input rows / columns one tile reads: 32 / s + 5 <= 37 for every integer scale s >= 1
#define KS 5   // taps per output: bicubic up-sampling has ksize = 5 at every scale
#define UC 3   // channels per workgroup

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// i / d for 0 <= i < 2^13 and 0 < d <= 64 without an integer division: (i + 0.5) / d is at least 1 / 128 away from
// every integer, the fp32 product at most 2^-10
__device__ __forceinline__ int small_div(int i, float rcp_d) { return (int)(((float)i + 0.5f) * rcp_d); }

// first input index and count of the inputs that outputs [o0, o0 + n) read.  The table's windows move monotonically, so the
// first and the last output give the range; it is clamped to the image and to the LDS tile, which changes nothing for a
// table of pil_bicubic_table and keeps every access in bounds for any other.
__device__ __forceinline__ void tile_extent(const int* __restrict__ bounds, int o0, int n, int in_size, int& lo, int& cnt) {
  lo = clampi(bounds[2 * o0], 0, in_size - 1);
  const int last = o0 + n - 1;
  const int hi = clampi(bounds[2 * last] + bounds[2 * last + 1], lo + 1, in_size);
  cnt = hi - lo < UH ? hi - lo : UH;
}

// first taps (relative to the tile's first input) and coefficients of a tile's UT outputs -> LDS.  Every output gets KS
// taps: those past its own count, and all taps of outputs past the image edge, have coefficient 0, so the passes below run
// without a tap count (what such a tap reads is some byte of the tile's LDS arrays, which are padded for it).
__device__ __forceinline__ void stage_table(const int* __restrict__ bounds, const int* __restrict__ coef, int o0, int n, int lo0,
                                            int cnt, int* first, int (*k)[KS]) {
  for (int i = threadIdx.x; i < UT * KS; i += 256) {
    const int o = i / KS, t = i - o * KS;
    k[o][t] = (o < n && t < bounds[2 * (o0 + o) + 1]) ? coef[(long)(o0 + o) * KS + t] : 0;
  }
  for (int o = threadIdx.x; o < UT; o += 256) first[o] = o < n ? clampi(bounds[2 * (o0 + o)] - lo0, 0, cnt - 1) : 0;
}

__device__ __forceinline__ int clip8(int ss) {
  const int v = ss >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The horizontal pass packs four clipped bytes into a word.  Left alone, hipcc fuses `shift, clamp to a byte, pack two` into
// v_ashr_pk_u8_i32 and takes the upper half of that instruction's result for zero; on gfx950 it was not, and bytes 2 and 3 of
// every packed word came out wrong (ROCm 7.2; found by the bit-for-bit tests).  An empty asm statement between the clamp and
// the packing keeps the two apart.
__device__ __forceinline__ int keep_apart(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(v));
#endif
  return v;
}

// ToTensor's k / 255 for a byte k, correctly rounded as the fp32 division is: the quotient by the rounded reciprocal, then
// one Newton step on the exact remainder (two fmas).  Equal to the division for all 256 bytes (checked exhaustively in
// exact arithmetic; tests/test_interp_gpu.py sends every byte through it).  The division itself costs ~3x as much, and the
// kernel is bound by its instruction count, not by its stores.
__device__ __forceinline__ float byte_over_255(int k) {
  const float x = (float)k, rc = 0x1.010102p-8f;  // fp32(1 / 255)
  const float q = x * rc;
  return __builtin_fmaf(__builtin_fmaf(-q, 255.0f, x), rc, q);
}

// metrics.rgb_to_ycbcr_jpg on a float32 image: every product and every sum rounded to fp32 on its own, in the order that
// function writes them.  Contraction is switched off for the block: hipcc fuses a * b + c into an fma by default (also
// through __fmul_rn / __fadd_rn, which are plain operators in this toolchain), and an fma moves the last bit.
__device__ __forceinline__ void ycbcr_jpg(float R, float G, float B, float& y, float& cb, float& cr) {
#pragma clang fp contract(off)
  const float bias = (float)(128.0 * (1.0 / 255));
  y = (0.299f * R + 0.587f * G) + 0.114f * B;
  cb = bias + ((-0.168736f * R - 0.331264f * G) + 0.5f * B);
  cr = bias + ((0.5f * R - 0.418688f * G) - 0.081312f * B);
}

// Horizontal pass over the nr input rows a block's vertical taps read, four neighbouring outputs to a lane: in_t [c][r][q]
// bytes (row pitch UH) -> tmp_t [c * UH + r][x / 4], four pixels to a word.  |coef| <= 2^22 and the inputs are bytes: 24-bit
// multiplies.  All 256 threads of the workgroup call it, between two barriers.
__device__ __forceinline__ void pil_pass_h(const unsigned char* in_t, unsigned (*tmp_t)[UT / 4], const int* fh, const int (*kh)[KS],
                                           int cn, int nr) {
  for (int i = threadIdx.x; i < cn * nr * (UT / 4); i += 256) {
    const int n8 = nr * (UT / 4);
    const int c = (i >= n8) + (i >= 2 * n8), t = i - c * n8;
    const int r = t / (UT / 4), q = t % (UT / 4);
    const unsigned char* row = in_t + (c * UH + r) * UH;
    unsigned word = 0;
    for (int j = 0; j < 4; ++j) {
      const int x = 4 * q + j, lo = fh[x];
      int ss = 1 << 21;
      for (int k = 0; k < KS; ++k) ss += __mul24((int)row[lo + k], kh[x][k]);
      word |= (unsigned)keep_apart(clip8(ss)) << (8 * j);
    }
    tmp_t[c * UH + r][q] = word;
  }
}

// Vertical pass for the four neighbouring pixels 4 q .. 4 q + 3 of the output row whose first tap is row `lo` of tmp_t and
// whose coefficients are cf, in every channel (channels past cn come out as the rounding constant's byte, 0), followed by
// ToTensor's division.
__device__ __forceinline__ void pil_pass_v(const unsigned (*tmp_t)[UT / 4], int lo, const int* cf, int q, int cn, float (&px)[UC][4]) {
  for (int c = 0; c < UC; ++c) {
    int ss[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
    if (c < cn) {
      for (int k = 0; k < KS; ++k) {
        const unsigned word = tmp_t[c * UH + lo + k][q];
        for (int j = 0; j < 4; ++j) ss[j] += __mul24((int)((word >> (8 * j)) & 255u), cf[k]);
      }
    }
    for (int j = 0; j < 4; ++j) px[c][j] = byte_over_255(clip8(ss[j]));  // ToTensor: .float().div(255)
  }
}
