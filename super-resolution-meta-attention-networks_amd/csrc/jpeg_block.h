// The 8 x 8 block arithmetic of the JPEG round trip (libjpeg: jfdctint, jcdctmgr, jdcoefct, jidctint, jccolor, jdcolor and
// jcparam's quality scaling), shared by the single-image kernel (jpeg.hip) and the batched tile kernel (degrade_tiles.hip).
// A lane owns one row of one block; see jpeg.hip for the scheme.
#pragma once
#include "sisr_common.h"

#define JP_THREADS 256                 // 32 blocks of 8 x 8 per workgroup
#define JP_BLOCKS (JP_THREADS / 8)
#define JP_LD 9                        // LDS row pitch of a block's 8 x 8 tile, in words

#define JP_FIX_0_298631336 2446
#define JP_FIX_0_390180644 3196
#define JP_FIX_0_541196100 4433
#define JP_FIX_0_765366865 6270
#define JP_FIX_0_899976223 7373
#define JP_FIX_1_175875602 9633
#define JP_FIX_1_501321110 12299
#define JP_FIX_1_847759065 15137
#define JP_FIX_1_961570560 16069
#define JP_FIX_2_053119869 16819
#define JP_FIX_2_562915447 20995
#define JP_FIX_3_072711026 25172

__device__ __forceinline__ int jp_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }
__device__ __forceinline__ int jp_clamp8(int v) { return min(max(v, 0), 255); }

// jfdctint.c, one 1-D pass over d[0..7] in place.  PASS2 = false: along a row (outputs scaled up by 2^2); true: along a column.
template <bool PASS2>
__device__ __forceinline__ void jp_fdct8(int* d) {
  const int n = PASS2 ? 15 : 11;
  const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = PASS2 ? jp_descale(t10 + t11, 2) : (t10 + t11) << 2;
  d[4] = PASS2 ? jp_descale(t10 - t11, 2) : (t10 - t11) << 2;
  int z1 = (t12 + t13) * JP_FIX_0_541196100;
  d[2] = jp_descale(z1 + t13 * JP_FIX_0_765366865, n);
  d[6] = jp_descale(z1 - t12 * JP_FIX_1_847759065, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * JP_FIX_1_175875602;
  const int a4 = t4 * JP_FIX_0_298631336, a5 = t5 * JP_FIX_2_053119869, a6 = t6 * JP_FIX_3_072711026,
            a7 = t7 * JP_FIX_1_501321110;
  z1 *= -JP_FIX_0_899976223;
  z2 *= -JP_FIX_2_562915447;
  z3 = -z3 * JP_FIX_1_961570560 + z5;
  z4 = -z4 * JP_FIX_0_390180644 + z5;
  d[7] = jp_descale(a4 + z1 + z3, n);
  d[5] = jp_descale(a5 + z2 + z4, n);
  d[3] = jp_descale(a6 + z2 + z3, n);
  d[1] = jp_descale(a7 + z1 + z4, n);
}

// jidctint.c, one 1-D pass over c[0..7] in place.  PASS2 = false: along a column (n = 11); true: along a row (n = 18).
template <bool PASS2>
__device__ __forceinline__ void jp_idct8(int* c) {
  const int n = PASS2 ? 18 : 11;
  int z1 = (c[2] + c[6]) * JP_FIX_0_541196100;
  int t2 = z1 - c[6] * JP_FIX_1_847759065, t3 = z1 + c[2] * JP_FIX_0_765366865;
  int t0 = (c[0] + c[4]) << 13, t1 = (c[0] - c[4]) << 13;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  t0 = c[7];
  t1 = c[5];
  t2 = c[3];
  t3 = c[1];
  z1 = t0 + t3;
  int z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const int z5 = (z3 + z4) * JP_FIX_1_175875602;
  t0 *= JP_FIX_0_298631336;
  t1 *= JP_FIX_2_053119869;
  t2 *= JP_FIX_3_072711026;
  t3 *= JP_FIX_1_501321110;
  z1 *= -JP_FIX_0_899976223;
  z2 *= -JP_FIX_2_562915447;
  z3 = -z3 * JP_FIX_1_961570560 + z5;
  z4 = -z4 * JP_FIX_0_390180644 + z5;
  t0 += z1 + z3;
  t1 += z2 + z4;
  t2 += z2 + z3;
  t3 += z1 + z4;
  c[0] = jp_descale(t10 + t3, n);
  c[7] = jp_descale(t10 - t3, n);
  c[1] = jp_descale(t11 + t2, n);
  c[6] = jp_descale(t11 - t2, n);
  c[2] = jp_descale(t12 + t1, n);
  c[5] = jp_descale(t12 - t1, n);
  c[3] = jp_descale(t13 + t0, n);
  c[4] = jp_descale(t13 - t0, n);
}

// One component of one block: v[0..7] = the lane's row of samples (0..255) in, the decoded row (0..255) out.
// tile: the block's 8 x JP_LD words of LDS; qt: 64 table entries in LDS; r: the lane's row, then its column.
__device__ __forceinline__ void jp_component(int* v, int* tile, const int* qt, int r) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] -= 128;
  jp_fdct8<false>(v);
#pragma unroll
  for (int j = 0; j < 8; ++j) tile[r * JP_LD + j] = v[j];
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = tile[i * JP_LD + r];  // column r, top to bottom
  jp_fdct8<true>(v);
#pragma unroll
  for (int i = 0; i < 8; ++i) {  // jcdctmgr: divide by 8 Q rounding half away from zero; jdcoefct: times Q
    const int q = qt[i * 8 + r], d = q << 3;
    const int a = (abs(v[i]) + (d >> 1)) / d;
    v[i] = (v[i] < 0 ? -a : a) * q;
  }
  jp_idct8<false>(v);
  __syncthreads();  // every lane of the block has read its column
#pragma unroll
  for (int i = 0; i < 8; ++i) tile[i * JP_LD + r] = v[i];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = tile[r * JP_LD + j];
  jp_idct8<true>(v);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = jp_clamp8(v[j] + 128);
  __syncthreads();  // the tile is free for the next component
}

// jccolor.c / jdcolor.c on the lane's 8 pixels of the three planes, in place
__device__ __forceinline__ void jp_rgb_to_ycc(int* p0, int* p1, int* p2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int R = p0[j], G = p1[j], B = p2[j];
    p0[j] = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
    p1[j] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
    p2[j] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
  }
}
__device__ __forceinline__ void jp_ycc_to_rgb(int* p0, int* p1, int* p2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int Y = p0[j], cb = p1[j] - 128, cr = p2[j] - 128;
    p0[j] = jp_clamp8(Y + ((91881 * cr + 32768) >> 16));
    p1[j] = jp_clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    p2[j] = jp_clamp8(Y + ((116130 * cb + 32768) >> 16));
  }
}

// jcparam.c: the Annex-K tables and their scaling by the quality (jpeg_quality_scaling, jpeg_add_quant_table with
// force_baseline); t = 0 luminance, 1 chrominance, natural (row-major) order
__host__ __device__ __forceinline__ int jp_base_entry(int t, int i) {
  constexpr unsigned char base[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

  return base[t][i];
}
// one entry of the table scaled for `quality` (1..100)
__host__ __device__ __forceinline__ int jp_scaled_entry(int t, int i, int quality) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  const int v = (jp_base_entry(t, i) * scale + 50) / 100;
  return v < 1 ? 1 : (v > 255 ? 255 : v);
}
