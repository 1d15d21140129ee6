// JPEG degradation on the device: the pixels PIL returns for
//   image.save(buf, "JPEG", subsampling=0, quality=q);  PIL.Image.open(buf)        ref: Code/data_converter.py (jpeg_compress)
// without the file in between.  With 4:4:4 sampling the round trip is libjpeg's integer arithmetic per 8 x 8 block --
// jccolor (RGB -> YCbCr), jfdctint (forward DCT, "islow"), jcdctmgr (quantise), jdcoefct (dequantise), jidctint (inverse
// DCT), jdcolor (YCbCr -> RGB) -- and the entropy coder in the middle is lossless, so it is left out.  Everything is
// int32 with arithmetic right shifts; the products stay below 2^31 (degrade.jpeg_roundtrip_host checks that against an
// int64 run of itself).
//
// One launch, no workspace, no state.  A lane owns one row of one 8 x 8 block for all components: it loads its 8 pixels
// per plane with clamped indices (the edge replication of libjpeg's padding to whole blocks) and converts the colours in
// registers.  Forward pass 1 runs along that row; a transpose through LDS gives the lane a column, on which forward
// pass 2, the quantiser, the dequantiser and inverse pass 1 all work; a second transpose gives it its row back for
// inverse pass 2 and the colour conversion out.  Two exchanges per component, each within the 8 lanes of a block.
#include "sisr_common.h"

#define JP_THREADS 256                 // 32 blocks of 8 x 8 per workgroup
#define JP_BLOCKS (JP_THREADS / 8)
#define JP_LD 9                        // LDS row pitch of a block's 8 x 8 tile, in words

struct JpegTables {  // the two scaled quantisation tables in natural (row-major) order, passed by value
  unsigned short q[2][64];
};

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

template <int C, bool TO_FLOAT>
__global__ __launch_bounds__(JP_THREADS) void jpeg_roundtrip_kernel(const unsigned char* __restrict__ in, void* __restrict__ outp,
                                                                    int H, int W, int nbx, int nblocks, JpegTables tab) {
  __shared__ int tiles[JP_BLOCKS * 8 * JP_LD];
  __shared__ int qt[2][64];
  if (threadIdx.x < 128) qt[threadIdx.x >> 6][threadIdx.x & 63] = tab.q[threadIdx.x >> 6][threadIdx.x & 63];
  __syncthreads();
  const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
  int g = blockIdx.x * JP_BLOCKS + lb;
  const bool live = g < nblocks;
  if (!live) g = nblocks - 1;  // lanes past the last block keep the barriers company and store nothing
  const int by = g / nbx, bx = g - by * nbx;
  const int y = by * 8 + r, x0 = bx * 8;
  const long plane = (long)H * W;
  const long row = (long)min(y, H - 1) * W;
  int* tile = tiles + lb * 8 * JP_LD;

  int p[C][8];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) p[c][j] = in[c * plane + row + min(x0 + j, W - 1)];

  constexpr int CB = C == 3 ? 1 : 0, CR = C == 3 ? 2 : 0;
  if (C == 3) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // jccolor.c
      const int R = p[0][j], G = p[CB][j], B = p[CR][j];
      p[0][j] = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
      p[CB][j] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
      p[CR][j] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) jp_component(p[c], tile, qt[c ? 1 : 0], r);
  if (C == 3) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {  // jdcolor.c
      const int Y = p[0][j], cb = p[CB][j] - 128, cr = p[CR][j] - 128;
      p[0][j] = jp_clamp8(Y + ((91881 * cr + 32768) >> 16));
      p[CB][j] = jp_clamp8(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
      p[CR][j] = jp_clamp8(Y + ((116130 * cb + 32768) >> 16));
    }
  }

  if (!live || y >= H) return;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (x0 + j >= W) continue;
      const long at = c * plane + (long)y * W + x0 + j;
      if (TO_FLOAT) static_cast<float*>(outp)[at] = (float)p[c][j] / 255.0f;  // ToTensor: .float().div(255)
      else static_cast<unsigned char*>(outp)[at] = (unsigned char)p[c][j];
    }
}

// jcparam.c: the Annex-K tables scaled by the quality (jpeg_quality_scaling, jpeg_add_quant_table with force_baseline)
static const unsigned char JP_BASE[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,
     14, 17, 22, 29, 51,  87,  80,  62,  18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

extern "C" int sisr_jpeg_roundtrip(const unsigned char* in, void* out, int C, int H, int W, int quality, int to_float,
                                   void* stream) {
  if (!in || !out || (C != 1 && C != 3) || H < 1 || W < 1 || quality < 1 || quality > 100 || (to_float != 0 && to_float != 1))
    return SISR_ERR_ARG;
  const long nbx = (W + 7L) / 8, nby = (H + 7L) / 8;
  if (nbx * nby > 0x7fffffffL) return SISR_ERR_UNSUPPORTED;
  const int nblocks = (int)(nbx * nby);
  JpegTables tab;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = (JP_BASE[t][i] * scale + 50) / 100;
      tab.q[t][i] = (unsigned short)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
  const dim3 grid((unsigned)((nblocks + JP_BLOCKS - 1) / JP_BLOCKS)), block(JP_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (C == 3) {
    if (to_float) hipLaunchKernelGGL((jpeg_roundtrip_kernel<3, true>), grid, block, 0, st, in, out, H, W, (int)nbx, nblocks, tab);
    else hipLaunchKernelGGL((jpeg_roundtrip_kernel<3, false>), grid, block, 0, st, in, out, H, W, (int)nbx, nblocks, tab);
  } else {
    if (to_float) hipLaunchKernelGGL((jpeg_roundtrip_kernel<1, true>), grid, block, 0, st, in, out, H, W, (int)nbx, nblocks, tab);
    else hipLaunchKernelGGL((jpeg_roundtrip_kernel<1, false>), grid, block, 0, st, in, out, H, W, (int)nbx, nblocks, tab);
  }
  return sisr_check_launch();
}
