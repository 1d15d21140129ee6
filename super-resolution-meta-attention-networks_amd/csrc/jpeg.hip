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
#include "jpeg_block.h"

struct JpegTables {  // the two scaled quantisation tables in natural (row-major) order, passed by value
  unsigned short q[2][64];
};

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
  if (C == 3) jp_rgb_to_ycc(p[0], p[CB], p[CR]);
#pragma unroll
  for (int c = 0; c < C; ++c) jp_component(p[c], tile, qt[c ? 1 : 0], r);
  if (C == 3) jp_ycc_to_rgb(p[0], p[CB], p[CR]);

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

extern "C" int sisr_jpeg_roundtrip(const unsigned char* in, void* out, int C, int H, int W, int quality, int to_float,
                                   void* stream) {
  if (!in || !out || (C != 1 && C != 3) || H < 1 || W < 1 || quality < 1 || quality > 100 || (to_float != 0 && to_float != 1))
    return SISR_ERR_ARG;
  const long nbx = (W + 7L) / 8, nby = (H + 7L) / 8;
  if (nbx * nby > 0x7fffffffL) return SISR_ERR_UNSUPPORTED;
  const int nblocks = (int)(nbx * nby);
  JpegTables tab;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) tab.q[t][i] = (unsigned short)jp_scaled_entry(t, i, quality);
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
