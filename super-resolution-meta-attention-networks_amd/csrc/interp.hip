// The evaluator's bicubic pre-up-sampling of a low-resolution batch on the device: the reference's
//   pil    = ToPILImage(lr[i])  = uint8(lr * 255)                     ref: evaluation/standard_eval.py:149 (`mul(255).byte()`: truncation)
//   up     = pil.resize((w * s, h * s), PIL.Image.BICUBIC)            ref: standard_eval.py:152
//   rgb    = ToTensor(up) = float(up) / 255                           ref: standard_eval.py:155
//   ycbcr  = rgb_to_ycbcr(rgb, 'jpg')                                 ref: standard_eval.py:160-164 (_high_res_prep)
// as ONE launch over the batch.  A workgroup owns a 32 x 32 output tile of all three channels: it quantises the input rows
// and columns the tile reads into LDS, runs PIL's horizontal pass into LDS (only the rows the tile's vertical taps touch),
// runs the vertical pass from there, and writes the RGB and / or YCbCr planes -- nothing intermediate goes to memory, and the
// colour conversion sees its three channels in registers.  Both passes are libImaging/Resample.c's 8-bit fixed-point
// arithmetic (22 fractional bits, rounding constant 1 << 21, clip to [0, 255] after EACH pass) on the host tables of
// degrade.pil_bicubic_table, as in degrade.hip, so `rgb` is bit-identical to PIL's result.  The colour conversion rounds
// every product and every sum on its own, in the order metrics.rgb_to_ycbcr_jpg writes them (no fma), so `ycbcr` is
// bit-identical to that function on a float32 image.
#include "pil_upsample.h"  // the block-level resampler, shared with interp_tiles.hip

// lr [B][C][h][w] fp32 -> rgb and / or ycbcr [B][C][H][W] fp32 (ycbcr: C == 3).  grid (W / 32, H / 32, B * ceil(C / 3)).
// VEC: W % 4 == 0 and 16-byte aligned outputs -- every lane stores its four pixels of a row as one 16-byte word.
template <bool VEC>
__global__ __launch_bounds__(256) void pil_upsample_kernel(const float* __restrict__ lr, float* __restrict__ rgb,
                                                           float* __restrict__ ycbcr, const int* __restrict__ bounds_h,
                                                           const int* __restrict__ coef_h, const int* __restrict__ bounds_v,
                                                           const int* __restrict__ coef_v, int C, int h, int w, int H, int W) {
  // (+ KS: a zero-weight tap past an output's own taps may read up to KS - 1 bytes / rows beyond the tile)
  __shared__ unsigned char in_t[UC * UH * UH + KS];  // [c][r][q]: the quantised input the tile reads
  __shared__ unsigned tmp_t[UC * UH + KS][UT / 4];   // [c * UH + r][x / 4]: its horizontally resampled rows, four pixels to a word
  __shared__ int kh[UT][KS], kv[UT][KS];             // (5 words a row: rows start on different LDS banks)
  __shared__ int fh[UT], fv[UT];
  const int groups = (C + UC - 1) / UC;
  const int b = blockIdx.z / groups, c0 = (blockIdx.z - b * groups) * UC;
  const int cn = C - c0 < UC ? C - c0 : UC;
  const int x0 = blockIdx.x * UT, y0 = blockIdx.y * UT;
  const int tw = W - x0 < UT ? W - x0 : UT, th = H - y0 < UT ? H - y0 : UT;
  int clo, nc, rlo, nr;
  tile_extent(bounds_h, x0, tw, w, clo, nc);
  tile_extent(bounds_v, y0, th, h, rlo, nr);
  stage_table(bounds_h, coef_h, x0, tw, clo, nc, fh, kh);
  stage_table(bounds_v, coef_v, y0, th, rlo, nr, fv, kv);
  // ToPILImage: byte(v * 255), truncating
  const float rcp_nc = 1.0f / (float)nc;
  const float* src = lr + (((long)b * C + c0) * h + rlo) * w + clo;
  for (int c = 0; c < cn; ++c)
    for (int i = threadIdx.x; i < nr * nc; i += 256) {
      const int r = small_div(i, rcp_nc), q = i - r * nc;
      in_t[(c * UH + r) * UH + q] = (unsigned char)(int)(src[((long)c * h + r) * w + q] * 255.0f);
    }
  __syncthreads();
  pil_pass_h(in_t, tmp_t, fh, kh, cn, nr);
  __syncthreads();
  // vertical pass: a lane owns four neighbouring pixels of one output row, in every channel
  const int y = threadIdx.x / (UT / 4), q = threadIdx.x % (UT / 4);
  if (y >= th || 4 * q >= tw) return;
  const int lo = fv[y];
  int cf[KS];
  for (int k = 0; k < KS; ++k) cf[k] = kv[y][k];
  float px[UC][4];
  pil_pass_v(tmp_t, lo, cf, q, cn, px);
  const long plane = (long)H * W;
  const long at = ((long)b * C + c0) * plane + (long)(y0 + y) * W + x0 + 4 * q;
  auto put = [&](float* __restrict__ dst, int c, const float* v) {
    float* p = dst + at + c * plane;
    if (VEC) {
      *reinterpret_cast<f32x4*>(p) = (f32x4){v[0], v[1], v[2], v[3]};
    } else {
      for (int j = 0; j < 4; ++j)
        if (4 * q + j < tw) p[j] = v[j];
    }
  };
  if (rgb)
    for (int c = 0; c < cn; ++c) put(rgb, c, px[c]);
  if (ycbcr) {
    float yy[4], cb[4], cr[4];
    for (int j = 0; j < 4; ++j) ycbcr_jpg(px[0][j], px[1][j], px[2][j], yy[j], cb[j], cr[j]);
    put(ycbcr, 0, yy);
    put(ycbcr, 1, cb);
    put(ycbcr, 2, cr);
  }
}

// lr [B][C][h][w] -> rgb / ycbcr [B][C][H][W] (each nullable, not both), H = s h and W = s w for an integer s >= 1; the
// tables are device copies of pil_bicubic_table(w, W) and (h, H), whose ksize is 5 at every such scale.  No workspace: the
// intermediate lives in LDS.
extern "C" int sisr_pil_upsample(const float* lr, float* rgb, float* ycbcr, const int* bounds_h, const int* coef_h,
                                 const int* bounds_v, const int* coef_v, int ksize, int B, int C, int h, int w, int H, int W,
                                 void* stream) {
  if (!lr || (!rgb && !ycbcr) || !bounds_h || !coef_h || !bounds_v || !coef_v || ksize <= 0 || B <= 0 || C <= 0 || h <= 0 ||
      w <= 0 || H <= 0 || W <= 0)
    return SISR_ERR_ARG;
  if (H % h || W % w || H / h != W / w) return SISR_ERR_UNSUPPORTED;  // one integer scale for both sides
  if (ksize != KS) return SISR_ERR_UNSUPPORTED;
  if (ycbcr && C != 3) return SISR_ERR_UNSUPPORTED;
  const long gz = (long)B * ((C + UC - 1) / UC);
  const dim3 grid((W + UT - 1) / UT, (H + UT - 1) / UT, (unsigned)gz);
  if (grid.y > 65535 || gz > 65535) return SISR_ERR_UNSUPPORTED;
  const bool vec = W % 4 == 0 && (!rgb || sisr_aligned16(rgb)) && (!ycbcr || sisr_aligned16(ycbcr));
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL((pil_upsample_kernel<true>), grid, dim3(256), 0, st, lr, rgb, ycbcr, bounds_h, coef_h, bounds_v, coef_v,
                       C, h, w, H, W);
  else
    hipLaunchKernelGGL((pil_upsample_kernel<false>), grid, dim3(256), 0, st, lr, rgb, ycbcr, bounds_h, coef_h, bounds_v, coef_v,
                       C, h, w, H, W);
  return sisr_check_launch();
}
