// The pieces of the perceptual (VGG19 feature) loss that are not convolutions, DESIGN.md 6n
// (ref: sr_tools/loss_functions.py:6-22 PerceptualMechanism, feature_extractors/VGGNets.py:118-131 VGGFeatureExtractor):
//   sisr_vgg_prep_fwd        planar RGB image -> ImageNet-normalised channels-last map, channels >= 3 zero
//   sisr_vgg_prep_bwd        that map's gradient -> the planar image gradient
//   sisr_maxpool2_fwd        MaxPool2d(2, 2) on a channels-last map
//   sisr_maxpool2_relu_bwd   the pool's input gradient with the derivative of the ReLU in front of the pool, one pass
// All four are streams.  In the pool kernels and the normalisation's forward a lane owns four neighbouring channels of one
// pixel (16 bytes) and neighbouring lanes own neighbouring quads, so a wave reads and writes whole 256-byte runs of a pixel's
// channels.  sisr_vgg_prep_bwd is the exception: it wants the first quad of every pixel only, so a lane's read stands cp
// floats from its neighbour's (16 bytes used of each 256-byte run at cp = 64); only its stores are dense.  It moves one
// quad per pixel of the image, once a step (0.06 ms at 8 x 3 x 512^2).  Nothing is accumulated: no atomics, no LDS.
//
// Arithmetic.  The normalisation is the reference's `(img - mean) / std` on fp32 tensors: one IEEE subtraction, then one
// correctly rounded IEEE division (hipcc's default; contraction is switched off so that neither is merged with a
// neighbour).  The pool takes the maximum in torch's scan order -- (dh, dw) = (0,0), (0,1), (1,0), (1,1), a later element
// wins only where it is greater (or NaN) -- and its backward hands the gradient to the FIRST maximum of a window.
#include "sisr_common.h"

// the scan step of torch's max_pool2d: `v` replaces the running maximum `m` (and takes the index) iff v > m or v is NaN
__device__ __forceinline__ void pool_step(float v, int k, float& m, int& arg) {
  if (v > m || v != v) {
    m = v;
    arg = k;
  }
}

// out[b][h][w][0..2] = (img[b][c][h][w] - mean[c]) / std[c], out[b][h][w][3..cp-1] = 0.  One thread per float4 of the output.
__global__ __launch_bounds__(256) void vgg_prep_fwd_kernel(const float* __restrict__ img, const float* __restrict__ mean3,
                                                           const float* __restrict__ std3, float* __restrict__ out, long hw,
                                                           int cp, long total4) {
#pragma clang fp contract(off)
  const int c4n = cp >> 2;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    const long pix = i / c4n;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (i - pix * c4n == 0) {
      const long b = pix / hw, p = pix - b * hw;
      const float* src = img + b * 3 * hw + p;
      v.x = (src[0] - mean3[0]) / std3[0];
      v.y = (src[hw] - mean3[1]) / std3[1];
      v.z = (src[2 * hw] - mean3[2]) / std3[2];
    }
    reinterpret_cast<f32x4*>(out)[i] = v;
  }
}

// dimg[b][c][h][w] = gmap[b][h][w][c] / std[c], c < 3.  One thread per pixel: it reads the pixel's first quad (a strided
// read: neighbouring lanes are cp floats apart) and writes one word to each of the three planes (dense: neighbouring lanes,
// neighbouring words of a plane).
__global__ __launch_bounds__(256) void vgg_prep_bwd_kernel(const float* __restrict__ gmap, const float* __restrict__ std3,
                                                           float* __restrict__ dimg, long hw, int cp, long pixels) {
  const float s0 = std3[0], s1 = std3[1], s2 = std3[2];
  for (long pix = (long)blockIdx.x * 256 + threadIdx.x; pix < pixels; pix += (long)gridDim.x * 256) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(gmap + pix * cp);
    const long b = pix / hw, p = pix - b * hw;
    float* dst = dimg + b * 3 * hw + p;
    dst[0] = g.x / s0;
    dst[hw] = g.y / s1;
    dst[2 * hw] = g.z / s2;
  }
}

// out[b][oh][ow][c] = max over the 2 x 2 window at (2 oh, 2 ow).  One thread per float4 of the output.
__global__ __launch_bounds__(256) void maxpool2_fwd_kernel(const float* __restrict__ y, float* __restrict__ out, int H, int W,
                                                           int C, long total4) {
  const int c4n = C >> 2, Ho = H >> 1, Wo = W >> 1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    long t = i / c4n;
    const int c4 = (int)(i - t * c4n);
    const int ow = (int)(t % Wo);
    t /= Wo;
    const int oh = (int)(t % Ho);
    const long b = t / Ho;
    const float* src = y + (((b * H + 2 * oh) * W + 2 * ow) * C + 4 * c4);
    const f32x4 v00 = *reinterpret_cast<const f32x4*>(src);
    const f32x4 v01 = *reinterpret_cast<const f32x4*>(src + C);
    const f32x4 v10 = *reinterpret_cast<const f32x4*>(src + (long)W * C);
    const f32x4 v11 = *reinterpret_cast<const f32x4*>(src + (long)W * C + C);
    f32x4 m = v00;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int arg = 0;
      float me = m[e];
      pool_step(v01[e], 1, me, arg);
      pool_step(v10[e], 2, me, arg);
      pool_step(v11[e], 3, me, arg);
      m[e] = me;
    }
    reinterpret_cast<f32x4*>(out)[i] = m;
  }
}

// dy[b][h][w][c] = dout[b][h / 2][w / 2][c] where (h, w) holds the first maximum of its window and y there is > 0, else 0;
// the odd last row / column that no window covers gets 0.  Gather form: one thread per float4 of the INPUT map re-reads its
// window (each element of y is read by the four lanes of its window, out of the cache) and writes its own quad once.
__global__ __launch_bounds__(256) void maxpool2_relu_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dout,
                                                                float* __restrict__ dy, int H, int W, int C, long total4) {
  const int c4n = C >> 2, Ho = H >> 1, Wo = W >> 1;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total4; i += (long)gridDim.x * 256) {
    long t = i / c4n;
    const int c4 = (int)(i - t * c4n);
    const int w = (int)(t % W);
    t /= W;
    const int h = (int)(t % H);
    const long b = t / H;
    const int oh = h >> 1, ow = w >> 1;
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (oh < Ho && ow < Wo) {
      const float* src = y + (((b * H + 2 * oh) * W + 2 * ow) * C + 4 * c4);
      f32x4 v[4];
      v[0] = *reinterpret_cast<const f32x4*>(src);
      v[1] = *reinterpret_cast<const f32x4*>(src + C);
      v[2] = *reinterpret_cast<const f32x4*>(src + (long)W * C);
      v[3] = *reinterpret_cast<const f32x4*>(src + (long)W * C + C);
      const f32x4 g = *reinterpret_cast<const f32x4*>(dout + (((b * Ho + oh) * Wo + ow) * C + 4 * c4));
      const int own = ((h & 1) << 1) | (w & 1);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int arg = 0;
        float me = v[0][e];
        pool_step(v[1][e], 1, me, arg);
        pool_step(v[2][e], 2, me, arg);
        pool_step(v[3][e], 3, me, arg);
        const float mine = own == 0 ? v[0][e] : (own == 1 ? v[1][e] : (own == 2 ? v[2][e] : v[3][e]));
        r[e] = (arg == own && mine > 0.f) ? g[e] : 0.f;
      }
    }
    reinterpret_cast<f32x4*>(dy)[i] = r;
  }
}

static unsigned stream_blocks(long n) {  // grid-stride launches: at most 65535 workgroups of 256
  const long b = (n + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

extern "C" int sisr_vgg_prep_fwd(const float* img, const float* mean3, const float* std3, float* out, int B, int H, int W,
                                 int cp, void* stream) {
  if (!img || !mean3 || !std3 || !out || B <= 0 || H <= 0 || W <= 0 || cp <= 0) return SISR_ERR_ARG;
  if (cp & 63) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(out)) return SISR_ERR_ALIGN;
  const long hw = (long)H * W, total4 = (long)B * hw * (cp >> 2);
  hipLaunchKernelGGL(vgg_prep_fwd_kernel, dim3(stream_blocks(total4)), dim3(256), 0, (hipStream_t)stream, img, mean3, std3,
                     out, hw, cp, total4);
  return sisr_check_launch();
}

extern "C" int sisr_vgg_prep_bwd(const float* gmap, const float* std3, float* dimg, int B, int H, int W, int cp, void* stream) {
  if (!gmap || !std3 || !dimg || B <= 0 || H <= 0 || W <= 0 || cp <= 0) return SISR_ERR_ARG;
  if (cp & 63) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(gmap)) return SISR_ERR_ALIGN;
  const long hw = (long)H * W, pixels = (long)B * hw;
  hipLaunchKernelGGL(vgg_prep_bwd_kernel, dim3(stream_blocks(pixels)), dim3(256), 0, (hipStream_t)stream, gmap, std3, dimg,
                     hw, cp, pixels);
  return sisr_check_launch();
}

extern "C" int sisr_maxpool2_fwd(const float* y, float* out, int B, int H, int W, int C, void* stream) {
  if (!y || !out || B <= 0 || H <= 0 || W <= 0 || C <= 0) return SISR_ERR_ARG;
  if ((C & 63) || H < 2 || W < 2) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(y) || !sisr_aligned16(out)) return SISR_ERR_ALIGN;
  const long total4 = (long)B * (H >> 1) * (W >> 1) * (C >> 2);
  hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3(stream_blocks(total4)), dim3(256), 0, (hipStream_t)stream, y, out, H, W, C,
                     total4);
  return sisr_check_launch();
}

extern "C" int sisr_maxpool2_relu_bwd(const float* y, const float* dout, float* dy, int B, int H, int W, int C, void* stream) {
  if (!y || !dout || !dy || B <= 0 || H <= 0 || W <= 0 || C <= 0) return SISR_ERR_ARG;
  if ((C & 63) || H < 2 || W < 2) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(y) || !sisr_aligned16(dout) || !sisr_aligned16(dy)) return SISR_ERR_ALIGN;
  const long total4 = (long)B * H * W * (C >> 2);
  hipLaunchKernelGGL(maxpool2_relu_bwd_kernel, dim3(stream_blocks(total4)), dim3(256), 0, (hipStream_t)stream, y, dout, dy,
                     H, W, C, total4);
  return sisr_check_launch();
}
