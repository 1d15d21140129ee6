// The output stage of evaluation and validation in one streaming pass over a batch of network outputs: the per-image mean
// squared error of the Y channels against the HR batch (what Y-PSNR is taken from) and the 8-bit RGB image in HWC order
// (what a PNG is written from), either or both (metrics.batch_psnr / batch_rgb8 / eval_output).
//
// Per pixel, every fp32 operation rounded on its own (no fma), in the order metrics.py writes it on the host:
//   Ys     sr_planes == 3: sl_clip_luma(R, G, B) = (0.299 clip(R) + 0.587 clip(G)) + 0.114 clip(B), metrics.batch_rgb_to_ycbcr's Y;
//          sr_planes == 1: clip(Y).  clip is np.clip(v, 0, 1).
//   Yh     the same of the HR pixel: hr_form 0 from its three RGB planes, hr_form 1 from plane 0 of hr_planes planes
//   mse    d = Ys - Yh in fp32, d * d in float64, summed over shave <= row < h - shave, shave <= col < w - shave and divided
//          by the count of those pixels
//   rgb8   sr_planes == 3: rint(clip(c) * 255) per channel (ties to even, as np.round);
//          sr_planes == 1: (Y, Cb, Cr) = clip of (sr, chroma plane 1, chroma plane 2), then metrics.ycbcr_to_rgb_jpg --
//            R = (Y + 1.402 Cr) - fl(1.402 b), G = ((Y - 0.344136 Cb) - 0.714136 Cr) + fl((0.714136 + 0.344136) b),
//            B = (Y + 1.772 Cb) - fl(1.772 b), b = 128 * (1 / 255) and fl the fp32 rounding of the float64 product -- then
//            rint(v * 255) CLAMPED to 0 .. 255.  Where the host's rounded value lies in 0 .. 255 the byte is the host's
//            `(rgb * 255).round().astype(uint8)`; elsewhere it saturates (0 or 255) where the host's cast wraps (253 for
//            -0.01, 2 for 1.01).  A NaN gives 0.
//
// An image is walked as a flat run of h * w pixels, four consecutive pixels per lane and group, EO_GROUPS groups per lane,
// EO_BLOCK_PIX pixels per block.  When h * w is a multiple of 4 and every base pointer is 16-byte (rgb8: 4-byte) aligned,
// each plane comes in as one 16-byte load per group and the twelve bytes of a group leave as three dwords (VEC); otherwise
// the same group is read and written element by element with the image's end checked per pixel.  With shave > 0 the row and
// column of a group's first pixel cost one division; the other three follow by increment.
//
// The sum is a two-stage ordered one, without atomics, so a repeat launch is bit-identical: a lane adds its
// 4 * EO_GROUPS squares in pixel order, the wave adds its lanes by six xor-shuffles, lane 0 of wave 0 adds the four wave sums
// in wave order and stores the block's partial at workspace[image][block]; sl_finish_kernel<double> then adds an image's
// partials (thread t takes t, t + 256, ...; eight tree steps) and divides once.  Longest chain of sequential additions:
// 8 + 6 + 3 + ceil(blocks / 256) + 8, blocks = ceil(h * w / 2048): 31 at 1356 x 2040, 4,121 at the largest plane taken
// (h * w just under 2^31).
// No allocation, no host synchronisation: capturable.
#include "sisr_common.h"
#include "ssim_window.h"
#include <math.h>

#define EO_THREADS 256
#define EO_GROUPS 2
#define EO_BLOCK_PIX (EO_THREADS * 4 * EO_GROUPS)

struct EoArgs {
  const float* sr;
  const float* chroma;
  const float* hr;
  double* part;          // null: no mse
  unsigned char* rgb8;   // null: no bytes
  int plane;             // h * w
  int w, h, shave;
  int hr_planes;         // planes between two HR images
  int blocks;            // per image
};

// metrics.ycbcr_to_rgb_jpg on clipped fp32 values; the bias terms are the fp32 roundings of the host's float64 products
__device__ __forceinline__ void eo_ycbcr_to_rgb(float y, float cb, float cr, float& r, float& g, float& b) {
#pragma clang fp contract(off)
  constexpr double bias = 128. * (1. / 255);
  constexpr float kr = (float)(1.402 * bias), kg = (float)((0.714136 + 0.344136) * bias), kb = (float)(1.772 * bias);
  r = (y + 1.402f * cr) - kr;
  g = ((y - 0.344136f * cb) - 0.714136f * cr) + kg;
  b = (y + 1.772f * cb) - kb;
}

// rint(v * 255) clamped to 0 .. 255 (a no-op on clipped values); NaN -> 0
__device__ __forceinline__ unsigned eo_byte(float v) {
#pragma clang fp contract(off)
  const float s = v * 255.f;
  return (unsigned)(int)fminf(fmaxf(rintf(s), 0.f), 255.f);
}

// four consecutive floats from p[off ..]: one 16-byte load, or the first `cnt` of them one by one (the rest 0)
template <bool VEC>
__device__ __forceinline__ void eo_load4(const float* __restrict__ p, long off, int cnt, float v[4]) {
  if (VEC) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(p + off);
    v[0] = q.x;
    v[1] = q.y;
    v[2] = q.z;
    v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[off + j] : 0.f;
  }
}

template <bool VEC, bool SR3, bool HR3>
__global__ __launch_bounds__(EO_THREADS) void eo_kernel(EoArgs a) {
#pragma clang fp contract(off)
  __shared__ double wave_sum[EO_THREADS / 64];
  const int img = blockIdx.x / a.blocks, blk = blockIdx.x - img * a.blocks;
  const long plane = a.plane;
  const float* sr = a.sr + (long)img * (SR3 ? 3 : 1) * plane;
  const float* ch = a.chroma + (long)img * 3 * plane;            // read only when !SR3 and bytes are wanted
  const float* hr = a.hr + (long)img * a.hr_planes * plane;      // read only when the mse is wanted
  unsigned char* out = a.rgb8 + (long)img * 3 * plane;
  const bool want_mse = a.part != nullptr, want_rgb8 = a.rgb8 != nullptr;
  double acc = 0.0;
#pragma unroll
  for (int g = 0; g < EO_GROUPS; ++g) {
    const long p0 = (long)blk * EO_BLOCK_PIX + (long)(g * EO_THREADS + (int)threadIdx.x) * 4;
    if (p0 < plane) {
      const int cnt = VEC ? 4 : (int)(plane - p0 < 4 ? plane - p0 : 4);  // pixels p0 .. p0 + cnt - 1 are inside the image
      float s[3][4], ys[4];
      eo_load4<VEC>(sr, p0, cnt, s[0]);
      if (SR3) {
        eo_load4<VEC>(sr + plane, p0, cnt, s[1]);
        eo_load4<VEC>(sr + 2 * plane, p0, cnt, s[2]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) ys[j] = SR3 ? sl_clip_luma(s[0][j], s[1][j], s[2][j]) : ssim_clip01(s[0][j]);
      if (want_mse) {
        float t[3][4];
        eo_load4<VEC>(hr, p0, cnt, t[0]);
        if (HR3) {
          eo_load4<VEC>(hr + plane, p0, cnt, t[1]);
          eo_load4<VEC>(hr + 2 * plane, p0, cnt, t[2]);
        }
        int row = 0, col = 0;
        if (a.shave > 0) {
          row = (int)((unsigned)p0 / (unsigned)a.w);
          col = (int)p0 - row * a.w;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float yh = HR3 ? sl_clip_luma(t[0][j], t[1][j], t[2][j]) : ssim_clip01(t[0][j]);
          const float d = ys[j] - yh;
          bool in = j < cnt;
          if (a.shave > 0) {
            in = in && row >= a.shave && row < a.h - a.shave && col >= a.shave && col < a.w - a.shave;
            if (++col == a.w) {
              col = 0;
              ++row;
            }
          }
          const double dd = (double)d;
          if (in) acc += dd * dd;
        }
      }
      if (want_rgb8) {
        unsigned b[12];
        if (SR3) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) b[3 * j + c] = eo_byte(ssim_clip01(s[c][j]));
        } else {
          float cb[4], cr[4];
          eo_load4<VEC>(ch + plane, p0, cnt, cb);
          eo_load4<VEC>(ch + 2 * plane, p0, cnt, cr);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float r, gg, bb;
            eo_ycbcr_to_rgb(ys[j], ssim_clip01(cb[j]), ssim_clip01(cr[j]), r, gg, bb);
            b[3 * j] = eo_byte(r);
            b[3 * j + 1] = eo_byte(gg);
            b[3 * j + 2] = eo_byte(bb);
          }
        }
        if (VEC) {  // out + 3 * p0 is 4-byte aligned: p0 and the plane are multiples of 4
          unsigned* o = reinterpret_cast<unsigned*>(out + 3 * p0);
#pragma unroll
          for (int k = 0; k < 3; ++k) o[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
        } else {
#pragma unroll
          for (int k = 0; k < 12; ++k)
            if (k < 3 * cnt) out[3 * p0 + k] = (unsigned char)b[k];
        }
      }
    }
  }
  if (!want_mse) return;  // uniform over the block
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.part[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

static inline long eo_blocks(long plane) { return (plane + EO_BLOCK_PIX - 1) / EO_BLOCK_PIX; }

static inline bool eo_shape_ok(int n, int h, int w) {
  return n > 0 && h > 0 && w > 0 && (long)h * w <= 0x7fffffffL - EO_BLOCK_PIX;
}

extern "C" size_t sisr_eval_output_workspace_bytes(int n, int h, int w) {
  if (!eo_shape_ok(n, h, w)) return 0;
  const size_t bytes = (size_t)n * (size_t)eo_blocks((long)h * w) * sizeof(double);
  return (bytes + 15) & ~(size_t)15;
}

template <bool VEC, bool SR3>
static void eo_launch(bool hr3, unsigned grid, hipStream_t s, const EoArgs& a) {
  if (hr3) hipLaunchKernelGGL((eo_kernel<VEC, SR3, true>), dim3(grid), dim3(EO_THREADS), 0, s, a);
  else hipLaunchKernelGGL((eo_kernel<VEC, SR3, false>), dim3(grid), dim3(EO_THREADS), 0, s, a);
}

extern "C" int sisr_eval_output(const float* sr, int sr_planes, const float* chroma, const float* hr, int hr_form,
                                int hr_planes, int n, int h, int w, int shave, double* mse, unsigned char* rgb8,
                                void* workspace, size_t workspace_bytes, void* stream) {
  if (!sr || (!mse && !rgb8) || (mse && !hr) || (sr_planes != 1 && sr_planes != 3)) return SISR_ERR_ARG;
  if (sr_planes == 1 && rgb8 && !chroma) return SISR_ERR_ARG;
  if (hr && (hr_form < 0 || hr_form > 1 || hr_planes < 1 || (hr_form == 0 && hr_planes < 3))) return SISR_ERR_ARG;
  if (n <= 0 || h <= 0 || w <= 0 || shave < 0 || 2L * shave >= (h < w ? h : w)) return SISR_ERR_ARG;
  if (!eo_shape_ok(n, h, w)) return SISR_ERR_UNSUPPORTED;
  const long plane = (long)h * w, blocks = eo_blocks(plane);
  if (mse && (!workspace || workspace_bytes < sisr_eval_output_workspace_bytes(n, h, w))) return SISR_ERR_ARG;
  if (((uintptr_t)sr & 3) || ((uintptr_t)chroma & 3) || ((uintptr_t)hr & 3) || ((uintptr_t)mse & 7) ||
      (mse && !sisr_aligned16(workspace)))
    return SISR_ERR_ALIGN;
  if ((long)n * blocks > 0x7fffffffL) return SISR_ERR_UNSUPPORTED;

  const bool sr3 = sr_planes == 3;
  const bool use_chroma = !sr3 && rgb8;
  EoArgs a;
  a.sr = sr;
  a.chroma = use_chroma ? chroma : nullptr;
  a.hr = mse ? hr : nullptr;
  a.part = mse ? static_cast<double*>(workspace) : nullptr;
  a.rgb8 = rgb8;
  a.plane = (int)plane;
  a.w = w;
  a.h = h;
  a.shave = shave;
  a.hr_planes = hr_planes;
  a.blocks = (int)blocks;
  // with h * w a multiple of 4 every plane of every image starts 16-byte aligned when its batch does, and every image's
  // byte run (3 h w bytes) 4-byte aligned
  const bool vec = plane % 4 == 0 && sisr_aligned16(sr) && sisr_aligned16(a.chroma) && sisr_aligned16(a.hr) &&
                   ((uintptr_t)rgb8 & 3) == 0;
  const bool hr3 = mse && hr_form == 0;
  const hipStream_t s = (hipStream_t)stream;
  const unsigned grid = (unsigned)((long)n * blocks);
  if (vec) {
    if (sr3) eo_launch<true, true>(hr3, grid, s, a);
    else eo_launch<true, false>(hr3, grid, s, a);
  } else {
    if (sr3) eo_launch<false, true>(hr3, grid, s, a);
    else eo_launch<false, false>(hr3, grid, s, a);
  }
  int rc;
  if ((rc = sisr_check_launch())) return rc;
  if (mse) {
    const double count = (double)(h - 2 * shave) * (double)(w - 2 * shave);
    hipLaunchKernelGGL(sl_finish_kernel<double>, dim3((unsigned)n), dim3(256), 0, s, a.part, blocks, count, mse);
    if ((rc = sisr_check_launch())) return rc;
  }
  return SISR_OK;
}
