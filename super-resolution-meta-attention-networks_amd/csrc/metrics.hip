// SSIM of image pairs, float64 window statistics (the reference's validation / evaluation metric).
//
// ref: Code/sr_tools/metrics.py:64-91 -> skimage.metrics.structural_similarity(a, b, data_range=R, gaussian_weights=True,
//      sigma=1.5, use_sample_covariance=False) on the Y channels of the clipped SR output and of the HR image, one image at a
//      time; the float64 form of scikit-image 0.16-0.18.
//   taps   w[k] = exp(-k^2 / (2 sigma^2)) / sum, k = -5..5 (scipy's _gaussian_kernel1d, truncate 3.5), applied separably
//   mu     mx, my, mxx, myy, mxy = filtered x, y, x^2, y^2, x*y;  vx = mxx - mx^2, vy = myy - my^2, vxy = mxy - mx*my
//   S      (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)),  C1 = (0.01 R)^2, C2 = (0.03 R)^2
//   result the mean of S over the map cropped by 5 pixels on every side.
// The crop equals the filter radius, so every surviving value reads in-bounds pixels only and the padding mode never shows:
// only the (H-10) x (W-10) valid windows are computed.
//
// Shape: one wave per tile of 64 output columns x SSIM_TH output rows.  Each input row of the tile (74 columns) is staged
// in LDS as fp32 (channels == 3: clipped and converted to Y on the way, so no Y map is written), every lane filters it
// horizontally for its column into five fp64 sums, and those slide through an 11-row register ring that the vertical
// filter reads.  Per-tile sums of S go to the workspace in tile order; a second launch adds them per image in a fixed
// order.  No atomics: a repeat launch is bit-identical.
#include "sisr_common.h"
#include <math.h>

#define SSIM_R 5                  // filter radius: int(3.5 * 1.5 + 0.5)
#define SSIM_K (2 * SSIM_R + 1)   // 11 taps
#define SSIM_TW 64                // output columns per tile: one per lane
#define SSIM_TH 32                // output rows per tile

struct SsimTaps {
  double w[SSIM_K];
};

static inline long ssim_tiles_x(int w) { return (w - 2 * SSIM_R + SSIM_TW - 1) / SSIM_TW; }
static inline long ssim_tiles(int h, int w) { return ssim_tiles_x(w) * ((h - 2 * SSIM_R + SSIM_TH - 1) / SSIM_TH); }

// np.clip(v, 0, 1): NaN stays NaN (both comparisons are false), -0 stays -0
__device__ __forceinline__ float ssim_clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// One staged value: the plane as given (C == 1), or the Y of the clipped RGB pixel exactly as metrics.batch_rgb_to_ycbcr
// forms it on the host in fp32: (0.299 R + 0.587 G) + 0.114 B, rounded after every operation.
template <int C>
__device__ __forceinline__ float ssim_load(const float* __restrict__ p, long plane, long off) {
#pragma clang fp contract(off)
  if (C == 1) return p[off];
  const float r = ssim_clip01(p[off]), g = ssim_clip01(p[plane + off]), b = ssim_clip01(p[2 * plane + off]);
  return (0.299f * r + 0.587f * g) + 0.114f * b;
}

// S in scikit-image's operation order; symmetric, so S(x, x) is exactly 1
__device__ __forceinline__ double ssim_pixel(double mx, double my, double mxx, double myy, double mxy, double c1,
                                             double c2) {
#pragma clang fp contract(off)
  const double vx = mxx - mx * mx, vy = myy - my * my, vxy = mxy - mx * my;
  const double a1 = 2.0 * mx * my + c1, a2 = 2.0 * vxy + c2;
  const double b1 = mx * mx + my * my + c1, b2 = vx + vy + c2;
  return (a1 * a2) / (b1 * b2);
}

template <int C>
__global__ __launch_bounds__(64) void ssim_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int h,
                                                       int w, int tiles_x, int tiles_per_img, double c1, double c2,
                                                       SsimTaps tp, double* __restrict__ part) {
  __shared__ float sx[2][SSIM_TW + 2 * SSIM_R], sy[2][SSIM_TW + 2 * SSIM_R];
  const int img = blockIdx.x / tiles_per_img, t = blockIdx.x - img * tiles_per_img;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int lane = threadIdx.x;
  const int c0 = tx * SSIM_TW, r0 = ty * SSIM_TH;
  const int n_in = min(SSIM_TH, h - 2 * SSIM_R - r0) + 2 * SSIM_R;  // input rows r0 .. r0 + n_in - 1, all < h
  const long plane = (long)h * w;
  const float* pa = a + (long)img * C * plane;
  const float* pb = b + (long)img * C * plane;
  // staged columns: c0 + lane, and c0 + 64 + lane on the first 10 lanes; clamped into the image on a right-edge tile,
  // where those values only reach columns that are not output
  const long col0 = min(c0 + lane, w - 1), col1 = min(c0 + SSIM_TW + lane, w - 1);
  const bool halo = lane < 2 * SSIM_R;
  const bool out_col = c0 + lane < w - 2 * SSIM_R;

  long off = (long)r0 * w;
  float x0 = ssim_load<C>(pa, plane, off + col0), y0 = ssim_load<C>(pb, plane, off + col0);
  float x1 = 0.f, y1 = 0.f;
  if (halo) {
    x1 = ssim_load<C>(pa, plane, off + col1);
    y1 = ssim_load<C>(pb, plane, off + col1);
  }

  double rx[SSIM_K], ry[SSIM_K], rxx[SSIM_K], ryy[SSIM_K], rxy[SSIM_K];  // horizontal sums of the last 11 rows
  double acc = 0.0;
  for (int i0 = 0; i0 < n_in; i0 += SSIM_K) {
#pragma unroll
    for (int j = 0; j < SSIM_K; ++j) {  // input row i = i0 + j sits in ring slot j
      const int i = i0 + j;
      if (i < n_in) {
        float* bx = sx[i & 1];
        float* by = sy[i & 1];
        bx[lane] = x0;
        by[lane] = y0;
        if (halo) {
          bx[SSIM_TW + lane] = x1;
          by[SSIM_TW + lane] = y1;
        }
        __syncthreads();
        if (i + 1 < n_in) {  // the next row's loads fly while this one is filtered
          off += w;
          x0 = ssim_load<C>(pa, plane, off + col0);
          y0 = ssim_load<C>(pb, plane, off + col0);
          if (halo) {
            x1 = ssim_load<C>(pa, plane, off + col1);
            y1 = ssim_load<C>(pb, plane, off + col1);
          }
        }
        double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
        for (int k = 0; k < SSIM_K; ++k) {
          const double xv = (double)bx[lane + k], yv = (double)by[lane + k];
          const double wx = tp.w[k] * xv, wy = tp.w[k] * yv;
          hx += wx;
          hy += wy;
          hxx += wx * xv;
          hyy += wy * yv;
          hxy += wx * yv;
        }
        rx[j] = hx;
        ry[j] = hy;
        rxx[j] = hxx;
        ryy[j] = hyy;
        rxy[j] = hxy;
        if (i >= 2 * SSIM_R) {  // output row r0 + i - 10: input rows i - 10 .. i are ring slots (j + 1 + k) % 11
          double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
          for (int k = 0; k < SSIM_K; ++k) {
            const int s = (j + 1 + k) % SSIM_K;
            mx += tp.w[k] * rx[s];
            my += tp.w[k] * ry[s];
            mxx += tp.w[k] * rxx[s];
            myy += tp.w[k] * ryy[s];
            mxy += tp.w[k] * rxy[s];
          }
          const double s = ssim_pixel(mx, my, mxx, myy, mxy, c1, c2);
          if (out_col) acc += s;
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) part[blockIdx.x] = acc;
}

// out[img] = (sum of the image's tile sums, in a fixed order) / ((h - 10) * (w - 10))
__global__ __launch_bounds__(256) void ssim_finish_kernel(const double* __restrict__ part, int tiles_per_img, double count,
                                                          double* __restrict__ out) {
  __shared__ double red[256];
  const double* p = part + (long)blockIdx.x * tiles_per_img;
  double s = 0.0;
  for (int i = threadIdx.x; i < tiles_per_img; i += 256) s += p[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0] / count;
}

extern "C" size_t sisr_ssim_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || h < SSIM_K || w < SSIM_K) return 0;
  return (size_t)n * (size_t)ssim_tiles(h, w) * sizeof(double);
}

extern "C" int sisr_ssim(const float* a, const float* b, int n, int channels, int h, int w, double data_range,
                         double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a || !b || !out || !workspace || n <= 0 || h < SSIM_K || w < SSIM_K || (channels != 1 && channels != 3) ||
      !isfinite(data_range) || !(data_range > 0.0))
    return SISR_ERR_ARG;
  if (workspace_bytes < sisr_ssim_workspace_bytes(n, h, w)) return SISR_ERR_ARG;
  const long tiles = ssim_tiles(h, w);
  if ((long)n * tiles > 0x7fffffffL) return SISR_ERR_UNSUPPORTED;
  // scipy.ndimage._gaussian_kernel1d(1.5, 0, 5): exp(-0.5 / sigma^2 * x^2), normalised by numpy's sum of 11 terms
  // (eight running partials paired up, then the last three added in order)
  SsimTaps tp;
  const double f = -0.5 / (1.5 * 1.5);
  for (int k = 0; k < SSIM_K; ++k) tp.w[k] = exp(f * (double)((k - SSIM_R) * (k - SSIM_R)));
  double sum = ((tp.w[0] + tp.w[1]) + (tp.w[2] + tp.w[3])) + ((tp.w[4] + tp.w[5]) + (tp.w[6] + tp.w[7]));
  for (int k = 8; k < SSIM_K; ++k) sum += tp.w[k];
  for (int k = 0; k < SSIM_K; ++k) tp.w[k] /= sum;
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  double* part = static_cast<double*>(workspace);
  const hipStream_t s = (hipStream_t)stream;
  if (channels == 3)
    hipLaunchKernelGGL(ssim_tile_kernel<3>, dim3((unsigned)(n * tiles)), dim3(64), 0, s, a, b, h, w, (int)ssim_tiles_x(w),
                       (int)tiles, c1, c2, tp, part);
  else
    hipLaunchKernelGGL(ssim_tile_kernel<1>, dim3((unsigned)(n * tiles)), dim3(64), 0, s, a, b, h, w, (int)ssim_tiles_x(w),
                       (int)tiles, c1, c2, tp, part);
  int rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)n), dim3(256), 0, s, part, (int)tiles,
                     (double)(h - 2 * SSIM_R) * (double)(w - 2 * SSIM_R), out);
  return sisr_check_launch();
}
