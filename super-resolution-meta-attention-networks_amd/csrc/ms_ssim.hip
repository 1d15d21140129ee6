// Multi-scale SSIM of two image batches, as a training loss term and as a metric: the per-plane values, their mean and the
// gradient of that mean with respect to the first operand (multiscale.MultiScaleStructuralMechanism, metrics.batch_ms_ssim;
// DESIGN.md 6t).
//
// Per plane pair, M weights w_j and data range R:
//   scale 0 is the plane as given; scale j + 1 is the 2 x 2 mean of scale j with stride 2, a trailing odd row or column
//   dropped (F.avg_pool2d(t, 2));
//   on every scale the window maps of csrc/ssim_loss.hip (11 Gaussian taps, sigma 1.5, population covariance, the windows
//   inside the plane, C1 = (0.01 R)^2, C2 = (0.03 R)^2);
//   c_j = mean over windows of A2 / B2 for j < M - 1, c_{M-1} = mean over windows of S = (A1 A2) / (B1 B2);
//   MS = prod_j c_j^{w_j}, and exactly 0 with an exactly zero gradient when any c_j <= 0 -- a scale whose weight is 0
//   included: the rule looks at the means, not at the weights, so it is not max(c_j, 0)^0 = 1 there.
// The batch value is the mean of MS over the planes, rounded to fp32 once.
//
// Gradient.  For cs = A2 / B2 the coefficients of the differential are
//   beta = d cs / d Exx = -cs / B2,  gamma = d cs / d Exy = 2 / B2,  alpha = d cs / d mx = -my gamma - 2 mx beta
// (SlSsim::pixel's alpha without its two luminance terms); at the last scale they are SlSsim::pixel's.  With
//   g_j = G^T alpha + 2 x_j G^T beta + y_j G^T gamma            (x_j, y_j: the planes at scale j)
//   f_j = w_j MS / (c_j windows_j planes)                        (per plane; 0 when the plane's value is 0)
// the gradient at scale j is D_j = f_j g_j + (1/4) D_{j+1}[parent pixel], the second term absent at the last scale and on
// the pixels of a dropped row or column; D_0, rounded to fp32, is the result.
//
// Entry points sisr_ms_ssim (planes as given -> per-plane float64 values, the fp32 mean, the fp32 gradient) and
// sisr_luma_clip (clipped RGB -> Y planes, for the metric).  Launches of sisr_ms_ssim, 3 M + 1 for M scales with `value` and
// a gradient (16 for five; the M of sl_grad_kernel fewer without a gradient: 2 M + 1; one fewer, sl_finish_kernel, without
// `value`: 3 M and 2 M), none depending on the batch; the sl_* kernels are those of csrc/ssim_window.h:
//   ms_pool_kernel   x (M - 1)   scale j -> j + 1 of both operands, float64 (the sum of four floats is exact there)
//   sl_fwd_kernel    x M         LOAD = SlPlane<float> at scale 0, SlPlane<double> above; PIXEL = MsContrastStructure, SlSsim
//                                at the last scale; the tile's sum of cs or S and, with a gradient, alpha, beta, gamma
//   ms_plane_kernel  x 1         one wave per plane: the tile sums of every scale added in a fixed order, c_j, MS (pow in
//                                float64) and the factors f_j
//   sl_finish_kernel x 1         (with `value`) the planes' MS added in a fixed order, divided by the plane count, rounded
//                                to fp32 once
//   sl_grad_kernel   x M         coarsest scale first; SCALE = MsPlaneFactor: scaled by f_j, a quarter of the parent pixel
//                                of D_{j+1} added (PARENT), D_j stored in float64 (j >= 1) or the result in fp32 (j = 0)
// No atomics: a repeat call is bit-identical.  No allocation, no host synchronisation.  Everything between the fp32 inputs
// and the two fp32 roundings of the outputs is float64, in registers and in memory.
#include "sisr_common.h"
#include "ssim_window.h"
#include <math.h>

#define MS_MAX_LEVELS 8

struct MsPlan {
  int levels;
  int tiles[MS_MAX_LEVELS];       // window tiles per plane at scale j
  long part_off[MS_MAX_LEVELS];   // where scale j's [planes][tiles] sums start
  double windows[MS_MAX_LEVELS];  // windows per plane at scale j
  double weight[MS_MAX_LEVELS];
};

// the per-window quantity of every scale but the last: cs = A2 / B2 in the operation order of SlSsim::pixel, with the
// coefficients of its differential
struct MsContrastStructure {
  template <bool GRAD>
  static __device__ __forceinline__ double pixel(double mx, double my, double mxx, double myy, double mxy, double c1,
                                                 double c2, double& alpha, double& beta, double& gamma) {
#pragma clang fp contract(off)
    const double vx = mxx - mx * mx, vy = myy - my * my, vxy = mxy - mx * my;
    const double a2 = 2.0 * vxy + c2;
    const double b2 = vx + vy + c2;
    const double cs = a2 / b2;
    if (GRAD) {
      beta = -cs / b2;
      gamma = 2.0 / b2;
      alpha = -my * gamma - 2.0 * mx * beta;
    }
    return cs;
  }
};

// the last step of the gradient at one scale: times the plane's factor f_j (`factor` points at [0][j] of [planes][8])
struct MsPlaneFactor {
  const double* factor;
  __device__ __forceinline__ double of(int plane) const { return factor[(long)plane * MS_MAX_LEVELS]; }
  static __device__ __forceinline__ double apply(double f, double g) { return f * g; }
};

// scale j -> j + 1 of both operands: out[r][c] = mean of in[2r .. 2r + 1][2c .. 2c + 1]; ho = h / 2, wo = w / 2
template <typename T>
__global__ __launch_bounds__(256) void ms_pool_kernel(const T* __restrict__ xin, const T* __restrict__ yin, int h, int w,
                                                      int ho, int wo, long total, double* __restrict__ xout,
                                                      double* __restrict__ yout) {
#pragma clang fp contract(off)
  const long per = (long)ho * wo;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long p = i / per, q = i - p * per;
    const int r = (int)(q / wo), c = (int)(q - (long)r * wo);
    const long s = p * h * w + (long)(2 * r) * w + 2 * c;  // rows 2r, 2r + 1 < h and columns 2c, 2c + 1 < w
    xout[i] = ((((double)xin[s] + (double)xin[s + 1]) + (double)xin[s + w]) + (double)xin[s + w + 1]) * 0.25;
    yout[i] = ((((double)yin[s] + (double)yin[s + 1]) + (double)yin[s + w]) + (double)yin[s + w + 1]) * 0.25;
  }
}

// One wave per plane: c_j = (tile sums of scale j, in a fixed order) / windows_j; MS = prod c_j^{w_j}, or 0 when a c_j <= 0;
// factor[plane][j] = w_j MS / (c_j windows_j planes), or 0
__global__ __launch_bounds__(64) void ms_plane_kernel(const double* __restrict__ part, MsPlan pl, int planes,
                                                      double* __restrict__ per_plane, double* __restrict__ factor) {
  const int p = blockIdx.x, lane = threadIdx.x;
  double c[MS_MAX_LEVELS];
#pragma unroll
  for (int j = 0; j < MS_MAX_LEVELS; ++j) {
    c[j] = 1.0;
    if (j < pl.levels) {
      const double* src = part + pl.part_off[j] + (long)p * pl.tiles[j];
      double s = 0.0;
      for (int i = lane; i < pl.tiles[j]; i += 64) s += src[i];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      c[j] = s / pl.windows[j];
    }
  }
  if (lane != 0) return;
  bool dead = false;
  double ms = 1.0;
#pragma unroll
  for (int j = 0; j < MS_MAX_LEVELS; ++j)
    if (j < pl.levels) {
      dead = dead || c[j] <= 0.0;  // a NaN mean is not "<= 0": it goes through pow and shows in the value
      ms *= pow(c[j], pl.weight[j]);
    }
  if (dead) ms = 0.0;
  per_plane[p] = ms;
#pragma unroll
  for (int j = 0; j < MS_MAX_LEVELS; ++j)
    if (j < pl.levels)
      factor[(long)p * MS_MAX_LEVELS + j] = dead ? 0.0 : pl.weight[j] * ms / (c[j] * pl.windows[j] * (double)planes);
}

// the Y planes that sisr_ssim stages on the way into LDS, written out: y[n][q] = sl_clip_luma of pixel q of RGB image n
__global__ __launch_bounds__(256) void ms_luma_kernel(const float* __restrict__ rgb, long plane, long total,
                                                      float* __restrict__ y) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long n = i / plane, q = i - n * plane;
    y[i] = SlClippedLuma::load(rgb + n * 3 * plane, plane, q);
  }
}

// workspace, every block padded to 16 bytes: the tile sums of every scale; [planes][8] factors; [planes] values; with more
// than one scale the float64 pyramids of both operands (scales 1 .. M - 1); with a gradient three float64 maps on every
// scale's window grid and the float64 gradients of scales 1 .. M - 1
struct MsLayout {
  size_t part, factor, per_plane, px, py, maps, dbuf, total;
  size_t part_off[MS_MAX_LEVELS];  // in doubles, from `part`
  size_t pyr_off[MS_MAX_LEVELS];   // in doubles, from `px` / `py` / `dbuf`; [0] unused
  size_t map_off[MS_MAX_LEVELS];   // in doubles, from `maps`
};

static inline size_t ms_pad16(size_t n) { return (n + 15) & ~(size_t)15; }

static inline bool ms_shape_ok(int planes, int h, int w, int levels) {
  if (planes <= 0 || levels < 1 || levels > MS_MAX_LEVELS) return false;
  const long least = (long)SL_K << (levels - 1);  // every scale holds a window
  return h >= least && w >= least;
}

static MsLayout ms_layout(int planes, int h, int w, int levels, bool want_grad) {
  MsLayout l;
  size_t n_part = 0, n_pyr = 0, n_map = 0;
  for (int j = 0; j < MS_MAX_LEVELS; ++j) l.part_off[j] = l.pyr_off[j] = l.map_off[j] = 0;
  for (int j = 0; j < levels; ++j) {
    const int hj = h >> j, wj = w >> j;
    l.part_off[j] = n_part;
    n_part += (size_t)planes * (size_t)sl_win_tiles(hj, wj);
    l.map_off[j] = n_map;
    n_map += 3 * (size_t)planes * (size_t)(hj - 2 * SL_R) * (size_t)(wj - 2 * SL_R);
    if (j) {
      l.pyr_off[j] = n_pyr;
      n_pyr += (size_t)planes * (size_t)hj * (size_t)wj;
    }
  }
  size_t o = 0;
  l.part = o;
  o += ms_pad16(n_part * sizeof(double));
  l.factor = o;
  o += ms_pad16((size_t)planes * MS_MAX_LEVELS * sizeof(double));
  l.per_plane = o;
  o += ms_pad16((size_t)planes * sizeof(double));
  l.px = o;
  o += ms_pad16(n_pyr * sizeof(double));
  l.py = o;
  o += ms_pad16(n_pyr * sizeof(double));
  l.maps = l.dbuf = o;
  if (want_grad) {
    o += ms_pad16(n_map * sizeof(double));
    l.dbuf = o;
    o += ms_pad16(n_pyr * sizeof(double));
  }
  l.total = o;
  return l;
}

extern "C" size_t sisr_ms_ssim_workspace_bytes(int planes, int h, int w, int levels, int want_grad) {
  if (!ms_shape_ok(planes, h, w, levels)) return 0;
  return ms_layout(planes, h, w, levels, want_grad != 0).total;
}

template <typename T, typename O>
static void ms_launch_grad(bool has_parent, unsigned blocks, hipStream_t s, const T* a, const T* b, int h, int w,
                           const double* factor, const SsimLossTaps& tp, const double* ma, const double* mb,
                           const double* mg, const double* parent, O* out) {
  const int tx = (int)sl_pix_tiles_x(w), pt = (int)sl_pix_tiles(h, w);
  if (has_parent)
    hipLaunchKernelGGL((sl_grad_kernel<T, O, MsPlaneFactor, true>), dim3(blocks), dim3(64), 0, s, a, b, h, w, tx, pt,
                       MsPlaneFactor{factor}, tp, ma, mb, mg, parent, h >> 1, w >> 1, out);
  else
    hipLaunchKernelGGL((sl_grad_kernel<T, O, MsPlaneFactor, false>), dim3(blocks), dim3(64), 0, s, a, b, h, w, tx, pt,
                       MsPlaneFactor{factor}, tp, ma, mb, mg, (const double*)nullptr, 0, 0, out);
}

extern "C" int sisr_ms_ssim(const float* sr, const float* y, int planes, int h, int w, double data_range,
                            const double* weights, int levels, double* per_plane, float* value, float* grad,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!sr || !y || !weights || !workspace || (!per_plane && !value) || !ms_shape_ok(planes, h, w, levels) ||
      !isfinite(data_range) || !(data_range > 0.0))
    return SISR_ERR_ARG;
  for (int j = 0; j < levels; ++j)
    if (!isfinite(weights[j]) || weights[j] < 0.0) return SISR_ERR_ARG;
  const bool want_grad = grad != nullptr;
  const MsLayout l = ms_layout(planes, h, w, levels, want_grad);
  if (workspace_bytes < l.total) return SISR_ERR_ARG;
  if (!sisr_aligned16(workspace) || ((uintptr_t)sr & 3) || ((uintptr_t)y & 3) || ((uintptr_t)value & 3) ||
      ((uintptr_t)grad & 3) || ((uintptr_t)per_plane & 7))
    return SISR_ERR_ALIGN;
  // scale 0 has the most tiles of every kind
  if ((long)planes * sl_win_tiles(h, w) > 0x7fffffffL || (long)planes * sl_pix_tiles(h, w) > 0x7fffffffL)
    return SISR_ERR_UNSUPPORTED;

  const SsimLossTaps tp = sl_make_taps();
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  char* base = static_cast<char*>(workspace);
  double* part = reinterpret_cast<double*>(base + l.part);
  double* factor = reinterpret_cast<double*>(base + l.factor);
  double* pplane = per_plane ? per_plane : reinterpret_cast<double*>(base + l.per_plane);
  double* px = reinterpret_cast<double*>(base + l.px);
  double* py = reinterpret_cast<double*>(base + l.py);
  double* maps = reinterpret_cast<double*>(base + l.maps);
  double* dbuf = reinterpret_cast<double*>(base + l.dbuf);
  const hipStream_t s = (hipStream_t)stream;
  int rc;

  MsPlan pl;
  pl.levels = levels;
  for (int j = 0; j < MS_MAX_LEVELS; ++j) {
    const bool on = j < levels;
    const int hj = on ? h >> j : SL_K, wj = on ? w >> j : SL_K;
    pl.tiles[j] = on ? (int)sl_win_tiles(hj, wj) : 0;
    pl.part_off[j] = (long)l.part_off[j];
    pl.windows[j] = (double)(hj - 2 * SL_R) * (double)(wj - 2 * SL_R);
    pl.weight[j] = on ? weights[j] : 0.0;
  }

  for (int j = 0; j < levels; ++j) {
    const int hj = h >> j, wj = w >> j;
    const bool last = j == levels - 1;
    const long nwin = (long)(hj - 2 * SL_R) * (long)(wj - 2 * SL_R);
    double* ma = maps + l.map_off[j];
    double* mb = ma + (long)planes * nwin;
    double* mg = mb + (long)planes * nwin;
    const unsigned blocks = (unsigned)((long)planes * sl_win_tiles(hj, wj));
    double* pj = part + l.part_off[j];
    const double* xj = px + l.pyr_off[j];
    const double* yj = py + l.pyr_off[j];
    if (j == 0) {
      if (last) sl_launch_fwd<float, SlSsim>(want_grad, blocks, s, sr, y, hj, wj, c1, c2, tp, pj, ma, mb, mg);
      else sl_launch_fwd<float, MsContrastStructure>(want_grad, blocks, s, sr, y, hj, wj, c1, c2, tp, pj, ma, mb, mg);
    } else {
      if (last) sl_launch_fwd<double, SlSsim>(want_grad, blocks, s, xj, yj, hj, wj, c1, c2, tp, pj, ma, mb, mg);
      else sl_launch_fwd<double, MsContrastStructure>(want_grad, blocks, s, xj, yj, hj, wj, c1, c2, tp, pj, ma, mb, mg);
    }
    if ((rc = sisr_check_launch())) return rc;
    if (!last) {  // the next scale of both operands
      const int ho = hj >> 1, wo = wj >> 1;
      const long total = (long)planes * ho * wo;
      const unsigned pb = (unsigned)(sl_div_up(total, 256) < (1L << 20) ? sl_div_up(total, 256) : (1L << 20));
      double* xo = px + l.pyr_off[j + 1];
      double* yo = py + l.pyr_off[j + 1];
      if (j == 0)
        hipLaunchKernelGGL(ms_pool_kernel<float>, dim3(pb), dim3(256), 0, s, sr, y, hj, wj, ho, wo, total, xo, yo);
      else
        hipLaunchKernelGGL(ms_pool_kernel<double>, dim3(pb), dim3(256), 0, s, xj, yj, hj, wj, ho, wo, total, xo, yo);
      if ((rc = sisr_check_launch())) return rc;
    }
  }
  hipLaunchKernelGGL(ms_plane_kernel, dim3((unsigned)planes), dim3(64), 0, s, part, pl, planes, pplane, factor);
  if ((rc = sisr_check_launch())) return rc;
  if (value) {
    hipLaunchKernelGGL(sl_finish_kernel<float>, dim3(1), dim3(256), 0, s, pplane, (long)planes, (double)planes, value);
    if ((rc = sisr_check_launch())) return rc;
  }
  if (!want_grad) return SISR_OK;
  for (int j = levels - 1; j >= 0; --j) {
    const int hj = h >> j, wj = w >> j;
    const bool last = j == levels - 1;
    const long nwin = (long)(hj - 2 * SL_R) * (long)(wj - 2 * SL_R);
    const double* ma = maps + l.map_off[j];
    const double* mb = ma + (long)planes * nwin;
    const double* mg = mb + (long)planes * nwin;
    const unsigned blocks = (unsigned)((long)planes * sl_pix_tiles(hj, wj));
    const double* parent = last ? nullptr : dbuf + l.pyr_off[j + 1];
    if (j == 0)
      ms_launch_grad<float, float>(!last, blocks, s, sr, y, hj, wj, factor + j, tp, ma, mb, mg, parent, grad);
    else
      ms_launch_grad<double, double>(!last, blocks, s, px + l.pyr_off[j], py + l.pyr_off[j], hj, wj, factor + j, tp, ma, mb,
                                     mg, parent, dbuf + l.pyr_off[j]);
    if ((rc = sisr_check_launch())) return rc;
  }
  return SISR_OK;
}

extern "C" int sisr_luma_clip(const float* rgb, int n, int h, int w, float* y, void* stream) {
  if (!rgb || !y || n <= 0 || h <= 0 || w <= 0) return SISR_ERR_ARG;
  if (((uintptr_t)rgb & 3) || ((uintptr_t)y & 3)) return SISR_ERR_ALIGN;
  const long plane = (long)h * w, total = (long)n * plane;
  const unsigned blocks = (unsigned)(sl_div_up(total, 256) < (1L << 20) ? sl_div_up(total, 256) : (1L << 20));
  hipLaunchKernelGGL(ms_luma_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rgb, plane, total, y);
  return sisr_check_launch();
}
