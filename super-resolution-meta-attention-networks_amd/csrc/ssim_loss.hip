// Mean SSIM of two image batches as a training loss term: the value and its gradient with respect to the first operand
// (structural.StructuralMechanism: loss = pixel term + alpha * (1 - mean SSIM)).
//
// Per plane it is the quantity csrc/metrics.hip documents -- 11 Gaussian taps (sigma 1.5) applied separably, population
// covariance, C1 = (0.01 R)^2, C2 = (0.03 R)^2, S = (2 mx my + C1)(2 vxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)) on the
// (H - 10) x (W - 10) windows inside the image -- on every plane as it is given: no clipping (it would kill the gradient
// outside [0, 1]) and no Y conversion.  The result is the mean of S over all windows of all planes.
//
// Gradient.  With the window maps mx, my, Exx, Exy, A1 = 2 mx my + C1, A2 = 2 vxy + C2, B1, B2:
//   beta  = dS/dExx = -S / B2
//   gamma = dS/dExy = 2 A1 / (B1 B2)
//   alpha = dS/dmx  = 2 my A2 / (B1 B2) - 2 mx S / B1 - my gamma - 2 mx beta
//   d(mean S)/dx    = (G^T alpha + 2 x G^T beta + y G^T gamma) / count
// G^T is the transposed ("full") separable Gaussian correlation: pixel p collects from the windows [p - 10, p] that exist.
//
// Launches (no atomics anywhere: a repeat call is bit-identical; no allocation, no host synchronisation):
//   ssim_loss_fwd_kernel   the shape of ssim_tile_kernel: one wave per tile of 64 x 32 windows, input rows staged in LDS as fp32,
//                          horizontal sums in five 11-slot float64 register rings, the vertical filter reads the rings.  Writes
//                          the tile's sum of S and, when a gradient is wanted, alpha, beta, gamma on the window grid.
//   ssim_loss_grad_kernel  one wave per tile of 64 x 32 pixels: the rows of the three maps (10-window halo, zero outside the
//                          window grid) staged in LDS, filtered horizontally into three 11-slot rings, then vertically;
//                          combined with x and y, divided by the count, one fp32 store per pixel.
//   ssim_loss_finish_kernel  adds the tile sums in a fixed order, divides by the count and rounds to fp32 once.
// The window statistics, S and the three maps are float64.  The maps are float64 in memory too: near convergence the three
// terms of the gradient are O(1 / B2) each and cancel down to O(|x - y| / B2), so maps rounded to fp32 (6e-8 relative) would
// put back, at |x - y| ~ 2e-3, the 3e-5 relative error of an fp32 composition that this kernel exists to avoid.
#include "sisr_common.h"
#include "ssim_window.h"  // SL_*, SsimLossTaps, the tile counts, sl_make_taps, sl_pixel
#include <math.h>

template <bool GRAD>
__global__ __launch_bounds__(64) void ssim_loss_fwd_kernel(const float* __restrict__ a, const float* __restrict__ b, int h,
                                                           int w, int tiles_x, int tiles_per_plane, double c1, double c2,
                                                           SsimLossTaps tp, double* __restrict__ part,
                                                           double* __restrict__ ma, double* __restrict__ mb,
                                                           double* __restrict__ mg) {
  __shared__ float sx[2][SL_SW], sy[2][SL_SW];
  const int plane_i = blockIdx.x / tiles_per_plane, t = blockIdx.x - plane_i * tiles_per_plane;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int lane = threadIdx.x;
  const int c0 = tx * SL_TW, r0 = ty * SL_TH;
  const int hw = h - 2 * SL_R, ww = w - 2 * SL_R;              // the window grid
  const int n_in = min(SL_TH, hw - r0) + 2 * SL_R;             // input rows r0 .. r0 + n_in - 1, all < h
  const float* pa = a + (long)plane_i * h * w;
  const float* pb = b + (long)plane_i * h * w;
  // staged columns: c0 + lane, and c0 + 64 + lane on the first 10 lanes; clamped into the image on a right-edge tile,
  // where those values only reach windows that are not output
  const long col0 = min(c0 + lane, w - 1), col1 = min(c0 + SL_TW + lane, w - 1);
  const bool halo = lane < 2 * SL_R;
  const bool out_col = c0 + lane < ww;
  const long mbase = (long)plane_i * hw * ww + c0 + lane;      // + row * ww: this lane's window in the maps

  long off = (long)r0 * w;
  float x0 = pa[off + col0], y0 = pb[off + col0];
  float x1 = 0.f, y1 = 0.f;
  if (halo) {
    x1 = pa[off + col1];
    y1 = pb[off + col1];
  }

  double rx[SL_K], ry[SL_K], rxx[SL_K], ryy[SL_K], rxy[SL_K];  // horizontal sums of the last 11 rows
  double acc = 0.0;
  for (int i0 = 0; i0 < n_in; i0 += SL_K) {
#pragma unroll
    for (int j = 0; j < SL_K; ++j) {  // input row i = i0 + j sits in ring slot j
      const int i = i0 + j;
      if (i < n_in) {
        float* bx = sx[i & 1];
        float* by = sy[i & 1];
        bx[lane] = x0;
        by[lane] = y0;
        if (halo) {
          bx[SL_TW + lane] = x1;
          by[SL_TW + lane] = y1;
        }
        __syncthreads();
        if (i + 1 < n_in) {  // the next row's loads fly while this one is filtered
          off += w;
          x0 = pa[off + col0];
          y0 = pb[off + col0];
          if (halo) {
            x1 = pa[off + col1];
            y1 = pb[off + col1];
          }
        }
        double hx = 0.0, hy = 0.0, hxx = 0.0, hyy = 0.0, hxy = 0.0;
#pragma unroll
        for (int k = 0; k < SL_K; ++k) {
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
        if (i >= 2 * SL_R) {  // window row r0 + i - 10: input rows i - 10 .. i are ring slots (j + 1 + k) % 11
          double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
          for (int k = 0; k < SL_K; ++k) {
            const int s = (j + 1 + k) % SL_K;
            mx += tp.w[k] * rx[s];
            my += tp.w[k] * ry[s];
            mxx += tp.w[k] * rxx[s];
            myy += tp.w[k] * ryy[s];
            mxy += tp.w[k] * rxy[s];
          }
          double al = 0.0, be = 0.0, ga = 0.0;
          const double s = sl_pixel<GRAD>(mx, my, mxx, myy, mxy, c1, c2, al, be, ga);
          if (out_col) {
            acc += s;
            if (GRAD) {
              const long m = mbase + (long)(r0 + i - 2 * SL_R) * ww;  // row < hw by n_in, column < ww by out_col
              ma[m] = al;
              mb[m] = be;
              mg[m] = ga;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (lane == 0) part[blockIdx.x] = acc;
}

// One wave per tile of 64 x 32 pixels of one plane.  Window row i = r0 - 10 + ii, ii = 0 .. n_in - 1, is staged (columns
// c0 - 10 .. c0 + 63 of the window grid, zero outside it), filtered horizontally for this lane's pixel column into ring slot
// ii % 11; pixel row r = r0 + ii - 10 then reads window rows r - 10 .. r from the ring with tap r - i.
__global__ __launch_bounds__(64) void ssim_loss_grad_kernel(const float* __restrict__ a, const float* __restrict__ b, int h,
                                                            int w, int tiles_x, int tiles_per_plane, double count,
                                                            SsimLossTaps tp, const double* __restrict__ ma,
                                                            const double* __restrict__ mb, const double* __restrict__ mg,
                                                            float* __restrict__ grad) {
  __shared__ double sa[2][SL_SW], sb[2][SL_SW], sg[2][SL_SW];
  const int plane_i = blockIdx.x / tiles_per_plane, t = blockIdx.x - plane_i * tiles_per_plane;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int lane = threadIdx.x;
  const int c0 = tx * SL_TW, r0 = ty * SL_TH;
  const int hw = h - 2 * SL_R, ww = w - 2 * SL_R;
  const int n_out = min(SL_TH, h - r0);   // pixel rows r0 .. r0 + n_out - 1
  const int n_in = n_out + 2 * SL_R;      // window rows r0 - 10 .. r0 + n_out - 1, those outside [0, hw) read as zero
  const long wbase = (long)plane_i * hw * ww;
  // staged window columns: c0 - 10 + lane, and c0 + 54 + lane on the first 10 lanes.  The address is clamped into the
  // row and the value replaced by zero where the column is outside the window grid.
  const int wc0 = c0 - 2 * SL_R + lane, wc1 = c0 + SL_TW - 2 * SL_R + lane;
  const bool in0 = wc0 >= 0 && wc0 < ww, in1 = wc1 < ww;  // wc1 >= 54
  const long cc0 = min(max(wc0, 0), ww - 1), cc1 = min(wc1, ww - 1);
  const bool halo = lane < 2 * SL_R;
  const bool out_col = c0 + lane < w;
  const long pcol = min(c0 + lane, w - 1);
  const float* pa = a + (long)plane_i * h * w;
  const float* pb = b + (long)plane_i * h * w;
  float* pg = grad + (long)plane_i * h * w;

  double a0 = 0.0, b0 = 0.0, g0 = 0.0, a1 = 0.0, b1 = 0.0, g1 = 0.0;
  auto fetch = [&](int ii) {  // window row r0 - 10 + ii into the six registers
    const int wr = r0 - 2 * SL_R + ii;
    const bool row_ok = wr >= 0 && wr < hw;
    const long ro = wbase + (long)min(max(wr, 0), hw - 1) * ww;
    const bool k0 = row_ok && in0, k1 = row_ok && in1;
    const double ta = ma[ro + cc0], tb = mb[ro + cc0], tg = mg[ro + cc0];
    a0 = k0 ? ta : 0.0;
    b0 = k0 ? tb : 0.0;
    g0 = k0 ? tg : 0.0;
    if (halo) {
      const double ua = ma[ro + cc1], ub = mb[ro + cc1], ug = mg[ro + cc1];
      a1 = k1 ? ua : 0.0;
      b1 = k1 ? ub : 0.0;
      g1 = k1 ? ug : 0.0;
    }
  };
  fetch(0);

  double ra[SL_K], rb[SL_K], rg[SL_K];  // horizontal sums of the last 11 window rows
  for (int i0 = 0; i0 < n_in; i0 += SL_K) {
#pragma unroll
    for (int j = 0; j < SL_K; ++j) {  // window row ii = i0 + j sits in ring slot j
      const int ii = i0 + j;
      if (ii < n_in) {
        double* ba = sa[ii & 1];
        double* bb = sb[ii & 1];
        double* bg = sg[ii & 1];
        ba[lane] = a0;
        bb[lane] = b0;
        bg[lane] = g0;
        if (halo) {
          ba[SL_TW + lane] = a1;
          bb[SL_TW + lane] = b1;
          bg[SL_TW + lane] = g1;
        }
        __syncthreads();
        if (ii + 1 < n_in) fetch(ii + 1);  // the next row's loads fly while this one is filtered
        // pixel column c = c0 + lane collects window columns c - 10 .. c = staged slots lane .. lane + 10, tap c - j = 10 - k
        double ha = 0.0, hb = 0.0, hg = 0.0;
#pragma unroll
        for (int k = 0; k < SL_K; ++k) {
          const double wk = tp.w[SL_K - 1 - k];
          ha += wk * ba[lane + k];
          hb += wk * bb[lane + k];
          hg += wk * bg[lane + k];
        }
        ra[j] = ha;
        rb[j] = hb;
        rg[j] = hg;
        if (ii >= 2 * SL_R) {  // pixel row r = r0 + ii - 10: window rows r - 10 .. r are ring slots (j + 1 + k) % 11, tap 10 - k
          double va = 0.0, vb = 0.0, vg = 0.0;
#pragma unroll
          for (int k = 0; k < SL_K; ++k) {
            const int s = (j + 1 + k) % SL_K;
            const double wk = tp.w[SL_K - 1 - k];
            va += wk * ra[s];
            vb += wk * rb[s];
            vg += wk * rg[s];
          }
          const long p = (long)(r0 + ii - 2 * SL_R) * w + pcol;  // row < h by n_out
          const double xv = (double)pa[p], yv = (double)pb[p];
          const double d = (va + 2.0 * xv * vb + yv * vg) / count;
          if (out_col) pg[p] = (float)d;
        }
      }
    }
  }
}

// value = (sum of all tile sums, in a fixed order) / count, rounded to fp32 once
__global__ __launch_bounds__(256) void ssim_loss_finish_kernel(const double* __restrict__ part, long n_part, double count,
                                                               float* __restrict__ value) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < n_part; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) value[0] = (float)(red[0] / count);
}

// workspace: [planes * window tiles] tile sums, padded to 16 bytes; with a gradient, three [planes][h - 10][w - 10] maps
static inline size_t sl_part_bytes(long planes, int h, int w) {
  return (((size_t)planes * (size_t)sl_win_tiles(h, w) * sizeof(double)) + 15) & ~(size_t)15;
}

extern "C" size_t sisr_ssim_loss_workspace_bytes(int planes, int h, int w, int want_grad) {
  if (planes <= 0 || h < SL_K || w < SL_K) return 0;
  size_t n = sl_part_bytes(planes, h, w);
  if (want_grad) n += 3 * (size_t)planes * (size_t)(h - 2 * SL_R) * (size_t)(w - 2 * SL_R) * sizeof(double);
  return n;
}

extern "C" int sisr_ssim_loss(const float* sr, const float* y, int planes, int h, int w, double data_range, float* value,
                              float* grad, void* workspace, size_t workspace_bytes, void* stream) {
  if (!sr || !y || !value || !workspace || planes <= 0 || h < SL_K || w < SL_K || !isfinite(data_range) ||
      !(data_range > 0.0))
    return SISR_ERR_ARG;
  if (workspace_bytes < sisr_ssim_loss_workspace_bytes(planes, h, w, grad != nullptr)) return SISR_ERR_ARG;
  if (!sisr_aligned16(workspace) || ((uintptr_t)sr & 3) || ((uintptr_t)y & 3) || ((uintptr_t)value & 3) ||
      ((uintptr_t)grad & 3))
    return SISR_ERR_ALIGN;
  const long wt = sl_win_tiles(h, w), pt = sl_pix_tiles(h, w);
  if ((long)planes * wt > 0x7fffffffL || (long)planes * pt > 0x7fffffffL) return SISR_ERR_UNSUPPORTED;
  const SsimLossTaps tp = sl_make_taps();
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  const long nwin = (long)(h - 2 * SL_R) * (long)(w - 2 * SL_R);
  const double count = (double)planes * (double)nwin;
  double* part = static_cast<double*>(workspace);
  double* ma = reinterpret_cast<double*>(static_cast<char*>(workspace) + sl_part_bytes(planes, h, w));
  double* mb = ma + (long)planes * nwin;
  double* mg = mb + (long)planes * nwin;
  const hipStream_t s = (hipStream_t)stream;
  if (grad)
    hipLaunchKernelGGL(ssim_loss_fwd_kernel<true>, dim3((unsigned)(planes * wt)), dim3(64), 0, s, sr, y, h, w,
                       (int)sl_win_tiles_x(w), (int)wt, c1, c2, tp, part, ma, mb, mg);
  else
    hipLaunchKernelGGL(ssim_loss_fwd_kernel<false>, dim3((unsigned)(planes * wt)), dim3(64), 0, s, sr, y, h, w,
                       (int)sl_win_tiles_x(w), (int)wt, c1, c2, tp, part, (double*)nullptr, (double*)nullptr,
                       (double*)nullptr);
  int rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(ssim_loss_finish_kernel, dim3(1), dim3(256), 0, s, part, (long)planes * wt, count, value);
  rc = sisr_check_launch();
  if (rc || !grad) return rc;
  hipLaunchKernelGGL(ssim_loss_grad_kernel, dim3((unsigned)(planes * pt)), dim3(64), 0, s, sr, y, h, w,
                     (int)sl_pix_tiles_x(w), (int)pt, count, tp, ma, mb, mg, grad);
  return sisr_check_launch();
}
