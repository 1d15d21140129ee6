// The 11 x 11 Gaussian window of the SSIM family (csrc/metrics.hip, csrc/ssim_loss.hip, csrc/ms_ssim.hip), held once: its
// taps, the tiling of the window and pixel grids by one wave per 64 x 32 tile, S with the three coefficients of its
// differential, the clipped-RGB luma, and the three kernels every form launches --
//   sl_fwd_kernel     one wave per tile of 64 x 32 windows: input rows staged in LDS, horizontal sums in five 11-slot float64
//                     register rings that the vertical filter reads; writes the tile's sum of the per-window quantity and,
//                     when a gradient is wanted, alpha, beta, gamma on the window grid
//   sl_grad_kernel    one wave per tile of 64 x 32 pixels: the rows of the three maps (10-window halo, zero outside the window
//                     grid) staged in LDS, filtered horizontally into three 11-slot rings, then vertically; combined with x
//                     and y, scaled, one store per pixel
//   sl_finish_kernel  block b adds its n values in a fixed order and divides once
// Each .hip file instantiates the ones it launches, with its own policies:
//   LOAD   how one staged value is read: SlPlane<T> (the plane as given) or SlClippedLuma (Y of the clipped RGB pixel)
//   PIXEL  the per-window quantity: SlSsim (S), or a form's own (ms_ssim.hip: A2 / B2)
//   SCALE  the last step of the gradient: `double of(int plane)` read once per tile, `apply(s, g)` per pixel
// The kernel bodies are compiled with default contraction; only the PIXEL policies and sl_clip_luma switch it off.
#pragma once
#include "sisr_common.h"
#include <math.h>

#define SL_R 5                // filter radius: int(3.5 * 1.5 + 0.5)
#define SL_K (2 * SL_R + 1)   // 11 taps
#define SL_TW 64              // tile columns: one per lane
#define SL_TH 32              // tile rows
#define SL_SW (SL_TW + 2 * SL_R)  // staged columns per row

struct SsimLossTaps {
  double w[SL_K];
};

static inline long sl_div_up(long a, long b) { return (a + b - 1) / b; }
// tiles of the window grid (forward) and of the pixel grid (gradient)
static inline long sl_win_tiles_x(int w) { return sl_div_up(w - 2 * SL_R, SL_TW); }
static inline long sl_win_tiles(int h, int w) { return sl_win_tiles_x(w) * sl_div_up(h - 2 * SL_R, SL_TH); }
static inline long sl_pix_tiles_x(int w) { return sl_div_up(w, SL_TW); }
static inline long sl_pix_tiles(int h, int w) { return sl_pix_tiles_x(w) * sl_div_up(h, SL_TH); }

// scipy.ndimage._gaussian_kernel1d(1.5, 0, 5): exp(-0.5 / sigma^2 * x^2), normalised by numpy's sum of 11 terms (eight
// running partials paired up, then the last three added in order)
static inline SsimLossTaps sl_make_taps() {
  SsimLossTaps tp;
  const double f = -0.5 / (1.5 * 1.5);
  for (int k = 0; k < SL_K; ++k) tp.w[k] = exp(f * (double)((k - SL_R) * (k - SL_R)));
  double sum = ((tp.w[0] + tp.w[1]) + (tp.w[2] + tp.w[3])) + ((tp.w[4] + tp.w[5]) + (tp.w[6] + tp.w[7]));
  for (int k = 8; k < SL_K; ++k) sum += tp.w[k];
  for (int k = 0; k < SL_K; ++k) tp.w[k] /= sum;
  return tp;
}

// S in scikit-image's operation order (symmetric, so S(x, x) is exactly 1), and the three coefficients of its differential
struct SlSsim {
  template <bool GRAD>
  static __device__ __forceinline__ double pixel(double mx, double my, double mxx, double myy, double mxy, double c1,
                                                 double c2, double& alpha, double& beta, double& gamma) {
#pragma clang fp contract(off)
    const double vx = mxx - mx * mx, vy = myy - my * my, vxy = mxy - mx * my;
    const double a1 = 2.0 * mx * my + c1, a2 = 2.0 * vxy + c2;
    const double b1 = mx * mx + my * my + c1, b2 = vx + vy + c2;
    const double s = (a1 * a2) / (b1 * b2);
    if (GRAD) {
      beta = -s / b2;
      gamma = 2.0 * a1 / (b1 * b2);
      alpha = 2.0 * my * a2 / (b1 * b2) - 2.0 * mx * s / b1 - my * gamma - 2.0 * mx * beta;
    }
    return s;
  }
};

// np.clip(v, 0, 1): NaN stays NaN (both comparisons are false), -0 stays -0
__device__ __forceinline__ float ssim_clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// Y of the clipped RGB pixel exactly as metrics.batch_rgb_to_ycbcr forms it on the host in fp32:
// (0.299 R + 0.587 G) + 0.114 B, rounded after every operation
__device__ __forceinline__ float sl_clip_luma(float r, float g, float b) {
#pragma clang fp contract(off)
  return (0.299f * ssim_clip01(r) + 0.587f * ssim_clip01(g)) + 0.114f * ssim_clip01(b);
}

// One staged value of an image of `planes` planes of `plane` elements each
template <typename T>
struct SlPlane {
  typedef T type;
  static constexpr int planes = 1;
  static __device__ __forceinline__ T load(const T* __restrict__ p, long plane, long off) { return p[off]; }
};

struct SlClippedLuma {  // no Y map is written
  typedef float type;
  static constexpr int planes = 3;
  static __device__ __forceinline__ float load(const float* __restrict__ p, long plane, long off) {
    return sl_clip_luma(p[off], p[plane + off], p[2 * plane + off]);
  }
};

template <typename LOAD, typename PIXEL, bool GRAD>
__global__ __launch_bounds__(64) void sl_fwd_kernel(const typename LOAD::type* __restrict__ a,
                                                    const typename LOAD::type* __restrict__ b, int h, int w, int tiles_x,
                                                    int tiles_per_plane, double c1, double c2, SsimLossTaps tp,
                                                    double* __restrict__ part, double* __restrict__ ma,
                                                    double* __restrict__ mb, double* __restrict__ mg) {
  typedef typename LOAD::type T;
  __shared__ T sx[2][SL_SW], sy[2][SL_SW];
  const int plane_i = blockIdx.x / tiles_per_plane, t = blockIdx.x - plane_i * tiles_per_plane;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int lane = threadIdx.x;
  const int c0 = tx * SL_TW, r0 = ty * SL_TH;
  const int hw = h - 2 * SL_R, ww = w - 2 * SL_R;              // the window grid
  const int n_in = min(SL_TH, hw - r0) + 2 * SL_R;             // input rows r0 .. r0 + n_in - 1, all < h
  const long plane = (long)h * w;
  const T* pa = a + (long)plane_i * LOAD::planes * plane;
  const T* pb = b + (long)plane_i * LOAD::planes * plane;
  // staged columns: c0 + lane, and c0 + 64 + lane on the first 10 lanes; clamped into the image on a right-edge tile,
  // where those values only reach windows that are not output
  const long col0 = min(c0 + lane, w - 1), col1 = min(c0 + SL_TW + lane, w - 1);
  const bool halo = lane < 2 * SL_R;
  const bool out_col = c0 + lane < ww;
  const long mbase = (long)plane_i * hw * ww + c0 + lane;      // + row * ww: this lane's window in the maps

  long off = (long)r0 * w;
  T x0 = LOAD::load(pa, plane, off + col0), y0 = LOAD::load(pb, plane, off + col0);
  T x1 = 0, y1 = 0;
  if (halo) {
    x1 = LOAD::load(pa, plane, off + col1);
    y1 = LOAD::load(pb, plane, off + col1);
  }

  double rx[SL_K], ry[SL_K], rxx[SL_K], ryy[SL_K], rxy[SL_K];  // horizontal sums of the last 11 rows
  double acc = 0.0;
  for (int i0 = 0; i0 < n_in; i0 += SL_K) {
#pragma unroll
    for (int j = 0; j < SL_K; ++j) {  // input row i = i0 + j sits in ring slot j
      const int i = i0 + j;
      if (i < n_in) {
        T* bx = sx[i & 1];
        T* by = sy[i & 1];
        bx[lane] = x0;
        by[lane] = y0;
        if (halo) {
          bx[SL_TW + lane] = x1;
          by[SL_TW + lane] = y1;
        }
        __syncthreads();
        if (i + 1 < n_in) {  // the next row's loads fly while this one is filtered
          off += w;
          x0 = LOAD::load(pa, plane, off + col0);
          y0 = LOAD::load(pb, plane, off + col0);
          if (halo) {
            x1 = LOAD::load(pa, plane, off + col1);
            y1 = LOAD::load(pb, plane, off + col1);
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
          const double s = PIXEL::template pixel<GRAD>(mx, my, mxx, myy, mxy, c1, c2, al, be, ga);
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

// sl_fwd_kernel on planes as given, with the maps when a gradient is wanted
template <typename T, typename PIXEL>
static void sl_launch_fwd(bool want_grad, unsigned blocks, hipStream_t s, const T* a, const T* b, int h, int w, double c1,
                          double c2, const SsimLossTaps& tp, double* part, double* ma, double* mb, double* mg) {
  const int tx = (int)sl_win_tiles_x(w), wt = (int)sl_win_tiles(h, w);
  if (want_grad)
    hipLaunchKernelGGL((sl_fwd_kernel<SlPlane<T>, PIXEL, true>), dim3(blocks), dim3(64), 0, s, a, b, h, w, tx, wt, c1, c2, tp,
                       part, ma, mb, mg);
  else
    hipLaunchKernelGGL((sl_fwd_kernel<SlPlane<T>, PIXEL, false>), dim3(blocks), dim3(64), 0, s, a, b, h, w, tx, wt, c1, c2, tp,
                       part, (double*)nullptr, (double*)nullptr, (double*)nullptr);
}

// One wave per tile of 64 x 32 pixels of one plane.  Window row i = r0 - 10 + ii, ii = 0 .. n_in - 1, is staged (columns
// c0 - 10 .. c0 + 63 of the window grid, zero outside it), filtered horizontally for this lane's pixel column into ring slot
// ii % 11; pixel row r = r0 + ii - 10 then reads window rows r - 10 .. r from the ring with tap r - i.  The pixel's
// G^T alpha + 2 x G^T beta + y G^T gamma is scaled by SCALE; with PARENT a quarter of the parent pixel of the next coarser
// scale's gradient (hp x wp; pixels of a dropped odd row or column have no parent) is added.
template <typename T, typename O, typename SCALE, bool PARENT>
__global__ __launch_bounds__(64) void sl_grad_kernel(const T* __restrict__ a, const T* __restrict__ b, int h, int w,
                                                     int tiles_x, int tiles_per_plane, SCALE scale, SsimLossTaps tp,
                                                     const double* __restrict__ ma, const double* __restrict__ mb,
                                                     const double* __restrict__ mg, const double* __restrict__ parent,
                                                     int hp, int wp, O* __restrict__ grad) {
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
  const T* pa = a + (long)plane_i * h * w;
  const T* pb = b + (long)plane_i * h * w;
  O* pg = grad + (long)plane_i * h * w;
  const double f = scale.of(plane_i);
  // the parent's column; in range where has_parent
  const bool has_parent = PARENT && out_col && (int)(pcol >> 1) < wp;
  const double* pp = PARENT ? parent + (long)plane_i * hp * wp + (has_parent ? (pcol >> 1) : 0) : nullptr;

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
          const int r = r0 + ii - 2 * SL_R;  // < h by n_out
          const long p = (long)r * w + pcol;
          const double xv = (double)pa[p], yv = (double)pb[p];
          double d = SCALE::apply(f, va + 2.0 * xv * vb + yv * vg);
          if (PARENT) {
            if (has_parent && (r >> 1) < hp) d += 0.25 * pp[(long)(r >> 1) * wp];
          }
          if (out_col) pg[p] = (O)d;
        }
      }
    }
  }
}

// out[b] = (sum of part[b * n .. b * n + n - 1], in a fixed order) / divisor, rounded to O once
template <typename O>
__global__ __launch_bounds__(256) void sl_finish_kernel(const double* __restrict__ part, long n, double divisor,
                                                        O* __restrict__ out) {
  __shared__ double red[256];
  const double* p = part + (long)blockIdx.x * n;
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) s += p[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = (O)(red[0] / divisor);
}
