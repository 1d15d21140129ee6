// The 11 x 11 Gaussian window of the SSIM training terms (csrc/ssim_loss.hip, csrc/ms_ssim.hip): its taps, the tiling of the
// window and pixel grids by one wave per 64 x 32 tile, and S with the three coefficients of its differential.
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

// scipy.ndimage._gaussian_kernel1d(1.5, 0, 5), as sisr_ssim forms it: exp(-0.5 / sigma^2 * x^2), normalised by numpy's
// sum of 11 terms (eight running partials paired up, then the last three added in order)
static inline SsimLossTaps sl_make_taps() {
  SsimLossTaps tp;
  const double f = -0.5 / (1.5 * 1.5);
  for (int k = 0; k < SL_K; ++k) tp.w[k] = exp(f * (double)((k - SL_R) * (k - SL_R)));
  double sum = ((tp.w[0] + tp.w[1]) + (tp.w[2] + tp.w[3])) + ((tp.w[4] + tp.w[5]) + (tp.w[6] + tp.w[7]));
  for (int k = 8; k < SL_K; ++k) sum += tp.w[k];
  for (int k = 0; k < SL_K; ++k) tp.w[k] /= sum;
  return tp;
}

// S in scikit-image's operation order (the order of ssim_pixel in metrics.hip: symmetric, so S(x, x) is exactly 1), and
// the three coefficients of its differential
template <bool GRAD>
__device__ __forceinline__ double sl_pixel(double mx, double my, double mxx, double myy, double mxy, double c1, double c2,
                                           double& alpha, double& beta, double& gamma) {
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
