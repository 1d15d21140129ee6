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
// Entry point sisr_ssim_loss: planes as given -> the fp32 value and, with `grad`, the fp32 gradient.  Launches, all kernels of
// csrc/ssim_window.h (no atomics anywhere: a repeat call is bit-identical; no allocation, no host synchronisation):
//   sl_fwd_kernel     LOAD = SlPlane<float>, PIXEL = SlSsim; the tile sums of S and, when a gradient is wanted, the maps
//   sl_finish_kernel  one block adds all tile sums in a fixed order, divides by the count and rounds to fp32 once
//   sl_grad_kernel    SCALE = SlDivideByCount: the pixel's sum divided by the count, one fp32 store per pixel
// The window statistics, S and the three maps are float64.  The maps are float64 in memory too: near convergence the three
// terms of the gradient are O(1 / B2) each and cancel down to O(|x - y| / B2), so maps rounded to fp32 (6e-8 relative) would
// put back, at |x - y| ~ 2e-3, the 3e-5 relative error of an fp32 composition that this kernel exists to avoid.
#include "sisr_common.h"
#include "ssim_window.h"
#include <math.h>

// the last step of d(mean S)/dx is a division by the count: a multiplication by its reciprocal rounds differently
struct SlDivideByCount {
  double count;
  __device__ __forceinline__ double of(int) const { return count; }
  static __device__ __forceinline__ double apply(double count, double g) { return g / count; }
};

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
  sl_launch_fwd<float, SlSsim>(grad != nullptr, (unsigned)(planes * wt), s, sr, y, h, w, c1, c2, tp, part, ma, mb, mg);
  int rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(sl_finish_kernel<float>, dim3(1), dim3(256), 0, s, part, (long)planes * wt, count, value);
  rc = sisr_check_launch();
  if (rc || !grad) return rc;
  hipLaunchKernelGGL((sl_grad_kernel<float, float, SlDivideByCount, false>), dim3((unsigned)(planes * pt)), dim3(64), 0, s, sr,
                     y, h, w, (int)sl_pix_tiles_x(w), (int)pt, SlDivideByCount{count}, tp, ma, mb, mg, (const double*)nullptr, 0,
                     0, grad);
  return sisr_check_launch();
}
