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
// Entry point sisr_ssim: n images of 1 or 3 planes -> n float64 values.  Two launches, both kernels of csrc/ssim_window.h:
//   sl_fwd_kernel     LOAD = SlPlane<float> (channels == 1) or SlClippedLuma (channels == 3: clipped and converted to Y on
//                     the way into LDS), PIXEL = SlSsim, no maps; per-tile sums of S go to the workspace in tile order
//   sl_finish_kernel  one block per image adds its tile sums in a fixed order and divides by the window count
// Workspace: [n][window tiles] float64.  No atomics: a repeat launch is bit-identical.
#include "sisr_common.h"
#include "ssim_window.h"
#include <math.h>

extern "C" size_t sisr_ssim_workspace_bytes(int n, int h, int w) {
  if (n <= 0 || h < SL_K || w < SL_K) return 0;
  return (size_t)n * (size_t)sl_win_tiles(h, w) * sizeof(double);
}

extern "C" int sisr_ssim(const float* a, const float* b, int n, int channels, int h, int w, double data_range,
                         double* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!a || !b || !out || !workspace || n <= 0 || h < SL_K || w < SL_K || (channels != 1 && channels != 3) ||
      !isfinite(data_range) || !(data_range > 0.0))
    return SISR_ERR_ARG;
  if (workspace_bytes < sisr_ssim_workspace_bytes(n, h, w)) return SISR_ERR_ARG;
  const long tiles = sl_win_tiles(h, w);
  if ((long)n * tiles > 0x7fffffffL) return SISR_ERR_UNSUPPORTED;
  const SsimLossTaps tp = sl_make_taps();
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  double* part = static_cast<double*>(workspace);
  const hipStream_t s = (hipStream_t)stream;
  double* const no_map = nullptr;
  if (channels == 3)
    hipLaunchKernelGGL((sl_fwd_kernel<SlClippedLuma, SlSsim, false>), dim3((unsigned)(n * tiles)), dim3(64), 0, s, a, b, h, w,
                       (int)sl_win_tiles_x(w), (int)tiles, c1, c2, tp, part, no_map, no_map, no_map);
  else
    hipLaunchKernelGGL((sl_fwd_kernel<SlPlane<float>, SlSsim, false>), dim3((unsigned)(n * tiles)), dim3(64), 0, s, a, b, h, w,
                       (int)sl_win_tiles_x(w), (int)tiles, c1, c2, tp, part, no_map, no_map, no_map);
  int rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(sl_finish_kernel<double>, dim3((unsigned)n), dim3(256), 0, s, part, tiles,
                     (double)(h - 2 * SL_R) * (double)(w - 2 * SL_R), out);
  return sisr_check_launch();
}
