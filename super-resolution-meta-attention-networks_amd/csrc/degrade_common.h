// Pixel arithmetic shared by the whole-image degradation kernels (degrade.hip) and the tile-level ones (degrade_tiles.hip):
// both must give the same bytes for the same pixel, so the index rule and the two quantisations live here once.
#pragma once
#include "sisr_common.h"

#define BL_MAX 21             // largest blur kernel edge (reference default and maximum used: 21)

// nn.ReflectionPad2d: -1 -> 1, n -> n-2.  Clamped into the image: the staged tile of an edge block reaches past the
// reflection of rows / columns no output of the block reads (more than l - 1 - l / 2 beyond the image), where one
// reflection leaves an index below 0; every index an output does read lies within one reflection and is unchanged.
__device__ __forceinline__ int reflect_index(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return min(max(i, 0), n - 1);
}

// ToPILImage's `mul(255).byte()` on the blurred value: truncation
__device__ __forceinline__ unsigned char dg_quant(float blur) { return (unsigned char)(int)(blur * 255.0f); }

// b_GaussianNoising + clamp + the same quantisation: product and sum rounded separately, as torch's mul / add are
__device__ __forceinline__ unsigned char dg_noise_quant(float blur, float noise, float sigma) {
  float v = __fadd_rn(__fmul_rn(noise, sigma), blur);
  v = fminf(fmaxf(v, 0.f), 1.f);
  return (unsigned char)(int)(v * 255.0f);
}

// One output of a PIL resample pass from its 22-bit fixed-point sum (rounding constant included): clip8(ss >> 22)
__device__ __forceinline__ int dg_clip8(int ss) {
  const int v = ss >> 22;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The store map of the tile kernels (degrade_tiles.hip, interp_tiles.hip), sisr_crop_augment's index map restricted to a c x c
// tile: destination (i, j) in the augmented tile of source-orientation pixel (ry, rx); flips: 1 hflip, 2 vflip, 4 transpose
__device__ __forceinline__ long dt_store_index(int ry, int rx, int c, int flips) {
  const int a = (flips & 2) ? c - 1 - ry : ry, b = (flips & 1) ? c - 1 - rx : rx;
  return (flips & 4) ? (long)b * c + a : (long)a * c + b;
}
