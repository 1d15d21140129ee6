// The optimiser step's optional parts over the flat arenas of optim.FlatAdam (no counterpart in the reference, whose step is
// plain Adam behind a host-side clip): the global gradient norm and its clip coefficient, and the Adam pass of
// csrc/misc.hip extended by a device-side gradient scale, decoupled (AdamW) weight decay and an exponential moving average
// of the weights.  All of them are single-pass HBM-bound streams of plain 16-byte vector loads and stores.
//
//   norm   S = sum g^2 over the ranges the step updates, every product and sum in double (the product of two floats is exact
//          in double), two stages, no atomics:  norm = sqrt(S);  coef = min(1, max_norm / (norm + 1e-6))
//          (torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False); the coefficient is computed in double, rounded once)
//   update gg = g grad_scale [* *grad_scale_dev];  p = p decay_factor;  then adam_flat_kernel's lines on gg;
//          [e = e + (p_new - e) one_minus_decay]
//   ema    e = e + (p - e) one_minus_decay alone, for the ranges Adam skips in a step
//
// Determinism of the norm: a range of n floats is always cut over sumsq_blocks(n) workgroups in the same grid-stride
// pattern, a thread adds its products in rising address order, the 256 thread sums of a workgroup meet in a fixed tree, and
// the final workgroup adds the partials p[t], p[t + 256], ... per thread in rising order and joins them by the same tree.
// Nothing depends on which workgroup finishes first, so two calls on the same data give the same bits.
#include "sisr_common.h"

#define SUMSQ_BLOCKS 1024

static inline long sumsq_blocks(long n) {
  long blocks = ((n >> 2) + 255) / 256;
  if (blocks > SUMSQ_BLOCKS) blocks = SUMSQ_BLOCKS;
  return blocks < 1 ? 1 : blocks;
}

__device__ __forceinline__ double block_sum256(double s, double* red) {  // red: 256 doubles of LDS; the result in thread 0
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

__global__ __launch_bounds__(256) void sumsq_partial_kernel(const float* __restrict__ g, long n4, long n,
                                                            double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 x = reinterpret_cast<const f32x4*>(g)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (double)x[e] * (double)x[e];
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail
    const double x = g[(n4 << 2) + threadIdx.x];
    s += x * x;
  }
  s = block_sum256(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void clip_coef_kernel(const double* __restrict__ part, long nparts, double max_norm,
                                                        double* __restrict__ norm64, float* __restrict__ norm32,
                                                        float* __restrict__ coef) {
  __shared__ double red[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < nparts; i += 256) s += part[i];
  s = block_sum256(s, red);
  if (threadIdx.x == 0) {
    const double norm = sqrt(s);
    const double c = max_norm / (norm + 1e-6);
    *norm64 = norm;
    *norm32 = (float)norm;
    *coef = (float)(c > 1.0 ? 1.0 : c);  // not fmin: a NaN norm stays a NaN coefficient, as torch.clamp(max=1) keeps it
  }
}

extern "C" size_t sisr_sumsq_workspace_bytes(long n) { return n > 0 ? (size_t)sumsq_blocks(n) * sizeof(double) : 0; }

extern "C" int sisr_sumsq_partial(const float* g, long n, double* part, void* stream) {
  if (!g || !part || n <= 0) return SISR_ERR_ARG;
  if (!sisr_aligned16(g) || (reinterpret_cast<uintptr_t>(part) & 7)) return SISR_ERR_ALIGN;
  hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)sumsq_blocks(n)), dim3(256), 0, (hipStream_t)stream, g, n >> 2, n,
                     part);
  return sisr_check_launch();
}

extern "C" int sisr_clip_coef(const double* part, long nparts, double max_norm, double* norm64, float* norm32, float* coef,
                              void* stream) {
  if (!part || !norm64 || !norm32 || !coef || nparts <= 0 || !(max_norm > 0.0)) return SISR_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(part) & 7) || (reinterpret_cast<uintptr_t>(norm64) & 7)) return SISR_ERR_ALIGN;
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, part, nparts, max_norm, norm64, norm32,
                     coef);
  return sisr_check_launch();
}

// adam_flat_kernel (csrc/misc.hip) with the three additions; with gdev == nullptr, decay == 1 (p * 1.0f is exact) and
// ema == nullptr every element goes through the same roundings in the same order as there.
__global__ __launch_bounds__(256) void update_flat_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          float* __restrict__ ema, long n4, long n, float b2, float omb1,
                                                          float omb2, float eps, float step_size, float bc2_sqrt,
                                                          float gscale, const float* __restrict__ gdev, float decay,
                                                          float omd) {
#pragma clang fp contract(off)
  const bool scaled = gdev != nullptr;
  const float gs2 = scaled ? *gdev : 1.0f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    f32x4 gg = reinterpret_cast<const f32x4*>(g)[i] * gscale;
    if (scaled) gg = gg * gs2;
    f32x4 mm = reinterpret_cast<f32x4*>(m)[i];
    f32x4 vv = reinterpret_cast<f32x4*>(v)[i];
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i] * decay;
    mm = mm + (gg - mm) * omb1;
    vv = vv * b2 + gg * gg * omb2;
#pragma unroll
    for (int e = 0; e < 4; ++e) pp[e] = pp[e] - step_size * (mm[e] / (sqrtf(vv[e]) / bc2_sqrt + eps));
    reinterpret_cast<f32x4*>(m)[i] = mm;
    reinterpret_cast<f32x4*>(v)[i] = vv;
    reinterpret_cast<f32x4*>(p)[i] = pp;
    if (ema) {
      f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
      reinterpret_cast<f32x4*>(ema)[i] = ee + (pp - ee) * omd;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail
    const long i = (n4 << 2) + threadIdx.x;
    float gg = g[i] * gscale;
    if (scaled) gg = gg * gs2;
    const float mm = m[i] + (gg - m[i]) * omb1;
    const float vv = v[i] * b2 + gg * gg * omb2;
    const float pp = p[i] * decay - step_size * (mm / (sqrtf(vv) / bc2_sqrt + eps));
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
    if (ema) ema[i] = ema[i] + (pp - ema[i]) * omd;
  }
}

__global__ __launch_bounds__(256) void ema_flat_kernel(const float* __restrict__ p, float* __restrict__ ema, long n4, long n,
                                                       float omd) {
#pragma clang fp contract(off)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
    const f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
    reinterpret_cast<f32x4*>(ema)[i] = ee + (pp - ee) * omd;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail
    const long i = (n4 << 2) + threadIdx.x;
    ema[i] = ema[i] + (p[i] - ema[i]) * omd;
  }
}

static inline unsigned stream_blocks(long n4) {  // the grid of sisr_adam_flat
  long blocks = (n4 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int sisr_update_flat(float* p, const float* g, float* m, float* v, float* ema, long n, float beta2,
                                float one_minus_beta1, float one_minus_beta2, float eps, float step_size, float bc2_sqrt,
                                float grad_scale, const float* grad_scale_dev, float decay_factor, float one_minus_decay,
                                void* stream) {
  if (!p || !g || !m || !v || n <= 0) return SISR_ERR_ARG;
  if (!sisr_aligned16(p) || !sisr_aligned16(g) || !sisr_aligned16(m) || !sisr_aligned16(v) || !sisr_aligned16(ema))
    return SISR_ERR_ALIGN;
  if (reinterpret_cast<uintptr_t>(grad_scale_dev) & 3) return SISR_ERR_ALIGN;
  const long n4 = n >> 2;
  hipLaunchKernelGGL(update_flat_kernel, dim3(stream_blocks(n4)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n4, n,
                     beta2, one_minus_beta1, one_minus_beta2, eps, step_size, bc2_sqrt, grad_scale, grad_scale_dev,
                     decay_factor, one_minus_decay);
  return sisr_check_launch();
}

extern "C" int sisr_ema_flat(const float* p, float* ema, long n, float one_minus_decay, void* stream) {
  if (!p || !ema || n <= 0) return SISR_ERR_ARG;
  if (!sisr_aligned16(p) || !sisr_aligned16(ema)) return SISR_ERR_ALIGN;
  const long n4 = n >> 2;
  hipLaunchKernelGGL(ema_flat_kernel, dim3(stream_blocks(n4)), dim3(256), 0, (hipStream_t)stream, p, ema, n4, n,
                     one_minus_decay);
  return sisr_check_launch();
}
