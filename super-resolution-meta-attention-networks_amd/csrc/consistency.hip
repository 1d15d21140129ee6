// The degradation as a differentiable float operator: blur + Pillow's bicubic down-sampling by s = 2, 3, 4,
// away from the image border, is ONE per-sample stride-s cross-correlation with a composed kernel K = (w w^T) * k of edge
// n = taps + l - 1 (degrade.compose_degradation, float64 on the host):
//   y[b][c][i][j]  = sum_ef K[b][e][f] x[b][c][s i + off + e][s j + off + f]          0 <= i < ho, 0 <= j < wo   (forward)
//   dx[b][c][p][q] = sum_ij K[b][p - off - s i][q - off - s j] g[b][c][i][j]          0 <= p < H,  0 <= q < W    (adjoint)
// The channels do not mix, so this is vector-ALU work.  Both kernels accumulate in float64 over the float64 K in a fixed
// order and round once: the result is the fp32 number nearest the exact sum over the fp32 operands, which no fp32
// composition of the three steps can beat -- the accuracy condition of the tests (at most twice the error of the stock fp32
// composition) holds element by element, whatever the shape.  fp64 FMAs run at half the fp32 vector rate on gfx950; the
// kernels are bound by their LDS reads either way.  No atomics, no memset: repeated runs are bit-identical and every element
// of dx is written exactly once.
#include "sisr_common.h"

#define CT_FWD 16             // forward: LR outputs per workgroup edge (one output per thread)
#define CT_BWD 32             // adjoint: HR pixels per workgroup edge (four pixels per thread)
#define CT_NMAX 36            // largest composed kernel edge: 16 taps (s = 4) + 21 - 1
#define CT_GMAX 32            // adjoint: largest edge of the block of outputs whose footprints reach one HR tile
#define CT_LDS_MAX 65536      // forward: dynamic LDS the launch may ask for without an opt-in

// Forward.  The HR window of the workgroup's CT_FWD x CT_FWD outputs, (S (CT_FWD - 1) + n)^2 pixels, is staged in LDS split
// by column phase: xs[q % S][r][q / S] with row pitch `pitch`.  For one tap (e, f) the 16 lanes of an output row then read 16
// consecutive dwords, and the host picks the pitch with S * pitch = 16 (mod 32), so the second output row of a 32-lane group
// lands on the other 16 banks: conflict-free ds_read_b32.  K[b] is addressed uniformly over the workgroup (scalar loads).
template <int S>
__global__ __launch_bounds__(256) void degrade_valid_fwd_kernel(const float* __restrict__ x, const double* __restrict__ K,
                                                                float* __restrict__ y, int C, int H, int W, int n, int off,
                                                                int ho, int wo, int pitch) {
  extern __shared__ float xs[];
  const int bc = blockIdx.z, b = bc / C;
  const int i0 = blockIdx.y * CT_FWD, j0 = blockIdx.x * CT_FWD;
  const int edge = S * (CT_FWD - 1) + n;  // rows = columns of the window
  const int r0 = S * i0 + off, q0 = S * j0 + off;
  const float* xp = x + (long)bc * H * W;
  for (int t = threadIdx.x; t < edge * edge; t += 256) {
    const int r = t / edge, q = t - r * edge;
    const int gr = r0 + r, gq = q0 + q;
    // rows / columns past the image belong to outputs past ho / wo only (the host checks S (ho - 1) + off + n <= H)
    const float v = (gr < H && gq < W) ? xp[(long)gr * W + gq] : 0.f;
    xs[((q % S) * edge + r) * pitch + q / S] = v;
  }
  __syncthreads();
  const int r = threadIdx.x / CT_FWD, c = threadIdx.x % CT_FWD;
  if (i0 + r >= ho || j0 + c >= wo) return;
  const double* Kb = K + (long)b * n * n;
  double acc = 0.0;
  for (int e = 0; e < n; ++e) {
    const float* row = xs + (S * r + e) * pitch + c;
    const double* Ke = Kb + e * n;
#pragma unroll
    for (int ph = 0; ph < S; ++ph) {
      const float* rp = row + ph * edge * pitch;
      for (int f = ph, t = 0; f < n; f += S, ++t) acc = __builtin_fma((double)rp[t], Ke[f], acc);
    }
  }
  y[((long)bc * ho + i0 + r) * wo + j0 + c] = (float)acc;
}

__device__ __forceinline__ int ct_floor_div(int a, int s) { return a >= 0 ? a / s : -((-a + s - 1) / s); }

// Adjoint, as a gather (the polyphase form): HR pixel (p, q) sums the outputs (i, j) with 0 <= p - off - S i < n and
// 0 <= q - off - S j < n, at most ceil(n / S)^2 of them, in ascending (i, j).  The outputs that reach the workgroup's
// CT_BWD x CT_BWD pixels and the sample's K sit in LDS; lanes along q read the same g for S neighbours (broadcast) and S
// neighbouring doubles of K.  Pixels no footprint reaches are stored as zeros by the same code path.
template <int S>
__global__ __launch_bounds__(256) void degrade_valid_bwd_kernel(const float* __restrict__ g, const double* __restrict__ K,
                                                                float* __restrict__ dx, int C, int H, int W, int n, int off,
                                                                int ho, int wo) {
  __shared__ double Ks[CT_NMAX * CT_NMAX];
  __shared__ float gs[CT_GMAX * CT_GMAX];
  const int bc = blockIdx.z, b = bc / C;
  const int p0 = blockIdx.y * CT_BWD, q0 = blockIdx.x * CT_BWD;
  // outputs whose footprint holds a row of p0 .. p0 + CT_BWD - 1:  ceil((p0 - off - n + 1) / S) <= i <= floor((p0 + CT_BWD - 1 - off) / S)
  const int ia = max(ct_floor_div(p0 - off - n + S, S), 0), ib = min(ct_floor_div(p0 + CT_BWD - 1 - off, S), ho - 1);
  const int ja = max(ct_floor_div(q0 - off - n + S, S), 0), jb = min(ct_floor_div(q0 + CT_BWD - 1 - off, S), wo - 1);
  const int gh = ib - ia + 1, gw = jb - ja + 1;  // <= (CT_BWD + n - 2) / S + 1 <= CT_GMAX (checked on the host); may be <= 0
  const double* Kb = K + (long)b * n * n;
  for (int t = threadIdx.x; t < n * n; t += 256) Ks[t] = Kb[t];
  if (gh > 0 && gw > 0) {
    const float* gp = g + (long)bc * ho * wo;
    for (int t = threadIdx.x; t < gh * gw; t += 256) {
      const int r = t / gw, c = t - r * gw;
      gs[r * CT_GMAX + c] = gp[(long)(ia + r) * wo + ja + c];
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < CT_BWD * CT_BWD; t += 256) {
    const int p = p0 + t / CT_BWD, q = q0 + t % CT_BWD;
    if (p >= H || q >= W) continue;
    const int pp = p - off, qq = q - off;
    const int ilo = max(ct_floor_div(pp - n + S, S), ia), ihi = min(ct_floor_div(pp, S), ib);
    const int jlo = max(ct_floor_div(qq - n + S, S), ja), jhi = min(ct_floor_div(qq, S), jb);
    double acc = 0.0;
    for (int i = ilo; i <= ihi; ++i) {
      const double* Ke = Ks + (pp - S * i) * n + qq;
      const float* gr = gs + (i - ia) * CT_GMAX;
      for (int j = jlo; j <= jhi; ++j) acc = __builtin_fma((double)gr[j - ja], Ke[-S * j], acc);
    }
    dx[((long)bc * H + p) * W + q] = (float)acc;
  }
}

// edge of a workgroup's tile: LR outputs (forward) or HR pixels (adjoint)
extern "C" int sisr_degrade_valid_tile(int backward) { return backward ? CT_BWD : CT_FWD; }

static int ct_check(const void* a, const void* K, const void* c, int B, int C, int H, int W, int n, int scale, int off, int ho,
                    int wo) {
  if (!a || !K || !c || B < 1 || C < 1 || H < 1 || W < 1 || n < 1 || off < 0 || ho < 1 || wo < 1) return SISR_ERR_ARG;
  if (scale < 2 || scale > 4) return SISR_ERR_UNSUPPORTED;
  // every footprint inside the image: the kernels take this for granted
  if ((long)scale * (ho - 1) + off + n > H || (long)scale * (wo - 1) + off + n > W) return SISR_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(a) & 3) || (reinterpret_cast<uintptr_t>(c) & 3) || (reinterpret_cast<uintptr_t>(K) & 7))
    return SISR_ERR_ALIGN;
  if (n > CT_NMAX || (long)B * C > 65535) return SISR_ERR_UNSUPPORTED;
  return SISR_OK;
}

extern "C" int sisr_degrade_valid_fwd(const float* x, const double* K, float* y, int B, int C, int H, int W, int n, int scale,
                                      int off, int ho, int wo, void* stream) {
  const int rc = ct_check(x, K, y, B, C, H, W, n, scale, off, ho, wo);
  if (rc != SISR_OK) return rc;
  const int edge = scale * (CT_FWD - 1) + n;
  int pitch = (edge + scale - 1) / scale;
  while ((scale * pitch) % 32 != 16) ++pitch;
  const size_t lds = (size_t)scale * edge * pitch * sizeof(float);
  const dim3 grid((wo + CT_FWD - 1) / CT_FWD, (ho + CT_FWD - 1) / CT_FWD, B * C);
  if (lds > CT_LDS_MAX || grid.y > 65535) return SISR_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (scale == 2) hipLaunchKernelGGL(degrade_valid_fwd_kernel<2>, grid, dim3(256), lds, st, x, K, y, C, H, W, n, off, ho, wo, pitch);
  else if (scale == 3) hipLaunchKernelGGL(degrade_valid_fwd_kernel<3>, grid, dim3(256), lds, st, x, K, y, C, H, W, n, off, ho, wo, pitch);
  else hipLaunchKernelGGL(degrade_valid_fwd_kernel<4>, grid, dim3(256), lds, st, x, K, y, C, H, W, n, off, ho, wo, pitch);
  return sisr_check_launch();
}

extern "C" int sisr_degrade_valid_bwd(const float* g, const double* K, float* dx, int B, int C, int H, int W, int n, int scale,
                                      int off, int ho, int wo, void* stream) {
  const int rc = ct_check(g, K, dx, B, C, H, W, n, scale, off, ho, wo);
  if (rc != SISR_OK) return rc;
  const dim3 grid((W + CT_BWD - 1) / CT_BWD, (H + CT_BWD - 1) / CT_BWD, B * C);
  if ((CT_BWD + n - 2) / scale + 1 > CT_GMAX || grid.y > 65535) return SISR_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (scale == 2) hipLaunchKernelGGL(degrade_valid_bwd_kernel<2>, grid, dim3(256), 0, st, g, K, dx, C, H, W, n, off, ho, wo);
  else if (scale == 3) hipLaunchKernelGGL(degrade_valid_bwd_kernel<3>, grid, dim3(256), 0, st, g, K, dx, C, H, W, n, off, ho, wo);
  else hipLaunchKernelGGL(degrade_valid_bwd_kernel<4>, grid, dim3(256), 0, st, g, K, dx, C, H, W, n, off, ho, wo);
  return sisr_check_launch();
}
