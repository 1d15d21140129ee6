// SRCNN / VDSR building blocks: K x K convolutions (odd K <= 9, padding K/2), the one-channel (luminance) image ends and
// the MSE loss, fp32.  ref: Code/SISR/models/basic/architectures.py (SRCNN, VDSR), basic/handlers.py (nn.MSELoss).
//
// Maps between layers are channels-last with CP = 32 or 64 channels (zero-padded); the image ends are planar (B,1,H,W).
//
//   sisr_convk_y2f     planar Y -> CP-channel map on the VALU: one thread per pixel, all CP outputs in registers, the haloed
//                      input tile and the K^2 x CP weights in LDS, 16-byte stores.  With flip_taps (and an optional mask)
//                      it is the input gradient of sisr_convk_f2y.
//   sisr_convk_f2y     CP-channel map -> planar Y (+ bias, + residual): the haloed tile is staged 16 channels at a time.
//   sisr_corrk_y       weight / bias gradient of both ends: dw[c][kh][kw] = sum_pix P[pix + s (k - K/2)] * Q[pix][c] with a
//                      planar P and a channels-last Q; ordered two-stage sum (per-block partials, then one ordered pass).
//   sisr_convk_mfma    K x K conv between channels-last maps on v_mfma_f32_32x32x2_f32 (implicit GEMM: M = 32 pixels of a row,
//                      N = 32 output channels, contraction over K^2 x Cin).  The haloed input tile is staged 32 channels at
//                      a time; the weights are streamed per tap from the packed buffer (sisr_pack_convk), which stays in L2.
//                      The same kernel is the input gradient when given the 'dgrad' packing (taps flipped, roles swapped).
//   sisr_wgradk_mfma   its weight gradient: per (tap, 32 input channels, pixel slice) workgroup, M = Cout, N = 32 input
//                      channels, contraction over pixels; slices are summed in order by a second pass.
//   sisr_mse_loss      mean squared difference and its gradient 2 (a - b) / n in the same launch (ordered two-stage sum).
//   sisr_convk_mfma_leaky, sisr_wgradk_mfma_leaky   the two MFMA kernels with LeakyReLU(slope) in place of ReLU: the forward
//                      epilogue selects v > 0 ? v : slope * v, the gradient forms read dy as m > 0 ? dy : slope * dy through
//                      the layer's saved output m (one more template flag; the ReLU forms keep their own selects).
//   sisr_map_mean, sisr_map_mean_bwd   global mean of a map's real channels (ordered two-stage float64 sum) and its gradient:
//                      the degradation predictor's head (predictor.py).
//   sisr_convk_s2_mfma_leaky, sisr_dgradk_s2_mfma_leaky, sisr_wgradk_s2_mfma_leaky   the stride-2 conv (padding K/2) and its
//                      gradients: a forward kernel that forms only its own outputs' products, the transposed conv as four
//                      stride-1 phases, and the weight-gradient kernel with a strided x index (IKC's predictor).
//
// Within a lane the contraction index of the 32x32x2 MFMA is permuted (lane half h takes channels 16 h + kk at step kk), so
// both operands are read 16 bytes at a time; A and B use the same permutation, so the sum is over the same products.
#include "sisr_common.h"

#define BK_TH 8    // pixel tile: 8 rows x 32 columns, 256 threads
#define BK_TW 32
#define BK_MAXK 9
#define BK_PARTS 1024  // at most this many partial sums per reduced value (four workgroups per CU)
#define BK_XS 36       // LDS pixel stride (floats) of the 32-channel MFMA tile: 32 + 4, keeps 16-byte reads aligned
#define BK_FS 20       // LDS pixel stride of the 16-channel f2y tile

static inline bool bk_k_ok(int K) { return K >= 1 && K <= BK_MAXK && (K & 1); }
static inline bool bk_cp_ok(int cp) { return cp == 32 || cp == 64; }
static inline bool bk_dims_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && B <= 65535 && (long)B * H * W <= (1L << 28);
}
static inline int bk_s2_out(int n) { return (n - 1) / 2 + 1; }  // output size of a stride-2 conv with padding K / 2, K odd

// ------------------------------------------------------------------------------------------------ Y -> features
template <int CP>
__global__ __launch_bounds__(256) void bk_y2f_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ mask,
                                                     float* __restrict__ y, int H, int W, int K, int cout, int relu, int flip) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int p = K / 2, LW = BK_TW + K - 1, LH = BK_TH + K - 1, KK = K * K;
  float* ws = lds;                 // [KK][CP]
  float* bs = ws + KK * CP;        // [CP]
  float* xs = bs + CP;             // [LH][LW]
  const int tid = threadIdx.x, b = blockIdx.z, h0 = blockIdx.y * BK_TH, w0 = blockIdx.x * BK_TW;
  for (int i = tid; i < LH * LW; i += 256) {
    const int hh = h0 + i / LW - p, ww = w0 + i % LW - p;
    xs[i] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? x[((long)b * H + hh) * W + ww] : 0.f;
  }
  for (int i = tid; i < KK * CP; i += 256) {
    const int tap = i / CP, c = i % CP;
    ws[i] = c < cout ? w[c * KK + (flip ? KK - 1 - tap : tap)] : 0.f;
  }
  if (tid < CP) bs[tid] = (bias && tid < cout) ? bias[tid] : 0.f;
  __syncthreads();
  const int ty = tid / BK_TW, tx = tid % BK_TW;
  f32x4 acc[CP / 4];
#pragma unroll
  for (int q = 0; q < CP / 4; ++q) acc[q] = reinterpret_cast<const f32x4*>(bs)[q];
  for (int kh = 0; kh < K; ++kh)
    for (int kw = 0; kw < K; ++kw) {
      const float v = xs[(ty + kh) * LW + tx + kw];
      const f32x4* wr = reinterpret_cast<const f32x4*>(ws + (kh * K + kw) * CP);
#pragma unroll
      for (int q = 0; q < CP / 4; ++q) acc[q] += v * wr[q];
    }
  const int hh = h0 + ty, ww = w0 + tx;
  if (hh >= H || ww >= W) return;
  const long o = (((long)b * H + hh) * W + ww) * CP;
#pragma unroll
  for (int q = 0; q < CP / 4; ++q) {
    f32x4 v = acc[q];
    if (relu) {
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    if (mask) {
      const f32x4 m = reinterpret_cast<const f32x4*>(mask + o)[q];
      v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f; v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
    }
    reinterpret_cast<f32x4*>(y + o)[q] = v;
  }
}

static size_t bk_y2f_lds(int K, int cp) {
  return sizeof(float) * ((size_t)K * K * cp + cp + (size_t)(BK_TH + K - 1) * (BK_TW + K - 1));
}

extern "C" int sisr_convk_y2f(const float* x, const float* w, const float* bias, const float* mask, float* y, int B, int H,
                              int W, int K, int cout, int cp, int relu, int flip_taps, void* stream) {
  if (!x || !w || !y || !bk_dims_ok(B, H, W) || cout < 1) return SISR_ERR_ARG;
  if (!bk_k_ok(K) || !bk_cp_ok(cp) || cout > cp) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(y) || !sisr_aligned16(mask)) return SISR_ERR_ALIGN;
  const dim3 grid((W + BK_TW - 1) / BK_TW, (H + BK_TH - 1) / BK_TH, B);
  const size_t lds = bk_y2f_lds(K, cp);
  if (cp == 64)
    hipLaunchKernelGGL(bk_y2f_kernel<64>, grid, dim3(256), lds, (hipStream_t)stream, x, w, bias, mask, y, H, W, K, cout, relu,
                       flip_taps);
  else
    hipLaunchKernelGGL(bk_y2f_kernel<32>, grid, dim3(256), lds, (hipStream_t)stream, x, w, bias, mask, y, H, W, K, cout, relu,
                       flip_taps);
  return sisr_check_launch();
}

// ------------------------------------------------------------------------------------------------ features -> Y
__global__ __launch_bounds__(256) void bk_f2y_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ res,
                                                     float* __restrict__ y, int H, int W, int K, int cin, int cp) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int p = K / 2, LW = BK_TW + K - 1, LH = BK_TH + K - 1, KK = K * K;
  float* ws = lds;             // [KK][cp]
  float* xs = ws + KK * cp;    // [LH * LW][BK_FS]
  const int tid = threadIdx.x, b = blockIdx.z, h0 = blockIdx.y * BK_TH, w0 = blockIdx.x * BK_TW;
  for (int i = tid; i < KK * cp; i += 256) {
    const int tap = i / cp, c = i % cp;
    ws[i] = c < cin ? w[c * KK + tap] : 0.f;
  }
  const int ty = tid / BK_TW, tx = tid % BK_TW;
  float acc = 0.f;
  for (int c0 = 0; c0 < cin; c0 += 16) {
    __syncthreads();  // the previous chunk's readers (and, first time round, nothing) are done with xs
    for (int i = tid; i < LH * LW * 4; i += 256) {
      const int pix = i >> 2, q = i & 3;
      const int hh = h0 + pix / LW - p, ww = w0 + pix % LW - p;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (hh >= 0 && hh < H && ww >= 0 && ww < W)
        v = *reinterpret_cast<const f32x4*>(x + (((long)b * H + hh) * W + ww) * cp + c0 + q * 4);
      *reinterpret_cast<f32x4*>(xs + pix * BK_FS + q * 4) = v;
    }
    __syncthreads();
    for (int kh = 0; kh < K; ++kh)
      for (int kw = 0; kw < K; ++kw) {
        const f32x4* xp = reinterpret_cast<const f32x4*>(xs + ((ty + kh) * LW + tx + kw) * BK_FS);
        const f32x4* wp = reinterpret_cast<const f32x4*>(ws + (kh * K + kw) * cp + c0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4 a = xp[q], ww4 = wp[q];
          acc += a.x * ww4.x + a.y * ww4.y + a.z * ww4.z + a.w * ww4.w;
        }
      }
  }
  const int hh = h0 + ty, ww = w0 + tx;
  if (hh >= H || ww >= W) return;
  const long o = ((long)b * H + hh) * W + ww;
  float v = acc + (bias ? bias[0] : 0.f);
  if (res) v += res[o];
  y[o] = v;
}

static size_t bk_f2y_lds(int K, int cp) {
  return sizeof(float) * ((size_t)K * K * cp + (size_t)(BK_TH + K - 1) * (BK_TW + K - 1) * BK_FS);
}

extern "C" int sisr_convk_f2y(const float* x, const float* w, const float* bias, const float* residual, float* y, int B,
                              int H, int W, int K, int cin, int cp, void* stream) {
  if (!x || !w || !y || !bk_dims_ok(B, H, W) || cin < 1) return SISR_ERR_ARG;
  if (!bk_k_ok(K) || !bk_cp_ok(cp) || cin > cp) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(x)) return SISR_ERR_ALIGN;
  const dim3 grid((W + BK_TW - 1) / BK_TW, (H + BK_TH - 1) / BK_TH, B);
  const size_t lds = bk_f2y_lds(K, cp);  // 9 x 9 from 64 channels: 72 KB
  SISR_ALLOW_LDS(bk_f2y_kernel, bk_f2y_lds(BK_MAXK, 64));
  hipLaunchKernelGGL(bk_f2y_kernel, grid, dim3(256), lds, (hipStream_t)stream, x, w, bias, residual, y, H, W, K, cin, cp);
  return sisr_check_launch();
}

// ------------------------------------------------------------------------------------------------ gradients of the ends
// Thread (g, c): channel c, tap group g (256 / CP groups, NT = ceil(K^2 / groups) taps each).  A workgroup walks its pixel
// tiles in a fixed order and leaves one partial per value; bk_corr_final_kernel sums the partials in workgroup order.
template <int K, int CP>
__global__ __launch_bounds__(256) void bk_corr_kernel(const float* __restrict__ P, const float* __restrict__ Q,
                                                      const float* __restrict__ qmask, float* __restrict__ part, int B, int H,
                                                      int W, int flip, int db_mode) {
  constexpr int KK = K * K, G = 256 / CP, NT = (KK + G - 1) / G, p = K / 2, LW = BK_TW + K - 1, LH = BK_TH + K - 1;
  constexpr int U = NT > 12 ? 4 : 8;  // pixels per batch of loads (fewer where the taps already fill the registers)
  __shared__ float ps[LH * LW];
  const int tid = threadIdx.x, c = tid % CP, g = tid / CP;
  int off[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int tap = g * NT + j;
    int kh = tap / K, kw = tap % K;
    if (flip) { kh = K - 1 - kh; kw = K - 1 - kw; }
    off[j] = tap < KK ? kh * LW + kw : 0;
  }
  float acc[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) acc[j] = 0.f;
  float accb = 0.f;
  const int tx_n = (W + BK_TW - 1) / BK_TW, ty_n = (H + BK_TH - 1) / BK_TH, ntiles = B * ty_n * tx_n;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / (ty_n * tx_n), h0 = (tile / tx_n) % ty_n * BK_TH, w0 = tile % tx_n * BK_TW;
    __syncthreads();
    for (int i = tid; i < LH * LW; i += 256) {
      const int hh = h0 + i / LW - p, ww = w0 + i % LW - p;
      ps[i] = (hh >= 0 && hh < H && ww >= 0 && ww < W) ? P[((long)b * H + hh) * W + ww] : 0.f;
    }
    __syncthreads();
    const int rows = min(BK_TH, H - h0), cols = min(BK_TW, W - w0);
    for (int py = 0; py < rows; ++py)
      for (int px0 = 0; px0 < cols; px0 += U) {  // U pixels at a time: their loads are in flight together
        const long o = (((long)b * H + h0 + py) * W + w0 + px0) * CP + c;
        float q[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const bool ok = px0 + u < cols;
          const long ou = ok ? o + (long)u * CP : o;
          float v = Q[ou];
          if (qmask) v = qmask[ou] > 0.f ? v : 0.f;
          q[u] = ok ? v : 0.f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int base = py * LW + px0 + u;  // px0 + u <= 31: inside the staged tile even past `cols`, where q is 0
#pragma unroll
          for (int j = 0; j < NT; ++j) acc[j] += ps[base + off[j]] * q[u];
          accb += db_mode == 2 ? (px0 + u < cols ? ps[base + p * LW + p] : 0.f) : q[u];
        }
      }
  }
  float* out = part + (long)blockIdx.x * (KK + 1) * CP;
#pragma unroll
  for (int j = 0; j < NT; ++j)
    if (g * NT + j < KK) out[(g * NT + j) * CP + c] = acc[j];
  if (g == 0) out[KK * CP + c] = accb;
}

__global__ __launch_bounds__(256) void bk_corr_final_kernel(const float* __restrict__ part, int nparts, int KK, int cp,
                                                            int channels, int db_mode, float* __restrict__ dw,
                                                            float* __restrict__ db) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = (KK + 1) * cp;
  if (i >= n) return;
  float s = 0.f;
  for (int k = 0; k < nparts; ++k) s += part[(long)k * n + i];
  const int tap = i / cp, c = i % cp;
  if (tap < KK) {
    if (c < channels) dw[c * KK + tap] = s;
  } else if (db) {
    if (db_mode == 1 && c < channels) db[c] = s;
    if (db_mode == 2 && c == 0) db[0] = s;
  }
}

static int bk_corr_parts(int B, int H, int W) {
  const long tiles = (long)B * ((H + BK_TH - 1) / BK_TH) * ((W + BK_TW - 1) / BK_TW);
  return (int)(tiles < BK_PARTS ? tiles : BK_PARTS);
}

extern "C" size_t sisr_corrk_y_workspace_bytes(int B, int H, int W, int K, int cp) {
  if (!bk_dims_ok(B, H, W) || !bk_k_ok(K) || !bk_cp_ok(cp)) return 0;
  return sizeof(float) * (size_t)bk_corr_parts(B, H, W) * (K * K + 1) * cp;
}

template <int K>
static void bk_corr_launch(int cp, int parts, hipStream_t s, const float* P, const float* Q, const float* qmask, float* ws,
                           int B, int H, int W, int flip, int db_mode) {
  if (cp == 64)
    hipLaunchKernelGGL((bk_corr_kernel<K, 64>), dim3(parts), dim3(256), 0, s, P, Q, qmask, ws, B, H, W, flip, db_mode);
  else
    hipLaunchKernelGGL((bk_corr_kernel<K, 32>), dim3(parts), dim3(256), 0, s, P, Q, qmask, ws, B, H, W, flip, db_mode);
}

extern "C" int sisr_corrk_y(const float* P, const float* Q, const float* qmask, float* dw, float* db, int B, int H, int W,
                            int K, int channels, int cp, int flip_taps, int db_mode, float* workspace, size_t workspace_bytes,
                            void* stream) {
  if (!P || !Q || !dw || !workspace || !bk_dims_ok(B, H, W) || channels < 1 || db_mode < 0 || db_mode > 2 ||
      (db_mode && !db))
    return SISR_ERR_ARG;
  if (!bk_k_ok(K) || !bk_cp_ok(cp) || channels > cp) return SISR_ERR_UNSUPPORTED;
  if (workspace_bytes < sisr_corrk_y_workspace_bytes(B, H, W, K, cp)) return SISR_ERR_ARG;
  const int parts = bk_corr_parts(B, H, W);
  hipStream_t s = (hipStream_t)stream;
  switch (K) {
    case 1: bk_corr_launch<1>(cp, parts, s, P, Q, qmask, workspace, B, H, W, flip_taps, db_mode); break;
    case 3: bk_corr_launch<3>(cp, parts, s, P, Q, qmask, workspace, B, H, W, flip_taps, db_mode); break;
    case 5: bk_corr_launch<5>(cp, parts, s, P, Q, qmask, workspace, B, H, W, flip_taps, db_mode); break;
    case 7: bk_corr_launch<7>(cp, parts, s, P, Q, qmask, workspace, B, H, W, flip_taps, db_mode); break;
    default: bk_corr_launch<9>(cp, parts, s, P, Q, qmask, workspace, B, H, W, flip_taps, db_mode); break;
  }
  int rc = sisr_check_launch();
  if (rc) return rc;
  const int n = (K * K + 1) * cp;
  hipLaunchKernelGGL(bk_corr_final_kernel, dim3((n + 255) / 256), dim3(256), 0, s, workspace, parts, K * K, cp, channels,
                     db_mode, dw, db);
  return sisr_check_launch();
}

// ------------------------------------------------------------------------------------------------ K x K conv, fp32 MFMA
// Packed weight: [tap][cin_p / 16][cout_p][16]: element (tap, ci, co) at ((tap * cin_p/16 + ci/16) * cout_p + co) * 16 + ci%16.
__global__ __launch_bounds__(256) void bk_pack_kernel(const float* __restrict__ w, float* __restrict__ fwd,
                                                      float* __restrict__ dgrad, int KK, int cout, int cin, int cop, int cip) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x, n = (long)KK * cop * cip;
  if (e >= n) return;
  const int kk = (int)(e % 16);
  {  // forward: contraction over the weight's input channels
    const int co = (int)(e / 16 % cop), cg = (int)(e / 16 / cop % (cip / 16)), tap = (int)(e / 16 / cop / (cip / 16));
    const int ci = cg * 16 + kk;
    fwd[e] = (co < cout && ci < cin) ? w[((long)co * cin + ci) * KK + tap] : 0.f;
  }
  if (dgrad) {  // input gradient: contraction over the weight's output channels, taps flipped
    const int ci = (int)(e / 16 % cip), og = (int)(e / 16 / cip % (cop / 16)), tap = (int)(e / 16 / cip / (cop / 16));
    const int co = og * 16 + kk;
    dgrad[e] = (co < cout && ci < cin) ? w[((long)co * cin + ci) * KK + (KK - 1 - tap)] : 0.f;
  }
}

extern "C" int sisr_pack_convk(const float* w, float* fwd, float* dgrad, int K, int cout, int cin, int cop, int cip,
                               void* stream) {
  if (!w || !fwd || cout < 1 || cin < 1) return SISR_ERR_ARG;
  if (!bk_k_ok(K) || !bk_cp_ok(cop) || !bk_cp_ok(cip) || cout > cop || cin > cip) return SISR_ERR_UNSUPPORTED;
  const long n = (long)K * K * cop * cip;
  hipLaunchKernelGGL(bk_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, fwd, dgrad,
                     K * K, cout, cin, cop, cip);
  return sisr_check_launch();
}

// Wave v of the 4 computes rows 2v, 2v+1 of the 8 x 32 pixel tile: MT = 2 M-tiles of 32 pixels x NT N-tiles of 32 channels.
// LEAKY: the LeakyReLU forms -- in_mask scales by `slope` where the map is <= 0 instead of zeroing (dy read through the saved
// output of a leaky layer), and `relu` selects v > 0 ? v : slope * v.  The ReLU forms keep their selects (slope unused).
template <int NT, bool LEAKY>
__global__ __launch_bounds__(256) void bk_convk_mfma_kernel(const float* __restrict__ x, const float* __restrict__ in_mask,
                                                            const float* __restrict__ wp, const float* __restrict__ bias,
                                                            int nbias, const float* __restrict__ mask, float* __restrict__ y,
                                                            int H, int W, int K, int cin_p, int relu, float slope) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [LH * LW][BK_XS]
  constexpr int cout_p = NT * 32;
  const int p = K / 2, LW = BK_TW + K - 1, LH = BK_TH + K - 1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
  const int b = blockIdx.z, h0 = blockIdx.y * BK_TH, w0 = blockIdx.x * BK_TW;
  f32x16 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
  const int groups = cin_p / 16;
  for (int ch = 0; ch < cin_p / 32; ++ch) {
    __syncthreads();
    for (int idx = tid; idx < LH * LW * 8; idx += 256) {
      const int pix = idx >> 3, q = idx & 7;
      const int hh = h0 + pix / LW - p, ww = w0 + pix % LW - p;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
        const long o = (((long)b * H + hh) * W + ww) * cin_p + ch * 32 + q * 4;
        v = *reinterpret_cast<const f32x4*>(x + o);
        if (in_mask) {
          const f32x4 m = *reinterpret_cast<const f32x4*>(in_mask + o);
          if constexpr (LEAKY) {
            v.x = m.x > 0.f ? v.x : slope * v.x; v.y = m.y > 0.f ? v.y : slope * v.y;
            v.z = m.z > 0.f ? v.z : slope * v.z; v.w = m.w > 0.f ? v.w : slope * v.w;
          } else {
            v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f; v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;
          }
        }
      }
      *reinterpret_cast<f32x4*>(lds + pix * BK_XS + q * 4) = v;
    }
    __syncthreads();
    for (int kh = 0; kh < K; ++kh)
      for (int kw = 0; kw < K; ++kw) {
        const int tap = kh * K + kw;
        f32x4 bf[NT][4], af[2][4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const f32x4* bp =
              reinterpret_cast<const f32x4*>(wp + (((long)tap * groups + ch * 2 + h) * cout_p + nt * 32 + i) * 16);
#pragma unroll
          for (int q = 0; q < 4; ++q) bf[nt][q] = bp[q];
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const f32x4* ap = reinterpret_cast<const f32x4*>(lds + ((wave * 2 + mt + kh) * LW + i + kw) * BK_XS + h * 16);
#pragma unroll
          for (int q = 0; q < 4; ++q) af[mt][q] = ap[q];
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt][kk >> 2][kk & 3], bf[nt][kk >> 2][kk & 3],
                                                                 acc[mt][nt], 0, 0, 0);
      }
  }
  // D: column (lane & 31) = output channel, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = pixel of the 32-pixel row segment
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int hh = h0 + wave * 2 + mt;
    if (hh >= H) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int co = nt * 32 + i;
      const float bv = (bias && co < nbias) ? bias[co] : 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ww = w0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (ww >= W) continue;
        const long o = (((long)b * H + hh) * W + ww) * cout_p + co;
        float v = acc[mt][nt][r] + bv;
        if constexpr (LEAKY) {
          if (relu) v = v > 0.f ? v : slope * v;
        } else {
          if (relu) v = fmaxf(v, 0.f);
        }
        if (mask) v = mask[o] > 0.f ? v : 0.f;
        y[o] = v;
      }
    }
  }
}

static size_t bk_mfma_lds(int K) { return sizeof(float) * (size_t)(BK_TH + K - 1) * (BK_TW + K - 1) * BK_XS; }

template <bool LEAKY>
static int bk_convk_mfma(const float* x, const float* in_mask, const float* packed, const float* bias, int nbias,
                         const float* mask, float* y, int B, int H, int W, int K, int cin_p, int cout_p, int relu, float slope,
                         void* stream) {
  if (!x || !packed || !y || !bk_dims_ok(B, H, W) || nbias < 0) return SISR_ERR_ARG;
  if (!bk_k_ok(K) || !bk_cp_ok(cin_p) || !bk_cp_ok(cout_p) || nbias > cout_p) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(x) || !sisr_aligned16(in_mask) || !sisr_aligned16(packed)) return SISR_ERR_ALIGN;
  const dim3 grid((W + BK_TW - 1) / BK_TW, (H + BK_TH - 1) / BK_TH, B);
  const size_t lds = bk_mfma_lds(K);  // 9 x 9: 90 KB
  if (cout_p == 64) {
    SISR_ALLOW_LDS((bk_convk_mfma_kernel<2, LEAKY>), bk_mfma_lds(BK_MAXK));
    hipLaunchKernelGGL((bk_convk_mfma_kernel<2, LEAKY>), grid, dim3(256), lds, (hipStream_t)stream, x, in_mask, packed, bias,
                       nbias, mask, y, H, W, K, cin_p, relu, slope);
  } else {
    SISR_ALLOW_LDS((bk_convk_mfma_kernel<1, LEAKY>), bk_mfma_lds(BK_MAXK));
    hipLaunchKernelGGL((bk_convk_mfma_kernel<1, LEAKY>), grid, dim3(256), lds, (hipStream_t)stream, x, in_mask, packed, bias,
                       nbias, mask, y, H, W, K, cin_p, relu, slope);
  }
  return sisr_check_launch();
}

extern "C" int sisr_convk_mfma(const float* x, const float* in_mask, const float* packed, const float* bias, int nbias,
                               const float* mask, float* y, int B, int H, int W, int K, int cin_p, int cout_p, int relu,
                               void* stream) {
  return bk_convk_mfma<false>(x, in_mask, packed, bias, nbias, mask, y, B, H, W, K, cin_p, cout_p, relu, 0.f, stream);
}

extern "C" int sisr_convk_mfma_leaky(const float* x, const float* in_mask, const float* packed, const float* bias, int nbias,
                                     float* y, int B, int H, int W, int K, int cin_p, int cout_p, int act, float slope,
                                     void* stream) {
  if (!(slope == slope) || slope - slope != 0.f) return SISR_ERR_ARG;  // NaN / infinite slope
  return bk_convk_mfma<true>(x, in_mask, packed, bias, nbias, nullptr, y, B, H, W, K, cin_p, cout_p, act, slope, stream);
}

// ------------------------------------------------------------------------------------------------ its weight gradient
// Workgroup (tap, 32-channel chunk of Cin, slice s of the B*H image rows): D[co][ci] += sum_pixels dy[pix][co] x[pix + tap][ci],
// two pixels per MFMA (lane half h takes pixel w0 + h).  The 4 waves take every 4th row of the slice; their tiles are summed
// in wave order through LDS and written as slice s's partial.
// LEAKY: dy is scaled by `slope` where dymask <= 0 instead of zeroed (the layer's activation was a LeakyReLU).
// ST: the conv's stride.  dy (and dymask) is B x H x W; at ST = 2 x is B x Hx x Wx and dy pixel (h, w) meets x pixel
// (2 h + kh - p, 2 w + kw - p); at ST = 1 the two sizes are the same.
template <int MT, bool LEAKY, int ST = 1>
__global__ __launch_bounds__(256) void bk_wgradk_mfma_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             const float* __restrict__ dymask, float* __restrict__ part,
                                                             int B, int H, int W, int K, int cip, int S, float slope,
                                                             int Hx_, int Wx_) {
  const int Hx = ST == 1 ? H : Hx_, Wx = ST == 1 ? W : Wx_;
  __shared__ float red[4][MT][16 * 64];
  constexpr int cop = MT * 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
  const int tap = blockIdx.x, chunk = blockIdx.y, s = blockIdx.z, p = K / 2, kh = tap / K, kw = tap % K, KK = K * K;
  const int rows = B * H, per = (rows + S - 1) / S, r_begin = s * per, r_end = min(rows, r_begin + per);
  f32x16 acc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
  for (int R = r_begin + wave; R < r_end; R += 4) {
    const int b = R / H, hx = ST * (R % H) + kh - p;
    if (hx < 0 || hx >= Hx) continue;  // wave-uniform
    const float* dyr = dy + (long)R * W * cop;
    const float* mr = dymask ? dymask + (long)R * W * cop : nullptr;
    const float* xr = x + ((long)b * Hx + hx) * Wx * cip + chunk * 32 + i;
    for (int wq = 0; wq < W; wq += 16) {  // eight pixel pairs at a time: their loads are in flight together
      float av[8][MT], bv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int wd = wq + 2 * u + h, wx = ST * wd + kw - p;
        const bool okd = wd < W, okx = okd && wx >= 0 && wx < Wx;
        const float xv = xr[(long)(okx ? wx : 0) * cip];
        bv[u] = okx ? xv : 0.f;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const long o = (long)(okd ? wd : 0) * cop + mt * 32 + i;
          float a = dyr[o];
          if constexpr (LEAKY) {
            if (mr) a = mr[o] > 0.f ? a : slope * a;
          } else {
            if (mr) a = mr[o] > 0.f ? a : 0.f;
          }
          av[u][mt] = okd ? a : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u][mt], bv[u], acc[mt], 0, 0, 0);
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave][mt][r * 64 + lane] = acc[mt][r];
  __syncthreads();
  float* out = part + (long)s * cop * cip * KK;
  for (int e = tid; e < MT * 1024; e += 256) {
    const int mt = e >> 10, r = (e >> 6) & 15, l = e & 63;
    const float v = ((red[0][mt][e & 1023] + red[1][mt][e & 1023]) + red[2][mt][e & 1023]) + red[3][mt][e & 1023];
    const int co = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), ci = chunk * 32 + (l & 31);
    out[((long)co * cip + ci) * KK + tap] = v;
  }
}

__global__ __launch_bounds__(256) void bk_wgradk_final_kernel(const float* __restrict__ part, int S, int KK, int cout, int cin,
                                                              int cop, int cip, float* __restrict__ dw) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x, n = (long)cout * cin * KK;
  if (e >= n) return;
  const int tap = (int)(e % KK), ci = (int)(e / KK % cin), co = (int)(e / KK / cin);
  const long src = ((long)co * cip + ci) * KK + tap, stride = (long)cop * cip * KK;
  float sum = 0.f;
  for (int k = 0; k < S; ++k) sum += part[k * stride + src];
  dw[e] = sum;
}

// per-channel sum of a (masked) channels-last map: ordered partials per workgroup, then one ordered pass
template <int CP, bool LEAKY>
__global__ __launch_bounds__(256) void bk_colsum_kernel(const float* __restrict__ dy, const float* __restrict__ dymask,
                                                        long npix, float* __restrict__ part, float slope) {
  constexpr int G = 256 / CP;
  __shared__ float red[256];
  const int c = threadIdx.x % CP, g = threadIdx.x / CP;
  float s = 0.f;
  for (long pix = (long)blockIdx.x * G + g; pix < npix; pix += (long)gridDim.x * G) {
    float v = dy[pix * CP + c];
    if constexpr (LEAKY) {
      if (dymask) v = dymask[pix * CP + c] > 0.f ? v : slope * v;
    } else {
      if (dymask) v = dymask[pix * CP + c] > 0.f ? v : 0.f;
    }
    s += v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (g == 0) {
    float t = red[c];
    for (int k = 1; k < G; ++k) t += red[k * CP + c];
    part[(long)blockIdx.x * CP + c] = t;
  }
}

__global__ __launch_bounds__(64) void bk_colsum_final_kernel(const float* __restrict__ part, int nparts, int cp, int cout,
                                                             float* __restrict__ db) {
  const int c = threadIdx.x;
  if (c >= cout) return;
  float s = 0.f;
  for (int k = 0; k < nparts; ++k) s += part[(long)k * cp + c];
  db[c] = s;
}

static int bk_wgrad_slices(int B, int H, int K, int cip) {
  const int rows = B * H, blocks = K * K * (cip / 32);
  int S = 768 / blocks;
  if (S < 1) S = 1;
  if (S > 64) S = 64;
  const int cap = (rows + 3) / 4;
  return S < cap ? S : cap;
}

static int bk_colsum_parts(long npix, int cp) {
  const long n = (npix + 256 / cp - 1) / (256 / cp);
  return (int)(n < BK_PARTS ? n : BK_PARTS);
}

// H x W: the size of x; dy has H x W pixels at stride 1 and bk_s2_out(H) x bk_s2_out(W) at stride 2
static size_t bk_wgradk_ws_bytes(int B, int H, int W, int K, int cin_p, int cout_p, int stride) {
  if (!bk_dims_ok(B, H, W) || !bk_k_ok(K) || !bk_cp_ok(cin_p) || !bk_cp_ok(cout_p)) return 0;
  const int Hd = stride == 2 ? bk_s2_out(H) : H;
  return sizeof(float) * ((size_t)bk_wgrad_slices(B, Hd, K, cin_p) * cout_p * cin_p * K * K + (size_t)BK_PARTS * cout_p);
}

extern "C" size_t sisr_wgradk_mfma_workspace_bytes(int B, int H, int W, int K, int cin_p, int cout_p) {
  return bk_wgradk_ws_bytes(B, H, W, K, cin_p, cout_p, 1);
}

template <bool LEAKY, int ST = 1>
static int bk_wgradk_mfma(const float* x, const float* dy, const float* dymask, float* dw, float* db, int B, int H, int W,
                          int K, int cout, int cin, int cop, int cip, float* workspace, size_t workspace_bytes, float slope,
                          void* stream) {
  if (!x || !dy || !dw || !workspace || !bk_dims_ok(B, H, W) || cout < 1 || cin < 1) return SISR_ERR_ARG;
  if (!bk_k_ok(K) || !bk_cp_ok(cop) || !bk_cp_ok(cip) || cout > cop || cin > cip) return SISR_ERR_UNSUPPORTED;
  if (workspace_bytes < bk_wgradk_ws_bytes(B, H, W, K, cip, cop, ST)) return SISR_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int Hd = ST == 2 ? bk_s2_out(H) : H, Wd = ST == 2 ? bk_s2_out(W) : W;  // dy's size
  const int S = bk_wgrad_slices(B, Hd, K, cip), KK = K * K;
  const dim3 grid(KK, cip / 32, S);
  if (cop == 64)
    hipLaunchKernelGGL((bk_wgradk_mfma_kernel<2, LEAKY, ST>), grid, dim3(256), 0, s, x, dy, dymask, workspace, B, Hd, Wd, K,
                       cip, S, slope, H, W);
  else
    hipLaunchKernelGGL((bk_wgradk_mfma_kernel<1, LEAKY, ST>), grid, dim3(256), 0, s, x, dy, dymask, workspace, B, Hd, Wd, K,
                       cip, S, slope, H, W);
  int rc = sisr_check_launch();
  if (rc) return rc;
  const long n = (long)cout * cin * KK;
  hipLaunchKernelGGL(bk_wgradk_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, workspace, S, KK, cout, cin,
                     cop, cip, dw);
  rc = sisr_check_launch();
  if (rc || !db) return rc;
  float* bpart = workspace + (size_t)S * cop * cip * KK;
  const long npix = (long)B * Hd * Wd;
  const int parts = bk_colsum_parts(npix, cop);
  if (cop == 64)
    hipLaunchKernelGGL((bk_colsum_kernel<64, LEAKY>), dim3(parts), dim3(256), 0, s, dy, dymask, npix, bpart, slope);
  else
    hipLaunchKernelGGL((bk_colsum_kernel<32, LEAKY>), dim3(parts), dim3(256), 0, s, dy, dymask, npix, bpart, slope);
  rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(bk_colsum_final_kernel, dim3(1), dim3(64), 0, s, bpart, parts, cop, cout, db);
  return sisr_check_launch();
}

extern "C" int sisr_wgradk_mfma(const float* x, const float* dy, const float* dymask, float* dw, float* db, int B, int H,
                                int W, int K, int cout, int cin, int cop, int cip, float* workspace, size_t workspace_bytes,
                                void* stream) {
  return bk_wgradk_mfma<false>(x, dy, dymask, dw, db, B, H, W, K, cout, cin, cop, cip, workspace, workspace_bytes, 0.f, stream);
}

// dymask is the layer's saved output and is required: without it there is no activation to differentiate
extern "C" int sisr_wgradk_mfma_leaky(const float* x, const float* dy, const float* dymask, float* dw, float* db, int B, int H,
                                      int W, int K, int cout, int cin, int cop, int cip, float* workspace,
                                      size_t workspace_bytes, float slope, void* stream) {
  if (!dymask || !(slope == slope) || slope - slope != 0.f) return SISR_ERR_ARG;
  return bk_wgradk_mfma<true>(x, dy, dymask, dw, db, B, H, W, K, cout, cin, cop, cip, workspace, workspace_bytes, slope, stream);
}

// ------------------------------------------------------------------------------------------------ stride-2 K x K conv
// nn.Conv2d(cin, cout, K, stride=2, padding=K/2) between channels-last maps: x is B x H x W, y is B x Ho x Wo with
// Ho = (H - 1) / 2 + 1.  Same implicit GEMM, packing and lane layout as bk_convk_mfma_kernel; LeakyReLU family only.
//
// Forward: output tile of 4 rows x 32 columns, one row (one M-tile) per wave.  Its input halo is (K + 6) x (2 (32 + K/2))
// pixels, staged 32 channels at a time with the even and the odd input columns apart: [row][column parity][column / 2].
// Lane i of a tap (kh, kw) then reads column-pair i + kw/2 of parity kw & 1, so neighbouring lanes stay BK_XS floats apart
// as in the stride-1 kernel (interleaved, they would be 2 BK_XS apart: two lanes per bank group).  Only the outputs' own
// products are formed.  LDS: 63 KB (K = 1), 84 KB (3), 105 KB (5), 128 KB (7), 152 KB (9): one workgroup per CU from K = 3.
#define BK_S2_TH 4

static size_t bk_s2_lds(int K) { return sizeof(float) * (size_t)(2 * BK_S2_TH + K - 2) * 2 * (BK_TW + K / 2) * BK_XS; }

template <int NT>
__global__ __launch_bounds__(256) void bk_convk_s2_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                          const float* __restrict__ bias, int nbias, float* __restrict__ y,
                                                          int H, int W, int Ho, int Wo, int K, int cin_p, int act,
                                                          float slope) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [LH][2][LWH][BK_XS]
  constexpr int cout_p = NT * 32;
  const int p = K / 2, LWH = BK_TW + p, LH = 2 * BK_S2_TH + K - 2;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
  const int b = blockIdx.z, h0 = blockIdx.y * BK_S2_TH, w0 = blockIdx.x * BK_TW;
  f32x16 acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
  const int groups = cin_p / 16;
  for (int ch = 0; ch < cin_p / 32; ++ch) {
    __syncthreads();
    for (int idx = tid; idx < LH * 2 * LWH * 8; idx += 256) {
      const int pix = idx >> 3, q = idx & 7;
      const int lr = pix / (2 * LWH), par = pix % (2 * LWH) / LWH, half = pix % LWH;
      const int hh = 2 * h0 - p + lr, ww = 2 * w0 - p + 2 * half + par;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (hh >= 0 && hh < H && ww >= 0 && ww < W)
        v = *reinterpret_cast<const f32x4*>(x + (((long)b * H + hh) * W + ww) * cin_p + ch * 32 + q * 4);
      *reinterpret_cast<f32x4*>(lds + pix * BK_XS + q * 4) = v;
    }
    __syncthreads();
    for (int kh = 0; kh < K; ++kh)
      for (int kw = 0; kw < K; ++kw) {
        const int tap = kh * K + kw;
        f32x4 bf[NT][4], af[4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const f32x4* bp =
              reinterpret_cast<const f32x4*>(wp + (((long)tap * groups + ch * 2 + h) * cout_p + nt * 32 + i) * 16);
#pragma unroll
          for (int q = 0; q < 4; ++q) bf[nt][q] = bp[q];
        }
        const f32x4* ap = reinterpret_cast<const f32x4*>(
            lds + (((2 * wave + kh) * 2 + (kw & 1)) * LWH + i + (kw >> 1)) * BK_XS + h * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) af[q] = ap[q];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[kk >> 2][kk & 3], bf[nt][kk >> 2][kk & 3], acc[nt], 0, 0, 0);
      }
  }
  const int ho = h0 + wave;
  if (ho >= Ho) return;
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co = nt * 32 + i;
    const float bv = (bias && co < nbias) ? bias[co] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int wo = w0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (wo >= Wo) continue;
      float v = acc[nt][r] + bv;
      if (act) v = v > 0.f ? v : slope * v;
      y[(((long)b * Ho + ho) * Wo + wo) * cout_p + co] = v;
    }
  }
}

static inline bool bk_slope_ok(float slope) { return slope == slope && slope - slope == 0.f; }  // neither NaN nor infinite

extern "C" int sisr_convk_s2_out_size(int n) { return n > 0 ? bk_s2_out(n) : 0; }

extern "C" int sisr_convk_s2_mfma_leaky(const float* x, const float* packed, const float* bias, int nbias, float* y, int B,
                                        int H, int W, int K, int cin_p, int cout_p, int act, float slope, void* stream) {
  if (!x || !packed || !y || !bk_dims_ok(B, H, W) || nbias < 0 || !bk_slope_ok(slope)) return SISR_ERR_ARG;
  if (!bk_k_ok(K) || !bk_cp_ok(cin_p) || !bk_cp_ok(cout_p) || nbias > cout_p) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(x) || !sisr_aligned16(packed)) return SISR_ERR_ALIGN;
  const int Ho = bk_s2_out(H), Wo = bk_s2_out(W);
  const dim3 grid((Wo + BK_TW - 1) / BK_TW, (Ho + BK_S2_TH - 1) / BK_S2_TH, B);
  const size_t lds = bk_s2_lds(K);  // 9 x 9: 152 KB of the CU's 160
  if (cout_p == 64) {
    SISR_ALLOW_LDS(bk_convk_s2_kernel<2>, bk_s2_lds(BK_MAXK));
    hipLaunchKernelGGL(bk_convk_s2_kernel<2>, grid, dim3(256), lds, (hipStream_t)stream, x, packed, bias, nbias, y, H, W, Ho,
                       Wo, K, cin_p, act, slope);
  } else {
    SISR_ALLOW_LDS(bk_convk_s2_kernel<1>, bk_s2_lds(BK_MAXK));
    hipLaunchKernelGGL(bk_convk_s2_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, x, packed, bias, nbias, y, H, W, Ho,
                       Wo, K, cin_p, act, slope);
  }
  return sisr_check_launch();
}

// Input gradient (the transposed conv), polyphase: dx pixel (2a + rp, 2c + cq) takes only the taps kh = rp + p (mod 2),
// kw = cq + p (mod 2), and over those it is a stride-1 correlation of dy: dx[2a + rp] += dy[a + (rp + p - kh) / 2] w[kh].
// A workgroup takes one phase (rp, cq) and 8 x 32 of its pixels (a, c); the dy halo is at most (8 + p) x (32 + p) pixels
// (K = 5: the sub-kernels are 3x3, 3x2, 2x3, 2x2 taps).  No zero is inserted anywhere: the MFMA count is that of the forward.
// At K = 1 the odd phases have no tap and are written as zero.  wp: the 'dgrad' packing of sisr_pack_convk (taps flipped).
// NT counts dx's channel tiles; cop is dy's (padded) width, the contraction.
template <int NT>
__global__ __launch_bounds__(256) void bk_dgradk_s2_kernel(const float* __restrict__ dy, const float* __restrict__ dymask,
                                                           const float* __restrict__ wp, float* __restrict__ dx, int H, int W,
                                                           int Ho, int Wo, int K, int cop, float slope) {
  extern __shared__ __attribute__((aligned(16))) float lds[];  // [LH * LW][BK_XS]
  constexpr int cip = NT * 32;
  const int p = K / 2, tx = gridDim.x >> 1, ty = gridDim.y >> 1;
  const int cq = blockIdx.x >= tx, rp = blockIdx.y >= ty;
  const int b = blockIdx.z, a0 = (blockIdx.y - rp * ty) * BK_TH, c0 = (blockIdx.x - cq * tx) * BK_TW;
  if (2 * a0 + rp >= H || 2 * c0 + cq >= W) return;  // (the odd phases can be a tile shorter; block-uniform)
  const int kh0 = (rp + p) & 1, kw0 = (cq + p) & 1, nkh = (K - kh0 + 1) / 2, nkw = (K - kw0 + 1) / 2;
  const int LH = BK_TH + nkh - 1, LW = BK_TW + nkw - 1;
  // LDS row lr holds dy row a0 + lr + rofs: tap j (kh = kh0 + 2j) of output row a reads lr = a - a0 + nkh - 1 - j
  const int rofs = (rp + p - kh0) / 2 - (nkh - 1), cofs = (cq + p - kw0) / 2 - (nkw - 1);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
  f32x16 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
  const int groups = cop / 16, chunks = (nkh && nkw) ? cop / 32 : 0;
  for (int ch = 0; ch < chunks; ++ch) {
    __syncthreads();
    for (int idx = tid; idx < LH * LW * 8; idx += 256) {
      const int pix = idx >> 3, q = idx & 7;
      const int hh = a0 + pix / LW + rofs, ww = c0 + pix % LW + cofs;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (hh >= 0 && hh < Ho && ww >= 0 && ww < Wo) {
        const long o = (((long)b * Ho + hh) * Wo + ww) * cop + ch * 32 + q * 4;
        v = *reinterpret_cast<const f32x4*>(dy + o);
        if (dymask) {
          const f32x4 m = *reinterpret_cast<const f32x4*>(dymask + o);
          v.x = m.x > 0.f ? v.x : slope * v.x; v.y = m.y > 0.f ? v.y : slope * v.y;
          v.z = m.z > 0.f ? v.z : slope * v.z; v.w = m.w > 0.f ? v.w : slope * v.w;
        }
      }
      *reinterpret_cast<f32x4*>(lds + pix * BK_XS + q * 4) = v;
    }
    __syncthreads();
    for (int j = 0; j < nkh; ++j)
      for (int l = 0; l < nkw; ++l) {
        const int tap = K * K - 1 - ((kh0 + 2 * j) * K + kw0 + 2 * l);  // the flipped packing's index of (kh, kw)
        f32x4 bf[NT][4], af[2][4];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const f32x4* bp = reinterpret_cast<const f32x4*>(wp + (((long)tap * groups + ch * 2 + h) * cip + nt * 32 + i) * 16);
#pragma unroll
          for (int q = 0; q < 4; ++q) bf[nt][q] = bp[q];
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const f32x4* ap = reinterpret_cast<const f32x4*>(
              lds + ((wave * 2 + mt + nkh - 1 - j) * LW + i + nkw - 1 - l) * BK_XS + h * 16);
#pragma unroll
          for (int q = 0; q < 4; ++q) af[mt][q] = ap[q];
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt][kk >> 2][kk & 3], bf[nt][kk >> 2][kk & 3],
                                                                 acc[mt][nt], 0, 0, 0);
      }
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int hx = 2 * (a0 + wave * 2 + mt) + rp;
    if (hx >= H) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int ci = nt * 32 + i;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int wx = 2 * (c0 + (r & 3) + 8 * (r >> 2) + 4 * h) + cq;
        if (wx >= W) continue;
        dx[(((long)b * H + hx) * W + wx) * cip + ci] = acc[mt][nt][r];
      }
    }
  }
}

static size_t bk_s2_dgrad_lds(int K) { return sizeof(float) * (size_t)(BK_TH + K / 2) * (BK_TW + K / 2) * BK_XS; }

// H, W: the size of dx (odd and even sizes share Ho); dymask (optional): the layer's saved output
extern "C" int sisr_dgradk_s2_mfma_leaky(const float* dy, const float* dymask, const float* packed_dgrad, float* dx, int B,
                                         int H, int W, int K, int cout_p, int cin_p, float slope, void* stream) {
  if (!dy || !packed_dgrad || !dx || !bk_dims_ok(B, H, W) || !bk_slope_ok(slope)) return SISR_ERR_ARG;
  if (!bk_k_ok(K) || !bk_cp_ok(cin_p) || !bk_cp_ok(cout_p)) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(dy) || !sisr_aligned16(dymask) || !sisr_aligned16(packed_dgrad)) return SISR_ERR_ALIGN;
  const int Ho = bk_s2_out(H), Wo = bk_s2_out(W);  // = the even phase's pixel count, the larger of the two
  const dim3 grid(2 * ((Wo + BK_TW - 1) / BK_TW), 2 * ((Ho + BK_TH - 1) / BK_TH), B);
  const size_t lds = bk_s2_dgrad_lds(K);  // 9 x 9: 62 KB
  if (cin_p == 64)
    hipLaunchKernelGGL(bk_dgradk_s2_kernel<2>, grid, dim3(256), lds, (hipStream_t)stream, dy, dymask, packed_dgrad, dx, H, W,
                       Ho, Wo, K, cout_p, slope);
  else
    hipLaunchKernelGGL(bk_dgradk_s2_kernel<1>, grid, dim3(256), lds, (hipStream_t)stream, dy, dymask, packed_dgrad, dx, H, W,
                       Ho, Wo, K, cout_p, slope);
  return sisr_check_launch();
}

// Weight / bias gradient: bk_wgradk_mfma_kernel with the strided x index, slices over dy's B * Ho rows.  H, W: the size of x.
// dymask (the layer's saved output) is optional: without it the layer had no activation.
extern "C" size_t sisr_wgradk_s2_mfma_workspace_bytes(int B, int H, int W, int K, int cin_p, int cout_p) {
  return bk_wgradk_ws_bytes(B, H, W, K, cin_p, cout_p, 2);
}

extern "C" int sisr_wgradk_s2_mfma_leaky(const float* x, const float* dy, const float* dymask, float* dw, float* db, int B,
                                         int H, int W, int K, int cout, int cin, int cop, int cip, float* workspace,
                                         size_t workspace_bytes, float slope, void* stream) {
  if (!bk_slope_ok(slope)) return SISR_ERR_ARG;
  return bk_wgradk_mfma<true, 2>(x, dy, dymask, dw, db, B, H, W, K, cout, cin, cop, cip, workspace, workspace_bytes, slope,
                                 stream);
}

// ------------------------------------------------------------------------------------------------ pointwise (1 x 1) layers
// y[b,pix,:] = act(bias + ibias[b] + W x[b,pix,:]) between channels-last maps of 32 / 64 / 128 channels: the same implicit
// GEMM with no halo, so the A operand goes from global memory to registers (16 bytes at a time, the lane layout of the LDS
// reads above) and there is no LDS and no barrier.  A workgroup takes 256 pixels of ONE image (blockIdx.z): the per-image
// bias is a vector per workgroup.  A workgroup makes NT * 32 <= 64 output channels; at 128 outputs blockIdx.y names the
// 64-channel half (all four N-tiles in one wave, NT = 4, compile to 168 VGPRs + 128 AGPRs, one wave per SIMD, with nothing
// but occupancy to hide the loads behind; the halves are 105 + 64, two waves per SIMD, and the second read of x comes
// from L2).  With the 'dgrad' packing and in_mask it is the input gradient.  Packing: sisr_pack_conv1 = bk_pack_kernel at
// one tap.
static inline bool bk_pw_cp_ok(int cp) { return cp == 32 || cp == 64 || cp == 128; }

template <int NT>
__global__ __launch_bounds__(256) void bk_pw_kernel(const float* __restrict__ x, const float* __restrict__ in_mask,
                                                    const float* __restrict__ wp, const float* __restrict__ bias,
                                                    const float* __restrict__ ibias, int nbias, float* __restrict__ y, int HW,
                                                    int cin_p, int cout_p, int act, float slope) {
  const int n0 = blockIdx.y * NT * 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
  const int b = blockIdx.z, p0 = blockIdx.x * 256 + wave * 64;
  const long base = (long)b * HW;
  f32x16 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
  for (int ch = 0; ch < cin_p / 32; ++ch) {
    f32x4 bf[NT][4], af[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int pix = p0 + mt * 32 + i;  // (a pixel past the image reads pixel 0: its row of D is never stored)
      const long o = (base + (pix < HW ? pix : 0)) * cin_p + ch * 32 + h * 16;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        f32x4 v = *reinterpret_cast<const f32x4*>(x + o + q * 4);
        if (in_mask) {
          const f32x4 m = *reinterpret_cast<const f32x4*>(in_mask + o + q * 4);
          v.x = m.x > 0.f ? v.x : slope * v.x; v.y = m.y > 0.f ? v.y : slope * v.y;
          v.z = m.z > 0.f ? v.z : slope * v.z; v.w = m.w > 0.f ? v.w : slope * v.w;
        }
        af[mt][q] = v;
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const f32x4* bp = reinterpret_cast<const f32x4*>(wp + ((long)(ch * 2 + h) * cout_p + n0 + nt * 32 + i) * 16);
#pragma unroll
      for (int q = 0; q < 4; ++q) bf[nt][q] = bp[q];
    }
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt][kk >> 2][kk & 3], bf[nt][kk >> 2][kk & 3], acc[mt][nt],
                                                             0, 0, 0);
  }
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int co = n0 + nt * 32 + i;
    float bv = 0.f;
    if (co < nbias) {
      if (bias) bv = bias[co];
      if (ibias) bv += ibias[(long)b * nbias + co];
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int pix = p0 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (pix >= HW) continue;
        float v = acc[mt][nt][r] + bv;
        if (act) v = v > 0.f ? v : slope * v;
        y[(base + pix) * cout_p + co] = v;
      }
  }
}

extern "C" int sisr_pack_conv1(const float* w, float* fwd, float* dgrad, int cout, int cin, int cop, int cip, void* stream) {
  if (!w || !fwd || cout < 1 || cin < 1) return SISR_ERR_ARG;
  if (!bk_pw_cp_ok(cop) || !bk_pw_cp_ok(cip) || cout > cop || cin > cip) return SISR_ERR_UNSUPPORTED;
  const long n = (long)cop * cip;
  hipLaunchKernelGGL(bk_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, fwd, dgrad, 1,
                     cout, cin, cop, cip);
  return sisr_check_launch();
}

// bias (nbias values) and ibias (B x nbias, one row per image) are optional and added before the activation
extern "C" int sisr_conv1_mfma_leaky(const float* x, const float* in_mask, const float* packed, const float* bias,
                                     const float* ibias, int nbias, float* y, int B, int H, int W, int cin_p, int cout_p,
                                     int act, float slope, void* stream) {
  if (!x || !packed || !y || !bk_dims_ok(B, H, W) || nbias < 0 || !bk_slope_ok(slope)) return SISR_ERR_ARG;
  if (!bk_pw_cp_ok(cin_p) || !bk_pw_cp_ok(cout_p) || nbias > cout_p) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(x) || !sisr_aligned16(in_mask) || !sisr_aligned16(packed)) return SISR_ERR_ALIGN;
  const int HW = H * W;
  const dim3 grid((HW + 255) / 256, cout_p == 128 ? 2 : 1, B);
  hipStream_t s = (hipStream_t)stream;
  if (cout_p == 32)
    hipLaunchKernelGGL(bk_pw_kernel<1>, grid, dim3(256), 0, s, x, in_mask, packed, bias, ibias, nbias, y, HW, cin_p, cout_p,
                       act, slope);
  else
    hipLaunchKernelGGL(bk_pw_kernel<2>, grid, dim3(256), 0, s, x, in_mask, packed, bias, ibias, nbias, y, HW, cin_p, cout_p,
                       act, slope);
  return sisr_check_launch();
}

// Per-image column sums of the (masked) dy: part (b, k) sums every gridDim.x-th group of G pixels of image b, the groups in
// order through LDS; bk_pw_colsum_final_kernel sums an image's parts in order (d ibias), bk_pw_bias_kernel the images (db).
template <int CP>
__global__ __launch_bounds__(256) void bk_pw_colsum_kernel(const float* __restrict__ dy, const float* __restrict__ dymask,
                                                           int HW, float* __restrict__ part, float slope) {
  constexpr int G = 256 / CP;
  __shared__ float red[256];
  const int c = threadIdx.x % CP, g = threadIdx.x / CP;
  const long base = (long)blockIdx.y * HW;
  float s = 0.f;
  for (int pix = blockIdx.x * G + g; pix < HW; pix += gridDim.x * G) {
    float v = dy[(base + pix) * CP + c];
    if (dymask) v = dymask[(base + pix) * CP + c] > 0.f ? v : slope * v;
    s += v;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  if (g == 0) {
    float t = red[c];
    for (int k = 1; k < G; ++k) t += red[k * CP + c];
    part[((long)blockIdx.y * gridDim.x + blockIdx.x) * CP + c] = t;
  }
}

__global__ __launch_bounds__(128) void bk_pw_colsum_final_kernel(const float* __restrict__ part, int nparts, int cp, int cout,
                                                                 float* __restrict__ isum, float* __restrict__ dib) {
  const int c = threadIdx.x, b = blockIdx.x;
  if (c >= cp) return;
  float s = 0.f;
  for (int k = 0; k < nparts; ++k) s += part[((long)b * nparts + k) * cp + c];
  isum[(long)b * cp + c] = s;
  if (dib && c < cout) dib[(long)b * cout + c] = s;
}

__global__ __launch_bounds__(128) void bk_pw_bias_kernel(const float* __restrict__ isum, int B, int cp, int cout,
                                                         float* __restrict__ db) {
  const int c = threadIdx.x;
  if (c >= cout) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += isum[(long)b * cp + c];
  db[c] = s;
}

static int bk_pw_colsum_parts(int B, int HW, int cp) {
  const int G = 256 / cp, want = (HW + G - 1) / G, cap = BK_PARTS / B > 0 ? BK_PARTS / B : 1;
  return want < cap ? want : cap;
}

extern "C" size_t sisr_wgrad1_mfma_workspace_bytes(int B, int H, int W, int cin_p, int cout_p) {
  if (!bk_dims_ok(B, H, W) || !bk_pw_cp_ok(cin_p) || !bk_pw_cp_ok(cout_p)) return 0;
  return sizeof(float) * ((size_t)bk_wgrad_slices(B, H, 1, cin_p) * cout_p * cin_p +
                          ((size_t)bk_pw_colsum_parts(B, H * W, cout_p) + 1) * B * cout_p);
}

// dw (cout, cin) from x and dy' = dymask > 0 ? dy : slope * dy (dymask optional: no activation), by bk_wgradk_mfma_kernel at
// one tap; db (cout) and dib (B x cout, the gradient of the per-image bias), both optional, from the per-image column sums.
extern "C" int sisr_wgrad1_mfma_leaky(const float* x, const float* dy, const float* dymask, float* dw, float* db, float* dib,
                                      int B, int H, int W, int cout, int cin, int cop, int cip, float* workspace,
                                      size_t workspace_bytes, float slope, void* stream) {
  if (!x || !dy || !dw || !workspace || !bk_dims_ok(B, H, W) || cout < 1 || cin < 1 || !bk_slope_ok(slope)) return SISR_ERR_ARG;
  if (!bk_pw_cp_ok(cop) || !bk_pw_cp_ok(cip) || cout > cop || cin > cip) return SISR_ERR_UNSUPPORTED;
  if (workspace_bytes < sisr_wgrad1_mfma_workspace_bytes(B, H, W, cip, cop)) return SISR_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int S = bk_wgrad_slices(B, H, 1, cip);
  const dim3 grid(1, cip / 32, S);
  switch (cop) {
    case 128: hipLaunchKernelGGL((bk_wgradk_mfma_kernel<4, true>), grid, dim3(256), 0, s, x, dy, dymask, workspace, B, H, W, 1, cip, S, slope, H, W); break;
    case 64: hipLaunchKernelGGL((bk_wgradk_mfma_kernel<2, true>), grid, dim3(256), 0, s, x, dy, dymask, workspace, B, H, W, 1, cip, S, slope, H, W); break;
    default: hipLaunchKernelGGL((bk_wgradk_mfma_kernel<1, true>), grid, dim3(256), 0, s, x, dy, dymask, workspace, B, H, W, 1, cip, S, slope, H, W); break;
  }
  int rc = sisr_check_launch();
  if (rc) return rc;
  const long n = (long)cout * cin;
  hipLaunchKernelGGL(bk_wgradk_final_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, workspace, S, 1, cout, cin,
                     cop, cip, dw);
  rc = sisr_check_launch();
  if (rc || (!db && !dib)) return rc;
  const int HW = H * W, parts = bk_pw_colsum_parts(B, HW, cop);
  float* part = workspace + (size_t)S * cop * cip;
  float* isum = part + (size_t)parts * B * cop;
  const dim3 cgrid(parts, B);
  switch (cop) {
    case 128: hipLaunchKernelGGL(bk_pw_colsum_kernel<128>, cgrid, dim3(256), 0, s, dy, dymask, HW, part, slope); break;
    case 64: hipLaunchKernelGGL(bk_pw_colsum_kernel<64>, cgrid, dim3(256), 0, s, dy, dymask, HW, part, slope); break;
    default: hipLaunchKernelGGL(bk_pw_colsum_kernel<32>, cgrid, dim3(256), 0, s, dy, dymask, HW, part, slope); break;
  }
  rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(bk_pw_colsum_final_kernel, dim3(B), dim3(128), 0, s, part, parts, cop, cout, isum, dib);
  rc = sisr_check_launch();
  if (rc || !db) return rc;
  hipLaunchKernelGGL(bk_pw_bias_kernel, dim3(1), dim3(128), 0, s, isum, B, cop, cout, db);
  return sisr_check_launch();
}

// ------------------------------------------------------------------------------------------------ global mean of a map
// out[b][c] = (sum_pix x[b][pix][c]) / (H W) for the real channels of a channels-last map, and its gradient.  Two ordered
// stages in float64: part p of image b sums the fixed pixel range [p per, (p + 1) per) (thread group g takes every G-th pixel
// of it, the groups are summed in order through LDS), then one thread per channel sums the parts in order.  The float64 sum
// of fp32 values is exact far beyond the fp32 budget, so the result is the correctly rounded mean and repeats bit for bit.
#define MM_PIX 512   // pixels per part
#define MM_PARTS 128 // at most this many parts per image

static int mm_parts(int H, int W) {
  const long n = ((long)H * W + MM_PIX - 1) / MM_PIX;
  return (int)(n < MM_PARTS ? n : MM_PARTS);
}

template <int CP>
__global__ __launch_bounds__(256) void bk_map_mean_partial_kernel(const float* __restrict__ x, long HW, int per,
                                                                  double* __restrict__ part) {
  constexpr int Q = CP / 4, G = 256 / Q;  // Q lanes of 4 channels per pixel, G pixels per pass
  __shared__ double red[G][CP];
  const int q = threadIdx.x % Q, g = threadIdx.x / Q, b = blockIdx.y;
  const long begin = (long)blockIdx.x * per, end = begin + per < HW ? begin + per : HW;
  double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
  const float* xb = x + (long)b * HW * CP + q * 4;
  for (long pix = begin + g; pix < end; pix += G) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(xb + pix * CP);
    s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
  }
  red[g][q * 4 + 0] = s0; red[g][q * 4 + 1] = s1; red[g][q * 4 + 2] = s2; red[g][q * 4 + 3] = s3;
  __syncthreads();
  if (threadIdx.x < CP) {
    double t = red[0][threadIdx.x];
    for (int k = 1; k < G; ++k) t += red[k][threadIdx.x];
    part[((long)b * gridDim.x + blockIdx.x) * CP + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(64) void bk_map_mean_final_kernel(const double* __restrict__ part, int nparts, int cp, int c,
                                                               double hw, float* __restrict__ out) {
  const int ch = threadIdx.x, b = blockIdx.x;
  if (ch >= c) return;
  double s = 0.;
  for (int k = 0; k < nparts; ++k) s += part[((long)b * nparts + k) * cp + ch];
  out[(long)b * c + ch] = (float)(s / hw);
}

template <int CP>
__global__ __launch_bounds__(256) void bk_map_mean_bwd_kernel(const float* __restrict__ g, long HW, int c, float hw,
                                                              float* __restrict__ dx) {
  constexpr int Q = CP / 4;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;  // one 4-channel group of one pixel of image blockIdx.y
  if (e >= HW * Q) return;
  const int q = (int)(e % Q), b = blockIdx.y;
  f32x4 v;
  v.x = q * 4 + 0 < c ? g[(long)b * c + q * 4 + 0] / hw : 0.f;
  v.y = q * 4 + 1 < c ? g[(long)b * c + q * 4 + 1] / hw : 0.f;
  v.z = q * 4 + 2 < c ? g[(long)b * c + q * 4 + 2] / hw : 0.f;
  v.w = q * 4 + 3 < c ? g[(long)b * c + q * 4 + 3] / hw : 0.f;
  reinterpret_cast<f32x4*>(dx + (long)b * HW * CP)[e] = v;
}

// (H W <= 2^24 keeps float(H W) exact in the backward's division)
static inline bool mm_dims_ok(int B, int H, int W) { return bk_dims_ok(B, H, W) && (long)H * W <= (1L << 24); }

extern "C" size_t sisr_map_mean_workspace_bytes(int B, int H, int W, int cp) {
  if (!mm_dims_ok(B, H, W) || !bk_cp_ok(cp)) return 0;
  return sizeof(double) * (size_t)B * mm_parts(H, W) * cp;
}

extern "C" int sisr_map_mean(const float* x, float* out, int B, int H, int W, int c, int cp, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (!x || !out || !workspace || !mm_dims_ok(B, H, W) || c < 1) return SISR_ERR_ARG;
  if (!bk_cp_ok(cp) || c > cp) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(x) || ((uintptr_t)workspace & 7)) return SISR_ERR_ALIGN;
  if (workspace_bytes < sisr_map_mean_workspace_bytes(B, H, W, cp)) return SISR_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const long HW = (long)H * W;
  const int parts = mm_parts(H, W), per = (int)((HW + parts - 1) / parts);
  double* part = (double*)workspace;
  if (cp == 64)
    hipLaunchKernelGGL(bk_map_mean_partial_kernel<64>, dim3(parts, B), dim3(256), 0, s, x, HW, per, part);
  else
    hipLaunchKernelGGL(bk_map_mean_partial_kernel<32>, dim3(parts, B), dim3(256), 0, s, x, HW, per, part);
  int rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(bk_map_mean_final_kernel, dim3(B), dim3(64), 0, s, part, parts, cp, c, (double)HW, out);
  return sisr_check_launch();
}

extern "C" int sisr_map_mean_bwd(const float* g, float* dx, int B, int H, int W, int c, int cp, void* stream) {
  if (!g || !dx || !mm_dims_ok(B, H, W) || c < 1) return SISR_ERR_ARG;
  if (!bk_cp_ok(cp) || c > cp) return SISR_ERR_UNSUPPORTED;
  if (!sisr_aligned16(dx)) return SISR_ERR_ALIGN;
  const long HW = (long)H * W, n = HW * (cp / 4);
  const dim3 grid((unsigned)((n + 255) / 256), B);
  if (cp == 64)
    hipLaunchKernelGGL(bk_map_mean_bwd_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, g, HW, c, (float)HW, dx);
  else
    hipLaunchKernelGGL(bk_map_mean_bwd_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, g, HW, c, (float)HW, dx);
  return sisr_check_launch();
}

// ------------------------------------------------------------------------------------------------ MSE loss
#define MSE_BLOCKS 512

__global__ __launch_bounds__(256) void bk_mse_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                             float* __restrict__ grad, float two_inv_n, long n,
                                                             float* __restrict__ part) {
  __shared__ float red[256];
  float s = 0.f;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float d = a[i] - b[i];
    s += d * d;
    if (grad) grad[i] = d * two_inv_n;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void bk_mse_final_kernel(const float* __restrict__ part, int nparts, float inv_n,
                                                           float* __restrict__ loss) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = red[0] * inv_n;
}

extern "C" size_t sisr_mse_loss_workspace_bytes() { return MSE_BLOCKS * sizeof(float); }

extern "C" int sisr_mse_loss(const float* a, const float* b, long n, float* loss, float* grad, float* workspace,
                             void* stream) {
  if (!a || !b || !loss || !workspace || n <= 0) return SISR_ERR_ARG;
  long blocks = (n + 255) / 256;
  if (blocks > MSE_BLOCKS) blocks = MSE_BLOCKS;
  const float inv_n = 1.0f / (float)n;
  hipLaunchKernelGGL(bk_mse_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, b, grad,
                     2.0f * inv_n, n, workspace);
  int rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(bk_mse_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, workspace, (int)blocks, inv_n, loss);
  return sisr_check_launch();
}
