// Dense-block growth convolutions (RRDBNet / ESRGAN): 3 x 3, cin -> 32 with cin in {64, 96, 128, 160}, fp32, on
// v_mfma_f32_32x32x2_f32.  ref: the Residual Dense Block of ESRGAN -- x_j = lrelu(conv_j(cat(x, x_1 .. x_{j-1}))).
//
// A dense block lives in ONE channels-last stack S[B][H][W][192]: channels 0..63 the block input, slot j (channels
// 64 + 32 (j - 1) ...) the output of layer j.  Layer j reads channels [0, cin_j) and writes its slot of the same pixel records:
// no concatenation is ever built.  So every map argument is {pointer, pitch (floats per pixel)} and a channel count; the
// channels next to a range are live data of somebody else: every halo load is predicated, nothing is read or written outside
// [0, cin) / [0, 32) of a pixel that lies in the image.
//
//   sisr_pack_dense3x3     OIHW (32, cin, 3, 3) -> the forward packing [tap][cin / 16][32][16] and the input-gradient packing
//                          [tap][2][cin][16] (taps flipped, roles swapped), one launch.
//   sisr_dense3x3_fwd      implicit GEMM as bk_convk_mfma_kernel (basic.hip): M = 32 pixels of a row, N = 32 output channels,
//                          the haloed 10 x 34 tile staged 32 input channels at a time, weights streamed per tap.
//   sisr_dense3x3_dgrad    the same walk with one staged chunk (the 32 channels of dy') and N = cin: dx (+)= conv^T(dy'),
//                          dy' = mask > 0 ? dy : slope * dy taken on the staging loads.  accumulate: every element of dx is read
//                          and written once, by the lane that owns it.
//   sisr_dense3x3_wgrad    per workgroup (slice of the pixel tiles, 32-channel chunk of cin): ONE haloed x tile and its dy' tile in
//                          LDS per step, all nine taps formed from them (M = 32 output channels, N = 32 input channels, two
//                          pixels per MFMA); the four waves' tiles are summed in wave order, the slices by a second ordered pass.
//                          The bias gradient rides in chunk 0's workgroups.  No atomics: bitwise repeatable.
//
// Within a lane the contraction index of the forward / input-gradient MFMAs is permuted as in basic.hip (lane half h takes
// channels 16 h + kk at step kk) so that both operands are read 16 bytes at a time.
#include "sisr_common.h"

#define DN_TH 8   // pixel tile of all three kernels: 8 rows x 32 columns, 256 threads
#define DN_TW 32
#define DN_LH (DN_TH + 2)
#define DN_LW (DN_TW + 2)
#define DN_XS 36      // LDS pixel stride (floats) of the forward / input-gradient tile: 32 + 4, 16-byte reads stay aligned
#define DN_WS 32      // LDS pixel stride of the weight gradient's tiles: one float per lane and MFMA, the two lane halves 32 banks apart
#define DN_GROW 32    // output channels of a growth conv
#define DN_MAX_WG 768 // weight gradient: at most this many workgroups (three per CU)
#define DN_MAX_PITCH 4096

static inline bool dn_dims_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && B <= 65535 && H <= 65536 && W <= 65536 && (long)B * H * W <= (1L << 28);
}
static inline bool dn_pitch_ok(int pitch, int channels) { return pitch >= channels && pitch % 32 == 0 && pitch <= DN_MAX_PITCH; }
static inline bool dn_slope_ok(float slope) { return slope == slope && slope - slope == 0.f; }  // neither NaN nor infinite
// 0 built, else the error code
static inline int dn_cin_code(int cin) {
  if (cin <= 0 || cin % 32) return SISR_ERR_ARG;
  return (cin == 64 || cin == 96 || cin == 128 || cin == 160) ? 0 : SISR_ERR_UNSUPPORTED;
}
// Does the range [0, bn) of b's pixel records (pitch bp) touch the range [0, an) of a's?  Disjoint extents never do; inside
// one extent equal pitches interleave cleanly iff b's range falls between two of a's; different pitches are refused.
static bool dn_clash(const float* a, long ap, int an, const float* b, long bp, int bn, long npix) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  const uintptr_t a1 = a0 + 4 * (uintptr_t)((npix - 1) * ap + an), b1 = b0 + 4 * (uintptr_t)((npix - 1) * bp + bn);
  if (a1 <= b0 || b1 <= a0) return false;
  if (ap != bp || ((b0 ^ a0) & 3)) return true;
  long d = (b0 >= a0 ? (long)((b0 - a0) / 4) : -(long)((a0 - b0) / 4)) % ap;
  if (d < 0) d += ap;
  return d < an || d + bn > ap;
}

// ------------------------------------------------------------------------------------------------ packing
__global__ __launch_bounds__(256) void dn_pack_kernel(const float* __restrict__ w, float* __restrict__ fwd,
                                                      float* __restrict__ dgrad, int cin) {
  const int e = blockIdx.x * 256 + threadIdx.x, n = 9 * DN_GROW * cin;
  if (e >= n) return;
  const int kk = e % 16;
  if (fwd) {  // forward: contraction over the weight's input channels
    const int co = e / 16 % DN_GROW, cg = e / 16 / DN_GROW % (cin / 16), tap = e / 16 / DN_GROW / (cin / 16);
    fwd[e] = w[(co * cin + cg * 16 + kk) * 9 + tap];
  }
  if (dgrad) {  // input gradient: contraction over the weight's output channels, taps flipped
    const int ci = e / 16 % cin, og = e / 16 / cin % 2, tap = e / 16 / cin / 2;
    dgrad[e] = w[((og * 16 + kk) * cin + ci) * 9 + (8 - tap)];
  }
}

extern "C" int sisr_pack_dense3x3(const float* w, float* packed_fwd, float* packed_dgrad, int cin, void* stream) {
  if (!w || (!packed_fwd && !packed_dgrad)) return SISR_ERR_ARG;
  if (const int rc = dn_cin_code(cin)) return rc;
  const int n = 9 * DN_GROW * cin;
  hipLaunchKernelGGL(dn_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, packed_fwd, packed_dgrad, cin);
  return sisr_check_launch();
}

// ------------------------------------------------------------------------------------------------ gated skip between stacks
// y[..., 0:64] = t[..., 0:64] * g[b][c] + x[..., 0:64] (x nullable), each map with its own pitch: the RRDB's `out * 0.2 + x`
// (g constant) and the meta-attention form `(out * m) * 0.2 + x` (g = 0.2 m), read from one stack and written into the next.
// The product is rounded before the sum (sisr_mul_add4), as the stand-alone gate kernel does.
__global__ __launch_bounds__(256) void dn_skip_kernel(const float* __restrict__ t, int tp, const float* __restrict__ g,
                                                      const float* __restrict__ x, int xp, float* __restrict__ y, int yp,
                                                      long hw, long n) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const long pix = e >> 4;
  const int q = (int)(e & 15) * 4;
  const f32x4 tv = *reinterpret_cast<const f32x4*>(t + pix * tp + q);
  const f32x4 gv = *reinterpret_cast<const f32x4*>(g + (pix / hw) * 64 + q);
  f32x4 xv = {0.f, 0.f, 0.f, 0.f};
  if (x) xv = *reinterpret_cast<const f32x4*>(x + pix * xp + q);
  *reinterpret_cast<f32x4*>(y + pix * yp + q) = sisr_mul_add4(tv, gv, xv);
}

extern "C" int sisr_dense_skip(const float* t, int t_pitch, const float* g, const float* x, int x_pitch, float* y, int y_pitch,
                               int B, long hw, void* stream) {
  if (!t || !g || !y || B < 1 || hw < 1 || (long)B * hw > (1L << 28)) return SISR_ERR_ARG;
  if (!dn_pitch_ok(t_pitch, 64) || !dn_pitch_ok(y_pitch, 64) || (x && !dn_pitch_ok(x_pitch, 64))) return SISR_ERR_ARG;
  if (!sisr_aligned16(t) || !sisr_aligned16(g) || !sisr_aligned16(x) || !sisr_aligned16(y)) return SISR_ERR_ALIGN;
  const long npix = (long)B * hw, n = npix * 16;
  // y may be t or x itself (same pointer and pitch: every element is read and written by one thread); any other overlap is refused
  if (!(y == t && y_pitch == t_pitch) && dn_clash(t, t_pitch, 64, y, y_pitch, 64, npix)) return SISR_ERR_ARG;
  if (x && !(y == x && y_pitch == x_pitch) && dn_clash(x, x_pitch, 64, y, y_pitch, 64, npix)) return SISR_ERR_ARG;
  hipLaunchKernelGGL(dn_skip_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, t_pitch, g, x,
                     x_pitch, y, y_pitch, hw, n);
  return sisr_check_launch();
}

// ------------------------------------------------------------------------------------------------ staging, shared
// One 32-channel chunk of the haloed 10 x 34 tile at (h0 - 1, w0 - 1) into lds[pixel][DN_XS or DN_WS]; pixels outside the image
// are zero and are not loaded.  mask (nullable, own pitch): v -> mask > 0 ? v : slope * v (PyTorch's LeakyReLU' convention:
// zero takes the slope branch).
template <int STRIDE, int LH, int LW, int HALO>
__device__ __forceinline__ void dn_stage(float* lds, const float* __restrict__ src, int pitch, const float* __restrict__ mask,
                                         int mpitch, float slope, long img, int h0, int w0, int H, int W, int tid) {
  for (int idx = tid; idx < LH * LW * 8; idx += 256) {
    const int pix = idx >> 3, q = idx & 7;
    const int hh = h0 + pix / LW - HALO, ww = w0 + pix % LW - HALO;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
      const long p = img + (long)hh * W + ww;
      v = *reinterpret_cast<const f32x4*>(src + p * pitch + q * 4);
      if (mask) {
        const f32x4 m = *reinterpret_cast<const f32x4*>(mask + p * mpitch + q * 4);
        v.x = m.x > 0.f ? v.x : slope * v.x; v.y = m.y > 0.f ? v.y : slope * v.y;
        v.z = m.z > 0.f ? v.z : slope * v.z; v.w = m.w > 0.f ? v.w : slope * v.w;
      }
    }
    *reinterpret_cast<f32x4*>(lds + pix * STRIDE + q * 4) = v;
  }
}

// ------------------------------------------------------------------------------------------------ forward
// Wave v of the 4 computes rows 2v, 2v + 1 of the tile: two M-tiles of 32 pixels x one N-tile of 32 output channels.
__global__ __launch_bounds__(256) void dn_fwd_kernel(const float* __restrict__ x, int xp, int cin, const float* __restrict__ wp,
                                                     const float* __restrict__ bias, int act, float slope,
                                                     float* __restrict__ y, int yp, int H, int W) {
  __shared__ __attribute__((aligned(16))) float lds[DN_LH * DN_LW * DN_XS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
  const int h0 = blockIdx.y * DN_TH, w0 = blockIdx.x * DN_TW;
  const long img = (long)blockIdx.z * H * W;
  f32x16 acc[2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
  const int groups = cin / 16;
  for (int ch = 0; ch < cin / 32; ++ch) {
    __syncthreads();
    dn_stage<DN_XS, DN_LH, DN_LW, 1>(lds, x + ch * 32, xp, nullptr, 0, 0.f, img, h0, w0, H, W, tid);
    __syncthreads();
    for (int kh = 0; kh < 3; ++kh)
      for (int kw = 0; kw < 3; ++kw) {
        const int tap = kh * 3 + kw;
        f32x4 bf[4], af[2][4];
        const f32x4* bp = reinterpret_cast<const f32x4*>(wp + (((long)tap * groups + ch * 2 + h) * DN_GROW + i) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) bf[q] = bp[q];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const f32x4* ap = reinterpret_cast<const f32x4*>(lds + ((wave * 2 + mt + kh) * DN_LW + i + kw) * DN_XS + h * 16);
#pragma unroll
          for (int q = 0; q < 4; ++q) af[mt][q] = ap[q];
        }
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt][kk >> 2][kk & 3], bf[kk >> 2][kk & 3], acc[mt], 0, 0, 0);
      }
  }
  // D: column (lane & 31) = output channel, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5) = pixel of the 32-pixel row segment
  const float bv = bias ? bias[i] : 0.f;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int hh = h0 + wave * 2 + mt;
    if (hh >= H) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ww = w0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (ww >= W) continue;
      float v = acc[mt][r] + bv;
      if (act) v = v > 0.f ? v : slope * v;
      y[(img + (long)hh * W + ww) * yp + i] = v;
    }
  }
}

extern "C" int sisr_dense3x3_fwd(const float* x, int x_pitch, int cin, const float* packed, const float* bias, int act,
                                 float slope, float* y, int y_pitch, int B, int H, int W, void* stream) {
  if (!x || !packed || !y || !dn_dims_ok(B, H, W) || !dn_slope_ok(slope)) return SISR_ERR_ARG;
  if (const int rc = dn_cin_code(cin)) return rc;
  if (!dn_pitch_ok(x_pitch, cin) || !dn_pitch_ok(y_pitch, DN_GROW)) return SISR_ERR_ARG;
  if (!sisr_aligned16(x) || !sisr_aligned16(packed) || !sisr_aligned16(y)) return SISR_ERR_ALIGN;
  if (dn_clash(x, x_pitch, cin, y, y_pitch, DN_GROW, (long)B * H * W)) return SISR_ERR_ARG;
  const dim3 grid((W + DN_TW - 1) / DN_TW, (H + DN_TH - 1) / DN_TH, B);
  hipLaunchKernelGGL(dn_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, x_pitch, cin, packed, bias, act, slope, y,
                     y_pitch, H, W);
  return sisr_check_launch();
}

// ------------------------------------------------------------------------------------------------ input gradient
// NT = cin / 32 N-tiles of input channels; the contraction is over the 32 channels of dy' (one staged chunk) and nine taps.
template <int NT>
__global__ __launch_bounds__(256) void dn_dgrad_kernel(const float* __restrict__ dy, int dyp, const float* __restrict__ mask,
                                                       int mp, float slope, const float* __restrict__ wp,
                                                       float* __restrict__ dx, int dxp, int accumulate, int H, int W) {
  __shared__ __attribute__((aligned(16))) float lds[DN_LH * DN_LW * DN_XS];
  constexpr int cin = NT * 32;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
  const int h0 = blockIdx.y * DN_TH, w0 = blockIdx.x * DN_TW;
  const long img = (long)blockIdx.z * H * W;
  f32x16 acc[2][NT];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
  dn_stage<DN_XS, DN_LH, DN_LW, 1>(lds, dy, dyp, mask, mp, slope, img, h0, w0, H, W, tid);
  __syncthreads();
  for (int kh = 0; kh < 3; ++kh)
    for (int kw = 0; kw < 3; ++kw) {
      const int tap = kh * 3 + kw;
      f32x4 af[2][4];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const f32x4* ap = reinterpret_cast<const f32x4*>(lds + ((wave * 2 + mt + kh) * DN_LW + i + kw) * DN_XS + h * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) af[mt][q] = ap[q];
      }
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        f32x4 bf[4];
        const f32x4* bp = reinterpret_cast<const f32x4*>(wp + (((long)tap * 2 + h) * cin + nt * 32 + i) * 16);
#pragma unroll
        for (int q = 0; q < 4; ++q) bf[q] = bp[q];
#pragma unroll
        for (int kk = 0; kk < 16; ++kk)
#pragma unroll
          for (int mt = 0; mt < 2; ++mt)
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt][kk >> 2][kk & 3], bf[kk >> 2][kk & 3], acc[mt][nt], 0, 0, 0);
      }
    }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int hh = h0 + wave * 2 + mt;
    if (hh >= H) continue;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ww = w0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (ww >= W) continue;
      float* o = dx + (img + (long)hh * W + ww) * dxp + i;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        float v = acc[mt][nt][r];
        if (accumulate) v = o[nt * 32] + v;
        o[nt * 32] = v;
      }
    }
  }
}

extern "C" int sisr_dense3x3_dgrad(const float* dy, int dy_pitch, const float* dymask, int mask_pitch, float slope,
                                   const float* packed_dgrad, float* dx, int dx_pitch, int cin, int accumulate, int B, int H,
                                   int W, void* stream) {
  if (!dy || !packed_dgrad || !dx || !dn_dims_ok(B, H, W) || !dn_slope_ok(slope)) return SISR_ERR_ARG;
  if (const int rc = dn_cin_code(cin)) return rc;
  if (!dn_pitch_ok(dy_pitch, DN_GROW) || !dn_pitch_ok(dx_pitch, cin) || (dymask && !dn_pitch_ok(mask_pitch, DN_GROW)))
    return SISR_ERR_ARG;
  if (!sisr_aligned16(dy) || !sisr_aligned16(dymask) || !sisr_aligned16(packed_dgrad) || !sisr_aligned16(dx))
    return SISR_ERR_ALIGN;
  const long npix = (long)B * H * W;
  if (dn_clash(dy, dy_pitch, DN_GROW, dx, dx_pitch, cin, npix)) return SISR_ERR_ARG;
  if (dymask && dn_clash(dymask, mask_pitch, DN_GROW, dx, dx_pitch, cin, npix)) return SISR_ERR_ARG;
  const dim3 grid((W + DN_TW - 1) / DN_TW, (H + DN_TH - 1) / DN_TH, B);
  hipStream_t s = (hipStream_t)stream;
#define DN_DGRAD(NT)                                                                                                          \
  hipLaunchKernelGGL((dn_dgrad_kernel<NT>), grid, dim3(256), 0, s, dy, dy_pitch, dymask, mask_pitch, slope, packed_dgrad, dx, \
                     dx_pitch, accumulate, H, W)
  switch (cin / 32) {
    case 2: DN_DGRAD(2); break;
    case 3: DN_DGRAD(3); break;
    case 4: DN_DGRAD(4); break;
    default: DN_DGRAD(5); break;
  }
#undef DN_DGRAD
  return sisr_check_launch();
}

// ------------------------------------------------------------------------------------------------ weight gradient
// Workgroup (slice s, chunk c) walks the pixel tiles s, s + S, s + 2 S, ... of the batch.  Per tile: the haloed tile of x's
// channels 32 c .. 32 c + 31 and the tile of dy' go to LDS once; wave v takes rows 2v, 2v + 1, and for every pixel pair one
// read of dy' (A: lane = output channel) meets nine shifted reads of x (B: lane = input channel): D_tap[co][ci] += dy' x.
static constexpr size_t DN_WGRAD_LDS = sizeof(float) * (DN_LH * DN_LW + DN_TH * DN_TW) * DN_WS;

__global__ __launch_bounds__(256) void dn_wgrad_kernel(const float* __restrict__ x, int xp, const float* __restrict__ dy,
                                                       int dyp, const float* __restrict__ mask, int mp, float slope,
                                                       float* __restrict__ part, float* __restrict__ dbpart, int H, int W,
                                                       int cin, int tiles, int tiles_h, int tiles_w) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xt = lds;                           // [DN_LH * DN_LW][DN_WS]; after the walk: the four waves' tiles of one tap
  float* dt = lds + DN_LH * DN_LW * DN_WS;   // [DN_TH * DN_TW][DN_WS]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5, i = lane & 31;
  const int s = blockIdx.x, S = gridDim.x, chunk = blockIdx.y;
  const bool with_bias = dbpart != nullptr && chunk == 0;
  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;
  for (int t = s; t < tiles; t += S) {
    const int b = t / (tiles_h * tiles_w), rem = t % (tiles_h * tiles_w);
    const int h0 = rem / tiles_w * DN_TH, w0 = rem % tiles_w * DN_TW;
    const long img = (long)b * H * W;
    __syncthreads();
    dn_stage<DN_WS, DN_LH, DN_LW, 1>(xt, x + chunk * 32, xp, nullptr, 0, 0.f, img, h0, w0, H, W, tid);
    dn_stage<DN_WS, DN_TH, DN_TW, 0>(dt, dy, dyp, mask, mp, slope, img, h0, w0, H, W, tid);
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int row = wave * 2 + mt;
      for (int u = 0; u < 16; ++u) {
        const int col = 2 * u + h;
        const float a = dt[(row * DN_TW + col) * DN_WS + i];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const float bv = xt[((row + kh) * DN_LW + col + kw) * DN_WS + i];
            acc[kh * 3 + kw] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[kh * 3 + kw], 0, 0, 0);
          }
      }
    }
    if (with_bias) {  // thread (row g, channel c): the 32 pixels of its row, in order
      const int c = tid & 31, g = tid >> 5;
      for (int col = 0; col < DN_TW; ++col) bsum += dt[(g * DN_TW + col) * DN_WS + c];
    }
  }
  float* out = part + (long)s * DN_GROW * cin * 9;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; ++r) xt[wave * 1024 + r * 64 + lane] = acc[t][r];
    __syncthreads();
    for (int e = tid; e < 1024; e += 256) {
      const int r = e >> 6, l = e & 63;
      const float v = ((xt[e] + xt[1024 + e]) + xt[2048 + e]) + xt[3072 + e];
      const int co = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), ci = chunk * 32 + (l & 31);
      out[((long)co * cin + ci) * 9 + t] = v;
    }
  }
  if (with_bias) {
    __syncthreads();
    xt[tid] = bsum;
    __syncthreads();
    if (tid < DN_GROW) {
      float v = xt[tid];
      for (int g = 1; g < 8; ++g) v += xt[g * 32 + tid];
      dbpart[s * DN_GROW + tid] = v;
    }
  }
}

__global__ __launch_bounds__(256) void dn_wgrad_final_kernel(const float* __restrict__ part, const float* __restrict__ dbpart,
                                                             int S, int n, float* __restrict__ dw, float* __restrict__ db) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) {
    float sum = 0.f;
    for (int k = 0; k < S; ++k) sum += part[(long)k * n + e];
    dw[e] = sum;
  } else if (db && e < n + DN_GROW) {
    float sum = 0.f;
    for (int k = 0; k < S; ++k) sum += dbpart[k * DN_GROW + (e - n)];
    db[e - n] = sum;
  }
}

static int dn_wgrad_tiles(int B, int H, int W) { return B * ((H + DN_TH - 1) / DN_TH) * ((W + DN_TW - 1) / DN_TW); }
static int dn_wgrad_slices(int B, int H, int W, int cin) {
  const int tiles = dn_wgrad_tiles(B, H, W), cap = DN_MAX_WG / (cin / 32);
  return tiles < cap ? tiles : cap;
}

extern "C" size_t sisr_dense3x3_wgrad_workspace_bytes(int B, int H, int W, int cin) {
  if (!dn_dims_ok(B, H, W) || dn_cin_code(cin)) return 0;
  return sizeof(float) * (size_t)dn_wgrad_slices(B, H, W, cin) * (DN_GROW * cin * 9 + DN_GROW);
}

extern "C" int sisr_dense3x3_wgrad(const float* x, int x_pitch, int cin, const float* dy, int dy_pitch, const float* dymask,
                                   int mask_pitch, float slope, float* dw, float* db, float* workspace, size_t workspace_bytes,
                                   int B, int H, int W, void* stream) {
  if (!x || !dy || !dw || !workspace || !dn_dims_ok(B, H, W) || !dn_slope_ok(slope)) return SISR_ERR_ARG;
  if (const int rc = dn_cin_code(cin)) return rc;
  if (!dn_pitch_ok(x_pitch, cin) || !dn_pitch_ok(dy_pitch, DN_GROW) || (dymask && !dn_pitch_ok(mask_pitch, DN_GROW)))
    return SISR_ERR_ARG;
  if (!sisr_aligned16(x) || !sisr_aligned16(dy) || !sisr_aligned16(dymask) || !sisr_aligned16(workspace)) return SISR_ERR_ALIGN;
  if (workspace_bytes < sisr_dense3x3_wgrad_workspace_bytes(B, H, W, cin)) return SISR_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int S = dn_wgrad_slices(B, H, W, cin), n = DN_GROW * cin * 9;
  float* dbpart = workspace + (size_t)S * n;
  SISR_ALLOW_LDS(dn_wgrad_kernel, DN_WGRAD_LDS);
  hipLaunchKernelGGL(dn_wgrad_kernel, dim3(S, cin / 32), dim3(256), DN_WGRAD_LDS, s, x, x_pitch, dy, dy_pitch, dymask,
                     mask_pitch, slope, workspace, db ? dbpart : nullptr, H, W, cin, dn_wgrad_tiles(B, H, W),
                     (H + DN_TH - 1) / DN_TH, (W + DN_TW - 1) / DN_TW);
  const int rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(dn_wgrad_final_kernel, dim3((n + DN_GROW + 255) / 256), dim3(256), 0, s, workspace, dbpart, S, n, dw, db);
  return sisr_check_launch();
}
