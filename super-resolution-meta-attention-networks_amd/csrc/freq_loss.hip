// Frequency-domain (FFT L1) training loss: the mean absolute real and imaginary part of the orthonormal 2-D DFT of
// sr - y over the half spectrum (H x (W/2 + 1) bins per plane), and its gradient with respect to sr
// (frequency.FrequencyMechanism: loss = base + beta * spectral_l1).
//
// The transform is a dense linear map, so it runs as matrix products on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32: bit for
// bit a k-ordered fmaf chain) against cached cosine / sine tables -- any H x W, no radix cases:
//   d = sr - y                                        (formed on load)
//   Tr = d Cw^T,  Ti = -d Sw^T                        rows:     [H x W] x [W x Wh]           freq_rows_kernel
//                                                     (d[j] +- d[W - j] folded before the product: K = Wh)
//   Fr = Ch Tr + Sh Ti,  Fi = Ch Ti - Sh Tr           columns:  [H x H] x [H x Wh], 4 products   freq_cols_kernel
//                                                     (rows u and H - u share them: only u <= H / 2 is multiplied out)
//   value = (sum |Fr| + sum |Fi|) / (n sqrt(HW)),  n = 2 P H Wh
// |Fr| + |Fi| goes from the accumulators into one float64 partial per workgroup; freq_finish_kernel adds the partials in
// a fixed order and rounds to fp32 once.  The spectrum never reaches memory: with a gradient, one byte per bin holds
// sign(Fr) and sign(Fi) (two 2-bit fields, value + 1).  The gradient is the transposed map on the signs:
//   Gr = Ch sr_ - Sh si_,  -Gi = -(Sh sr_ + Ch si_)   freq_cols_kernel again, its B operand decoded from the sign bytes
//   grad = (Gr Cw + (-Gi) Sw) / (n sqrt(HW))          [H x Wh] x [Wh x W]                     freq_grad_kernel
//                                                     (columns j and W - j share the two products: only j <= W / 2)
// Tables (freq_tables_kernel): C[k][j] = cos(2 pi r / N), S[k][j] = sin(2 pi r / N), r = k j mod N in integers, sincospi of
// the reduced fraction in float64, rounded to fp32 once: exactly 0 / +-1 at quarter turns.  With those, Ti is an exact zero
// in the columns v = 0 and v = W / 2, and Fi in the rows u = 0 and u = H / 2 of those columns: sums of exact zeros.  sign(0)
// is 0, so the structural zeros take no gradient, and equal images give value 0 and an all-zero gradient.
//
// Every product kernel: a workgroup of four waves makes a 64 x 64 output tile of one plane, each wave a 32 x 32 MFMA tile,
// K in steps of 32.  Operand tiles sit in LDS as [row][k] with a row pitch of 33 floats, which serves both the k-contiguous
// and the row-contiguous global layouts without bank conflicts, on the store and on the MFMA operand read (lane l reads row
// l & 31, k = 2 s + (l >> 5)).  The next K step's global loads are issued into registers before the MFMAs of this one.  All
// loads are clamped into the array and masked to zero outside it: M, N and K remainders cost nothing but idle lanes.
// No atomics, no allocation, no host synchronisation: capturable, and a repeat call is bit-identical.
#include "sisr_common.h"
#include <math.h>

#define FQ_T 64      // output tile side per workgroup
#define FQ_K 32      // K step
#define FQ_P 33      // LDS row pitch in floats
#define FQ_E 8       // elements of one 64 x 32 operand tile per thread (256 threads)
#define FQ_MAX_SIDE 4096

static inline long fq_div_up(long a, long b) { return (a + b - 1) / b; }
static inline int fq_half(int w) { return w / 2 + 1; }

// where thread t keeps element e of a 64 x 32 operand tile.  KC: the global array is k-contiguous (consecutive lanes take
// consecutive k); otherwise it is row-contiguous (consecutive lanes take consecutive rows).
template <bool KC>
__device__ __forceinline__ void fq_slot(int t, int e, int& row, int& k) {
  if (KC) {
    k = t & 31;
    row = (t >> 5) + 8 * e;
  } else {
    row = t & 63;
    k = (t >> 6) + 4 * e;
  }
}

__device__ __forceinline__ float fq_keep_if(float v, bool ok) {
  return __builtin_bit_cast(float, __builtin_bit_cast(unsigned, v) & (ok ? 0xffffffffu : 0u));
}

// the MFMA result layout: register r of lane l is row (r & 3) + 8 (r >> 2) + 4 (l >> 5), column l & 31
__device__ __forceinline__ int fq_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// ---------------------------------------------------------------------------------------------------------------- tables
// blob: Ch [h][h], Sh [h][h], Cw [wh][w], Sw [wh][w]
__global__ __launch_bounds__(256) void freq_tables_kernel(int h, int w, float* __restrict__ out) {
  const int wh = w / 2 + 1;
  const long nh = (long)h * h, nw = (long)wh * w;
  const long total = 2 * nh + 2 * nw;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    long e = i;
    int n, cols;
    bool sine;
    if (e < 2 * nh) {
      sine = e >= nh;
      e -= sine ? nh : 0;
      n = h;
      cols = h;
    } else {
      e -= 2 * nh;
      sine = e >= nw;
      e -= sine ? nw : 0;
      n = w;
      cols = w;
    }
    const int k = (int)(e / cols), j = (int)(e - (long)k * cols);
    const int r = (int)(((long)k * j) % n);
    double s, c;
    sincospi(2.0 * (double)r / (double)n, &s, &c);
    out[i] = (float)(sine ? s : c);
  }
}

// ---------------------------------------------------------------------------------------------------------------- rows
// Tr[p][i][v] = sum_j d[i][j] Cw[v][j],  Ti[p][i][v] = -sum_j d[i][j] Sw[v][j].  Cw[v][w - j] = Cw[v][j] and
// Sw[v][w - j] = -Sw[v][j], so the row is folded before the product and K is wh instead of w:
//   e[j] = d[j] + d[w - j],  o[j] = d[j] - d[w - j]   (0 < j < w - j;  e[j] = d[j], o[j] = 0 at j = 0 and j = w / 2)
//   Tr[v] = sum_{j < wh} e[j] Cw[v][j],  Ti[v] = -sum_{j < wh} o[j] Sw[v][j]
// grid: (Wh tiles, H tiles, planes)
__global__ __launch_bounds__(256) void freq_rows_kernel(const float* __restrict__ sr, const float* __restrict__ y, int h,
                                                        int w, int wh, const float* __restrict__ cw,
                                                        const float* __restrict__ sw, float* __restrict__ tr,
                                                        float* __restrict__ ti) {
  __shared__ float le[FQ_T * FQ_P], lo[FQ_T * FQ_P], lc[FQ_T * FQ_P], ls[FQ_T * FQ_P];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.y * FQ_T, n0 = blockIdx.x * FQ_T;
  const long plane = (long)blockIdx.z * h * w;
  float re[FQ_E], ro[FQ_E], rc[FQ_E], rs[FQ_E];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int e = 0; e < FQ_E; ++e) {
      int row, k;
      fq_slot<true>(t, e, row, k);
      const int j = k0 + k, i = m0 + row, v = n0 + row;
      const int jc = min(j, wh - 1), j2 = w - jc;          // j2 in [w - wh + 1, w]
      const bool pair = jc > 0 && j2 > jc;                  // d[w - j] is another pixel than d[j]
      const long ra = plane + (long)min(i, h - 1) * w;
      const long ia = ra + jc, ia2 = ra + (pair ? j2 : jc), ib = (long)min(v, wh - 1) * w + jc;
      const float d1 = sr[ia] - y[ia], d2 = fq_keep_if(sr[ia2] - y[ia2], pair);
      re[e] = fq_keep_if(d1 + d2, j < wh && i < h);
      ro[e] = fq_keep_if(d1 - d2, j < wh && i < h && pair);
      rc[e] = fq_keep_if(cw[ib], j < wh && v < wh);
      rs[e] = fq_keep_if(sw[ib], j < wh && v < wh);
    }
  };
  f32x16 accr = {0}, acci = {0};
  const int ao = ((wave >> 1) * 32 + (lane & 31)) * FQ_P + (lane >> 5);
  const int bo = ((wave & 1) * 32 + (lane & 31)) * FQ_P + (lane >> 5);
  fetch(0);
  for (int k0 = 0; k0 < wh; k0 += FQ_K) {
#pragma unroll
    for (int e = 0; e < FQ_E; ++e) {
      int row, k;
      fq_slot<true>(t, e, row, k);
      le[row * FQ_P + k] = re[e];
      lo[row * FQ_P + k] = ro[e];
      lc[row * FQ_P + k] = rc[e];
      ls[row * FQ_P + k] = rs[e];
    }
    __syncthreads();
    if (k0 + FQ_K < wh) fetch(k0 + FQ_K);
#pragma unroll
    for (int s = 0; s < FQ_K / 2; ++s) {
      accr = __builtin_amdgcn_mfma_f32_32x32x2f32(le[ao + 2 * s], lc[bo + 2 * s], accr, 0, 0, 0);
      acci = __builtin_amdgcn_mfma_f32_32x32x2f32(lo[ao + 2 * s], ls[bo + 2 * s], acci, 0, 0, 0);
    }
    __syncthreads();
  }
  const int v = n0 + (wave & 1) * 32 + (lane & 31);
  if (v < wh) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = m0 + (wave >> 1) * 32 + fq_acc_row(r, lane);
      if (i < h) {
        const long o = ((long)blockIdx.z * h + i) * wh + v;
        tr[o] = accr[r];
        ti[o] = -acci[r];
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- columns
// R[u][v] = sum_i Ch[u][i] X[i][v] + Sh[u][i] Y[i][v],  I[u][v] = sum_i Ch[u][i] Y[i][v] - Sh[u][i] X[i][v]
//   MODE 0: X = Tr, Y = Ti; |R| + |I| into this workgroup's float64 partial
//   MODE 1: the same, and sign(R), sign(I) into the byte map
//   MODE 2: X = sign(Fr), Y = -sign(Fi) from the byte map; R (= Gr) and I (= -Gi) stored as fp32
// Ch[h - u][i] = Ch[u][i] and Sh[h - u][i] = -Sh[u][i], so rows u and h - u share their four products
//   p1 = Ch X, p2 = Sh Y, p3 = Ch Y, p4 = Sh X:   R[u] = p1 + p2, I[u] = p3 - p4;   R[h - u] = p1 - p2, I[h - u] = p3 + p4
// and only the rows u <= h / 2 are multiplied out (hh = h / 2 + 1 of them), each kept in four accumulators; rows 0 and, for
// even h, h / 2 have no partner.  grid: (Wh tiles, hh tiles, planes)
template <int MODE>
__global__ __launch_bounds__(256) void freq_cols_kernel(const float* __restrict__ ch, const float* __restrict__ sh,
                                                        const float* __restrict__ xin, const float* __restrict__ yin,
                                                        unsigned char* __restrict__ sgn, int h, int wh,
                                                        float* __restrict__ outr, float* __restrict__ outi,
                                                        double* __restrict__ part) {
  __shared__ float lc[FQ_T * FQ_P], ls[FQ_T * FQ_P], lx[FQ_T * FQ_P], ly[FQ_T * FQ_P];
  __shared__ double red[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.y * FQ_T, n0 = blockIdx.x * FQ_T;
  const int hh = h / 2 + 1;
  const long plane = (long)blockIdx.z * h * wh;
  float rc[FQ_E], rs[FQ_E], rx[FQ_E], ry[FQ_E];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int e = 0; e < FQ_E; ++e) {
      int row, k;
      fq_slot<true>(t, e, row, k);
      const int u = m0 + row, i = k0 + k;
      const long ia = (long)min(u, hh - 1) * h + min(i, h - 1);
      rc[e] = fq_keep_if(ch[ia], u < hh && i < h);
      rs[e] = fq_keep_if(sh[ia], u < hh && i < h);
    }
#pragma unroll
    for (int e = 0; e < FQ_E; ++e) {
      int row, k;
      fq_slot<false>(t, e, row, k);
      const int v = n0 + row, i = k0 + k;
      const long ib = plane + (long)min(i, h - 1) * wh + min(v, wh - 1);
      const bool ok = v < wh && i < h;
      if (MODE == 2) {
        const int b = sgn[ib];
        rx[e] = ok ? (float)((b & 3) - 1) : 0.f;
        ry[e] = ok ? (float)(1 - ((b >> 2) & 3)) : 0.f;
      } else {
        rx[e] = fq_keep_if(xin[ib], ok);
        ry[e] = fq_keep_if(yin[ib], ok);
      }
    }
  };
  f32x16 p1 = {0}, p2 = {0}, p3 = {0}, p4 = {0};
  const int ao = ((wave >> 1) * 32 + (lane & 31)) * FQ_P + (lane >> 5);
  const int bo = ((wave & 1) * 32 + (lane & 31)) * FQ_P + (lane >> 5);
  fetch(0);
  for (int k0 = 0; k0 < h; k0 += FQ_K) {
#pragma unroll
    for (int e = 0; e < FQ_E; ++e) {
      int row, k;
      fq_slot<true>(t, e, row, k);
      lc[row * FQ_P + k] = rc[e];
      ls[row * FQ_P + k] = rs[e];
      fq_slot<false>(t, e, row, k);
      lx[row * FQ_P + k] = rx[e];
      ly[row * FQ_P + k] = ry[e];
    }
    __syncthreads();
    if (k0 + FQ_K < h) fetch(k0 + FQ_K);
#pragma unroll
    for (int s = 0; s < FQ_K / 2; ++s) {
      const float ac = lc[ao + 2 * s], as = ls[ao + 2 * s], bx = lx[bo + 2 * s], by = ly[bo + 2 * s];
      p1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, bx, p1, 0, 0, 0);
      p2 = __builtin_amdgcn_mfma_f32_32x32x2f32(as, by, p2, 0, 0, 0);
      p3 = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, by, p3, 0, 0, 0);
      p4 = __builtin_amdgcn_mfma_f32_32x32x2f32(as, bx, p4, 0, 0, 0);
    }
    __syncthreads();
  }
  const int v = n0 + (wave & 1) * 32 + (lane & 31);
  double sum = 0.0;
  auto emit = [&](int u, float fr, float fi) {  // one bin of row u < h, column v < wh
    const long o = plane + (long)u * wh + v;
    if (MODE == 2) {
      outr[o] = fr;
      outi[o] = fi;
    } else {
      sum += (double)fabsf(fr) + (double)fabsf(fi);
      if (MODE == 1) {
        const int a = (fr > 0.f) - (fr < 0.f) + 1, b = (fi > 0.f) - (fi < 0.f) + 1;
        sgn[o] = (unsigned char)(a | (b << 2));
      }
    }
  };
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int u = m0 + (wave >> 1) * 32 + fq_acc_row(r, lane);
    if (u < hh && v < wh) {
      emit(u, p1[r] + p2[r], p3[r] - p4[r]);
      if (u > 0 && h - u > u) emit(h - u, p1[r] - p2[r], p3[r] + p4[r]);  // h - u >= hh: no other row writes it
    }
  }
  if (MODE != 2) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) red[wave] = sum;
    __syncthreads();
    if (t == 0)
      part[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}

// ---------------------------------------------------------------------------------------------------------------- gradient
// grad[p][i][j] = scale * sum_v (G1[i][v] Cw[v][j] + G2[i][v] Sw[v][j]).  The first sum E is even in j about w / 2 and the
// second, O, odd, so only the columns j < wh are multiplied out, each in two accumulators:
//   grad[j] = E[j] + O[j],  grad[w - j] = E[j] - O[j]   (0 < j < w - j)
// grid: (Wh tiles, H tiles, planes)
__global__ __launch_bounds__(256) void freq_grad_kernel(const float* __restrict__ g1, const float* __restrict__ g2, int h,
                                                        int w, int wh, const float* __restrict__ cw,
                                                        const float* __restrict__ sw, double scale,
                                                        float* __restrict__ grad) {
  __shared__ float l1[FQ_T * FQ_P], l2[FQ_T * FQ_P], lc[FQ_T * FQ_P], ls[FQ_T * FQ_P];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int m0 = blockIdx.y * FQ_T, n0 = blockIdx.x * FQ_T;
  const long plane = (long)blockIdx.z * h * wh;
  float r1[FQ_E], r2[FQ_E], rc[FQ_E], rs[FQ_E];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int e = 0; e < FQ_E; ++e) {
      int row, k;
      fq_slot<true>(t, e, row, k);
      const int i = m0 + row, v = k0 + k;
      const long ia = plane + (long)min(i, h - 1) * wh + min(v, wh - 1);
      r1[e] = fq_keep_if(g1[ia], i < h && v < wh);
      r2[e] = fq_keep_if(g2[ia], i < h && v < wh);
    }
#pragma unroll
    for (int e = 0; e < FQ_E; ++e) {
      int row, k;
      fq_slot<false>(t, e, row, k);
      const int j = n0 + row, v = k0 + k;
      const long ib = (long)min(v, wh - 1) * w + min(j, wh - 1);
      rc[e] = fq_keep_if(cw[ib], j < wh && v < wh);
      rs[e] = fq_keep_if(sw[ib], j < wh && v < wh);
    }
  };
  f32x16 acce = {0}, acco = {0};
  const int ao = ((wave >> 1) * 32 + (lane & 31)) * FQ_P + (lane >> 5);
  const int bo = ((wave & 1) * 32 + (lane & 31)) * FQ_P + (lane >> 5);
  fetch(0);
  for (int k0 = 0; k0 < wh; k0 += FQ_K) {
#pragma unroll
    for (int e = 0; e < FQ_E; ++e) {
      int row, k;
      fq_slot<true>(t, e, row, k);
      l1[row * FQ_P + k] = r1[e];
      l2[row * FQ_P + k] = r2[e];
      fq_slot<false>(t, e, row, k);
      lc[row * FQ_P + k] = rc[e];
      ls[row * FQ_P + k] = rs[e];
    }
    __syncthreads();
    if (k0 + FQ_K < wh) fetch(k0 + FQ_K);
#pragma unroll
    for (int s = 0; s < FQ_K / 2; ++s) {
      acce = __builtin_amdgcn_mfma_f32_32x32x2f32(l1[ao + 2 * s], lc[bo + 2 * s], acce, 0, 0, 0);
      acco = __builtin_amdgcn_mfma_f32_32x32x2f32(l2[ao + 2 * s], ls[bo + 2 * s], acco, 0, 0, 0);
    }
    __syncthreads();
  }
  const int j = n0 + (wave & 1) * 32 + (lane & 31);
  if (j < wh) {
    const bool pair = j > 0 && w - j > j;  // w - j >= wh: no other column writes it
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = m0 + (wave >> 1) * 32 + fq_acc_row(r, lane);
      if (i < h) {
        const long o = ((long)blockIdx.z * h + i) * w;
        grad[o + j] = (float)((double)(acce[r] + acco[r]) * scale);
        if (pair) grad[o + w - j] = (float)((double)(acce[r] - acco[r]) * scale);
      }
    }
  }
}

// value = (sum of all workgroup partials, in a fixed order) * mult, rounded to fp32 once
__global__ __launch_bounds__(256) void freq_finish_kernel(const double* __restrict__ part, long n_part, double mult,
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
  if (threadIdx.x == 0) value[0] = (float)(red[0] * mult);
}

// ---------------------------------------------------------------------------------------------------------------- host
static inline bool fq_sides_ok(int h, int w) { return h >= 2 && w >= 2 && h <= FQ_MAX_SIDE && w <= FQ_MAX_SIDE; }
static inline size_t fq_pad16(size_t n) { return (n + 15) & ~(size_t)15; }
// workgroups of the columns kernel per plane: it multiplies out the rows u <= h / 2 only
static inline long fq_tiles(int h, int w) { return fq_div_up(h / 2 + 1, FQ_T) * fq_div_up(fq_half(w), FQ_T); }
// workspace: [planes * tiles] float64 partials | two [planes][h][wh] fp32 maps (Tr, Ti; then Gr, -Gi) | with a gradient,
// [planes][h][wh] sign bytes; every part padded to 16 bytes
static inline size_t fq_part_bytes(long planes, int h, int w) { return fq_pad16((size_t)planes * fq_tiles(h, w) * sizeof(double)); }
static inline size_t fq_map_bytes(long planes, int h, int w) {
  return fq_pad16((size_t)planes * (size_t)h * (size_t)fq_half(w) * sizeof(float));
}

extern "C" size_t sisr_freq_loss_table_bytes(int h, int w) {
  if (!fq_sides_ok(h, w)) return 0;
  return (2 * (size_t)h * h + 2 * (size_t)fq_half(w) * w) * sizeof(float);
}

extern "C" int sisr_freq_loss_tables(int h, int w, float* tables, void* stream) {
  if (!tables || !fq_sides_ok(h, w)) return SISR_ERR_ARG;
  if ((uintptr_t)tables & 3) return SISR_ERR_ALIGN;
  const long total = (long)(sisr_freq_loss_table_bytes(h, w) / sizeof(float));
  const long blocks = fq_div_up(total, 256);
  hipLaunchKernelGGL(freq_tables_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream,
                     h, w, tables);
  return sisr_check_launch();
}

extern "C" size_t sisr_freq_loss_workspace_bytes(int planes, int h, int w, int want_grad) {
  if (planes < 1 || !fq_sides_ok(h, w)) return 0;
  size_t n = fq_part_bytes(planes, h, w) + 2 * fq_map_bytes(planes, h, w);
  if (want_grad) n += fq_pad16((size_t)planes * (size_t)h * (size_t)fq_half(w));
  return n;
}

extern "C" int sisr_freq_loss(const float* sr, const float* y, int planes, int h, int w, const float* tables, float* value,
                              float* grad, void* workspace, size_t workspace_bytes, void* stream) {
  if (!sr || !y || !tables || !value || !workspace || planes < 1 || !fq_sides_ok(h, w)) return SISR_ERR_ARG;
  if (workspace_bytes < sisr_freq_loss_workspace_bytes(planes, h, w, grad != nullptr)) return SISR_ERR_ARG;
  if (!sisr_aligned16(workspace) || ((uintptr_t)sr & 3) || ((uintptr_t)y & 3) || ((uintptr_t)tables & 3) ||
      ((uintptr_t)value & 3) || ((uintptr_t)grad & 3))
    return SISR_ERR_ALIGN;
  if (planes > 65535) return SISR_ERR_UNSUPPORTED;  // the plane is the grid's z
  const int wh = fq_half(w);
  const float* ch = tables;
  const float* sh = ch + (size_t)h * h;
  const float* cw = sh + (size_t)h * h;
  const float* sw = cw + (size_t)wh * w;
  char* ws = static_cast<char*>(workspace);
  double* part = reinterpret_cast<double*>(ws);
  float* m1 = reinterpret_cast<float*>(ws + fq_part_bytes(planes, h, w));
  float* m2 = reinterpret_cast<float*>(ws + fq_part_bytes(planes, h, w) + fq_map_bytes(planes, h, w));
  unsigned char* sgn = reinterpret_cast<unsigned char*>(ws + fq_part_bytes(planes, h, w) + 2 * fq_map_bytes(planes, h, w));
  const hipStream_t s = (hipStream_t)stream;
  const dim3 gh((unsigned)fq_div_up(wh, FQ_T), (unsigned)fq_div_up(h, FQ_T), (unsigned)planes);  // half-spectrum grid; the gradient's too: columns j <= w / 2
  const dim3 gc(gh.x, (unsigned)fq_div_up(h / 2 + 1, FQ_T), (unsigned)planes);                      // rows u <= h / 2 of the spectrum
  const double root = sqrt((double)h * (double)w), n = 2.0 * (double)planes * (double)h * (double)wh;

  hipLaunchKernelGGL(freq_rows_kernel, gh, dim3(256), 0, s, sr, y, h, w, wh, cw, sw, m1, m2);
  int rc = sisr_check_launch();
  if (rc) return rc;
  if (grad)
    hipLaunchKernelGGL(freq_cols_kernel<1>, gc, dim3(256), 0, s, ch, sh, (const float*)m1, (const float*)m2, sgn, h, wh,
                       (float*)nullptr, (float*)nullptr, part);
  else
    hipLaunchKernelGGL(freq_cols_kernel<0>, gc, dim3(256), 0, s, ch, sh, (const float*)m1, (const float*)m2,
                       (unsigned char*)nullptr, h, wh, (float*)nullptr, (float*)nullptr, part);
  rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(freq_finish_kernel, dim3(1), dim3(256), 0, s, part, (long)planes * fq_tiles(h, w), 1.0 / (n * root),
                     value);
  rc = sisr_check_launch();
  if (rc || !grad) return rc;
  // the maps have been consumed: they now take Gr and -Gi
  hipLaunchKernelGGL(freq_cols_kernel<2>, gc, dim3(256), 0, s, ch, sh, (const float*)nullptr, (const float*)nullptr, sgn, h,
                     wh, m1, m2, (double*)nullptr);
  rc = sisr_check_launch();
  if (rc) return rc;
  hipLaunchKernelGGL(freq_grad_kernel, gh, dim3(256), 0, s, (const float*)m1, (const float*)m2, h, w, wh, cw, sw,
                     1.0 / (n * root), grad);
  return sisr_check_launch();
}
