// Tile-level online degradation (`[data] degrade_tiles = true`): a training batch's LR and HR tiles straight from the
// device-resident HR images, without a whole-image intermediate.  The whole-image path (degrade.hip + jpeg.hip, driven per
// sample by degrade.OnlineDegrader) blurs, quantises and resamples the full image and then cuts a tile; blur, quantisation
// and PIL's two resample passes are local, so the tile can be computed from the HR window it depends on, with the same bytes:
//   * the blur is the same fp32 fmaf sum over the taps in row-major order, reflection against the IMAGE (not the window);
//   * the resample passes index the whole-image coefficient tables at the tile's absolute LR rows / columns, so tiles at the
//     border get Pillow's clipped, renormalised taps; the window a strip needs is read off those tables' bounds.
// sisr_degrade_tiles: one workgroup per (strip of DT_ROWS LR rows, channel, sample).  The blurred, quantised HR window of the
// strip and the horizontal pass's rows stay in LDS (the pattern of interp.hip's pil_upsample); the fp32 source is staged in
// column chunks.  Noise, when on, is the counter-based field of noise_field.h evaluated at the pixel's position in the full
// image.  sisr_jpeg_roundtrip_batch: the JPEG round trip of jpeg.hip on every tile of the batch in one launch, block grid at
// the tile's origin, one quality per sample read from the device, the scaled tables built in the kernel.
// sisr_crop_augment_strided: the HR tiles gathered from the full images with the centre-crop offset in the address.
// Every launch count is a constant; nothing is allocated, copied or synchronised here.
#include "degrade_common.h"
#include "jpeg_block.h"
#include "noise_field.h"

#define DT_ROWS 8             // LR rows per strip
#define DT_THREADS 512        // two waves per SIMD and workgroup: one alone leaves the LDS latency of the blur loop exposed
#define DT_BC 64              // most blurred columns per source chunk (a multiple of 4)
#define DT_SP (DT_BC + 24)    // row pitch of the staged source chunk in floats: DT_BC + BL_MAX - 1 columns + the read-ahead
#define DT_LDS_MAX 65536

struct DegradeTile {  // sisr_degrade_tile of include/sisr_hip.h
  const float* image;
  const int *bounds_h, *coef_h, *bounds_v, *coef_v;
  int H, W, t0, l0, rh, rw, ty, tx;
  int ksize_h, ksize_v, flips, noise;
  float sigma;
  unsigned seed;
};

__host__ __device__ static inline int dt_up16(int n) { return (n + 15) & ~15; }

template <bool TO_FLOAT>
__global__ __launch_bounds__(DT_THREADS) void degrade_tiles_kernel(const DegradeTile* __restrict__ recs, const float* __restrict__ kernels,
                                                            void* __restrict__ outp, int C, int c, int l, int wr_cap, int wc_pitch) {
  extern __shared__ __align__(16) unsigned char dt_smem[];
  const DegradeTile t = recs[blockIdx.z];
  const int tid = threadIdx.x, ch = blockIdx.y, r0 = blockIdx.x * DT_ROWS;
  const int nr = min(DT_ROWS, c - r0);
  const int ksh = t.ksize_h, ksv = t.ksize_v;

  float* kk = reinterpret_cast<float*>(dt_smem);
  float* src = kk + dt_up16(BL_MAX * BL_MAX);
  int* chs = reinterpret_cast<int*>(src + (wr_cap + BL_MAX - 1) * DT_SP);
  int* bnd = chs + dt_up16(c * ksh);
  unsigned char* win = reinterpret_cast<unsigned char*>(bnd + dt_up16(2 * c));
  unsigned char* hp = win + dt_up16(wr_cap * wc_pitch);

  // the HR window of this strip, in crop-box coordinates, from the tables' bounds (first tap, taps)
  const int ov0 = t.ty + r0, ov1 = ov0 + nr - 1, oh1 = t.tx + c - 1;
  const int vlo = t.bounds_v[2 * ov0], hlo = t.bounds_h[2 * t.tx];
  const int nrows = min(t.bounds_v[2 * ov1] + t.bounds_v[2 * ov1 + 1] - vlo, wr_cap);
  const int ncols = min(t.bounds_h[2 * oh1] + t.bounds_h[2 * oh1 + 1] - hlo, wc_pitch);

  for (int i = tid; i < l * l; i += DT_THREADS) kk[i] = kernels[(long)blockIdx.z * l * l + i];
  for (int i = tid; i < c * ksh; i += DT_THREADS) chs[i] = t.coef_h[(long)t.tx * ksh + i];
  for (int i = tid; i < 2 * c; i += DT_THREADS) bnd[i] = t.bounds_h[2 * t.tx + i];

  // ---- blur (+ noise) + quantisation of the window, DT_BC-column chunks of the source at a time
  const int pl = l / 2;  // odd l: l/2 both sides; even l: (l/2, l/2 - 1), as blur_quant_kernel
  const int nch = (ncols + DT_BC - 1) / DT_BC;
  const int BC = nch > 0 ? (((ncols + nch - 1) / nch + 3) & ~3) : 4;
  const float* img = t.image + (long)ch * t.H * t.W;
  const int y0 = t.t0 + vlo - pl, srows = nrows + l - 1, scols = BC + l - 1, q4 = BC >> 2;
  const bool noisy = t.noise != 0 && t.sigma != 0.f;  // sigma = 0: noise * 0 + blur = blur, only the clamp is left
  for (int cb = 0; cb < ncols; cb += BC) {
    __syncthreads();  // the previous chunk's readers are done (first pass: nothing to wait for)
    const int x0 = t.l0 + hlo + cb - pl;
    for (int i = tid; i < srows * scols; i += DT_THREADS) {
      const int rr = i / scols, qq = i - rr * scols;
      src[rr * DT_SP + qq] = img[(long)reflect_index(y0 + rr, t.H) * t.W + reflect_index(x0 + qq, t.W)];
    }
    __syncthreads();
    for (int it = tid; it < nrows * q4; it += DT_THREADS) {
      const int r = it / q4, q = (it - r * q4) << 2;
      float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;  // four neighbouring outputs; each sums its taps in row-major order
      for (int i = 0; i < l; ++i) {
        const float* trow = src + (r + i) * DT_SP + q;
        const float* krow = kk + i * l;
        f32x4 a = *reinterpret_cast<const f32x4*>(trow);
        for (int j = 0; j < l; j += 4) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(trow + j + 4);
          const float v[7] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z};
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            if (j + jj < l) {
              const float k = krow[j + jj];
              acc0 = __builtin_fmaf(v[jj], k, acc0);
              acc1 = __builtin_fmaf(v[jj + 1], k, acc1);
              acc2 = __builtin_fmaf(v[jj + 2], k, acc2);
              acc3 = __builtin_fmaf(v[jj + 3], k, acc3);
            }
          }
          a = b;
        }
      }
      const float acc[4] = {acc0, acc1, acc2, acc3};
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int col = cb + q + m;
        if (col >= ncols) continue;
        unsigned char v;
        if (t.noise) {
          const float nz = noisy ? sisr_normal_at(t.seed, ch, t.t0 + vlo + r, t.l0 + hlo + col) : 0.f;
          v = dg_noise_quant(acc[m], nz, t.sigma);
        } else {
          v = dg_quant(acc[m]);
        }
        win[r * wc_pitch + col] = v;
      }
    }
  }
  __syncthreads();

  // ---- PIL's horizontal pass over every window row: whole-image table entries tx .. tx + c - 1
  for (int it = tid; it < nrows * c; it += DT_THREADS) {
    const int r = it / c, x = it - r * c;
    const int n = min(bnd[2 * x + 1], ksh);
    const unsigned char* wp = win + r * wc_pitch + (bnd[2 * x] - hlo);
    const int* kp = chs + x * ksh;
    int ss = 1 << 21;
    for (int k = 0; k < n; ++k) ss += (int)wp[k] * kp[k];
    hp[r * c + x] = (unsigned char)dg_clip8(ss);
  }
  __syncthreads();

  // ---- PIL's vertical pass for the strip's rows, stored through the flips / transpose
  const long plane = (long)c * c;
  for (int it = tid; it < nr * c; it += DT_THREADS) {
    const int y = it / c, x = it - y * c, o = ov0 + y;
    const int n = min(t.bounds_v[2 * o + 1], ksv);
    const unsigned char* cp = hp + (t.bounds_v[2 * o] - vlo) * c + x;
    const int* kp = t.coef_v + (long)o * ksv;
    int ss = 1 << 21;
    for (int k = 0; k < n; ++k) ss += (int)cp[k * c] * kp[k];
    const int v = dg_clip8(ss);
    const long at = ((long)blockIdx.z * C + ch) * plane + dt_store_index(r0 + y, x, c, t.flips);
    if (TO_FLOAT) static_cast<float*>(outp)[at] = (float)v / 255.0f;  // ToTensor: .float().div(255)
    else static_cast<unsigned char*>(outp)[at] = (unsigned char)v;
  }
}

static size_t dt_lds_bytes(int c, int scale, int* wr_cap, int* wc_pitch) {
  const int ks = 4 * scale + 1;  // pil_bicubic_table's ksize of an integer-factor reduction: ceil(2 s) * 2 + 1
  *wr_cap = (DT_ROWS - 1) * scale + ks;      // consecutive outputs' first taps are exactly `scale` apart (or clipped at 0)
  *wc_pitch = ((c - 1) * scale + ks + 3) & ~3;
  return 4 * (size_t)(dt_up16(BL_MAX * BL_MAX) + (*wr_cap + BL_MAX - 1) * DT_SP + dt_up16(c * ks) + dt_up16(2 * c)) +
         (size_t)dt_up16(*wr_cap * *wc_pitch) + (size_t)dt_up16(*wr_cap * c);
}

extern "C" size_t sisr_degrade_tile_bytes(void) { return sizeof(DegradeTile); }

extern "C" int sisr_degrade_tiles(const void* tiles_host, const void* tiles_dev, const float* kernels, void* out, int B, int C,
                                  int c, int l, int scale, int to_float, void* stream) {
  if (!tiles_host || !tiles_dev || !kernels || !out || B <= 0 || C <= 0 || c <= 0 || l < 1 || (to_float != 0 && to_float != 1))
    return SISR_ERR_ARG;
  if (scale < 2 || scale > 4 || l > BL_MAX || B > 65535 || C > 65535) return SISR_ERR_UNSUPPORTED;
  const DegradeTile* t = static_cast<const DegradeTile*>(tiles_host);
  for (int b = 0; b < B; ++b) {
    const DegradeTile& r = t[b];
    if (!r.image || r.H <= 0 || r.W <= 0 || r.rh <= 0 || r.rw <= 0 || r.t0 < 0 || r.l0 < 0 || r.ty < 0 || r.tx < 0 ||
        (long)r.t0 + r.rh > r.H || (long)r.l0 + r.rw > r.W || r.rh % scale || r.rw % scale || (r.flips & ~7) || r.sigma < 0.f)
      return SISR_ERR_ARG;
    if (!r.bounds_h || !r.coef_h || !r.bounds_v || !r.coef_v || r.ksize_h != 4 * scale + 1 || r.ksize_v != 4 * scale + 1)
      return SISR_ERR_ARG;  // the tables of this scale were not supplied
    if ((long)r.ty + c > r.rh / scale || (long)r.tx + c > r.rw / scale) return SISR_ERR_ARG;  // tile outside the LR image
    if (l / 2 >= r.H || l / 2 >= r.W) return SISR_ERR_UNSUPPORTED;  // reflection padding needs pad < size
  }
  int wr_cap, wc_pitch;
  const size_t lds = dt_lds_bytes(c, scale, &wr_cap, &wc_pitch);
  if (lds > DT_LDS_MAX) return SISR_ERR_UNSUPPORTED;
  const dim3 grid((c + DT_ROWS - 1) / DT_ROWS, C, B);
  const DegradeTile* td = static_cast<const DegradeTile*>(tiles_dev);
  if (to_float)
    hipLaunchKernelGGL((degrade_tiles_kernel<true>), grid, dim3(DT_THREADS), lds, (hipStream_t)stream, td, kernels, out, C, c, l, wr_cap,
                       wc_pitch);
  else
    hipLaunchKernelGGL((degrade_tiles_kernel<false>), grid, dim3(DT_THREADS), lds, (hipStream_t)stream, td, kernels, out, C, c, l, wr_cap,
                       wc_pitch);
  return sisr_check_launch();
}

// ---------------------------------------------------------------- JPEG round trip of every tile of a batch
// jpeg.hip's kernel with a sample index: in [B][C][c][c] uint8 in source orientation; the tile's own block grid; the
// quality of sample b from quality[b] (clamped to 1..100: the host cannot see a device value, degrade.degrade_tiles refuses
// others before the upload); out through the sample's flips.
template <int C, bool TO_FLOAT>
__global__ __launch_bounds__(JP_THREADS) void jpeg_roundtrip_batch_kernel(const unsigned char* __restrict__ in, void* __restrict__ outp,
                                                                          const int* __restrict__ quality,
                                                                          const int* __restrict__ flips, int c, int nbx,
                                                                          int nblocks) {
  __shared__ int tiles[JP_BLOCKS * 8 * JP_LD];
  __shared__ int qt[2][64];
  const int smp = blockIdx.y;
  if (threadIdx.x < 128) {
    const int q = min(max(quality[smp], 1), 100);
    qt[threadIdx.x >> 6][threadIdx.x & 63] = jp_scaled_entry(threadIdx.x >> 6, threadIdx.x & 63, q);
  }
  __syncthreads();
  const int lb = threadIdx.x >> 3, r = threadIdx.x & 7;
  int g = blockIdx.x * JP_BLOCKS + lb;
  const bool live = g < nblocks;
  if (!live) g = nblocks - 1;  // lanes past the last block keep the barriers company and store nothing
  const int by = g / nbx, bx = g - by * nbx;
  const int y = by * 8 + r, x0 = bx * 8;
  const long plane = (long)c * c, base = (long)smp * C * plane;
  const long row = (long)min(y, c - 1) * c;
  int* tile = tiles + lb * 8 * JP_LD;

  int p[C][8];
#pragma unroll
  for (int k = 0; k < C; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) p[k][j] = in[base + k * plane + row + min(x0 + j, c - 1)];

  constexpr int CB = C == 3 ? 1 : 0, CR = C == 3 ? 2 : 0;
  if (C == 3) jp_rgb_to_ycc(p[0], p[CB], p[CR]);
#pragma unroll
  for (int k = 0; k < C; ++k) jp_component(p[k], tile, qt[k ? 1 : 0], r);
  if (C == 3) jp_ycc_to_rgb(p[0], p[CB], p[CR]);

  if (!live || y >= c) return;
  const int fl = flips ? flips[smp] : 0;
#pragma unroll
  for (int k = 0; k < C; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (x0 + j >= c) continue;
      const long at = base + k * plane + dt_store_index(y, x0 + j, c, fl);
      if (TO_FLOAT) static_cast<float*>(outp)[at] = (float)p[k][j] / 255.0f;
      else static_cast<unsigned char*>(outp)[at] = (unsigned char)p[k][j];
    }
}

extern "C" int sisr_jpeg_roundtrip_batch(const unsigned char* in, void* out, const int* quality, const int* flips, int B, int C,
                                         int c, int to_float, void* stream) {
  if (!in || !out || !quality || in == out || B <= 0 || (C != 1 && C != 3) || c < 1 || (to_float != 0 && to_float != 1))
    return SISR_ERR_ARG;
  if (B > 65535 || c > 32768) return SISR_ERR_UNSUPPORTED;
  const int nbx = (c + 7) / 8, nblocks = nbx * nbx;
  const dim3 grid((unsigned)((nblocks + JP_BLOCKS - 1) / JP_BLOCKS), B), block(JP_THREADS);
  hipStream_t st = (hipStream_t)stream;
  if (C == 3) {
    if (to_float) hipLaunchKernelGGL((jpeg_roundtrip_batch_kernel<3, true>), grid, block, 0, st, in, out, quality, flips, c, nbx, nblocks);
    else hipLaunchKernelGGL((jpeg_roundtrip_batch_kernel<3, false>), grid, block, 0, st, in, out, quality, flips, c, nbx, nblocks);
  } else {
    if (to_float) hipLaunchKernelGGL((jpeg_roundtrip_batch_kernel<1, true>), grid, block, 0, st, in, out, quality, flips, c, nbx, nblocks);
    else hipLaunchKernelGGL((jpeg_roundtrip_batch_kernel<1, false>), grid, block, 0, st, in, out, quality, flips, c, nbx, nblocks);
  }
  return sisr_check_launch();
}

// ---------------------------------------------------------------- the noise field on its own
// field [C][H][W] fp32 and / or words [C][H][ceil(W / 4)][4]: the Philox output of every call
__global__ __launch_bounds__(256) void normal_field_kernel(unsigned seed, float* __restrict__ field, unsigned* __restrict__ words,
                                                           int C, int H, int W) {
  const long n = (long)C * H * W;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int x = (int)(i % W);
    const long t = i / W;
    const int y = (int)(t % H), ch = (int)(t / H);
    if (field) field[i] = sisr_normal_at(seed, ch, y, x);
    if (words && (x & 3) == 0) {
      unsigned w[4];
      sisr_philox4x32_10((unsigned)x >> 2, (unsigned)y, (unsigned)ch, 0u, seed, 0u, w);
      unsigned* wp = words + (((long)ch * H + y) * ((W + 3) / 4) + (x >> 2)) * 4;
      wp[0] = w[0];
      wp[1] = w[1];
      wp[2] = w[2];
      wp[3] = w[3];
    }
  }
}

extern "C" int sisr_normal_field(unsigned seed, float* field, unsigned* words, int C, int H, int W, void* stream) {
  if ((!field && !words) || C <= 0 || H <= 0 || W <= 0) return SISR_ERR_ARG;
  const long n = (long)C * H * W, blocks = (n + 255) / 256;
  hipLaunchKernelGGL(normal_field_kernel, dim3((unsigned)(blocks > 65535 ? 65535 : blocks)), dim3(256), 0, (hipStream_t)stream, seed,
                     field, words, C, H, W);
  return sisr_check_launch();
}

// ---------------------------------------------------------------- HR tiles from the full images
// sisr_crop_augment (misc.hip) on a centre-cropped image that is never copied out: params[b] = {rh, rw, top, left, hflip,
// vflip, transpose, H, W, t0, l0, 0}, the crop box (t0, l0, rh, rw) of the [C][H][W] image src[b]; (top, left) and the flips
// refer to the cropped image, exactly as sisr_crop_augment's do.
struct CropStridedRec {
  int rh, rw, top, left, hflip, vflip, rot, H, W, t0, l0, pad;
};

__global__ __launch_bounds__(256) void crop_augment_strided_kernel(const float* const* __restrict__ src,
                                                                   const CropStridedRec* __restrict__ prm, float* __restrict__ dst,
                                                                   int C, int crop) {
  const int b = blockIdx.z, c = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= crop * crop) return;
  const CropStridedRec r = prm[b];
  const int i = idx / crop, j = idx - i * crop;
  const int y = r.top + i, x = r.left + j;           // coordinates in the augmented image
  const int y2 = r.rot ? x : y, x2 = r.rot ? y : x;  // undo the transpose
  const int sy = r.vflip ? r.rh - 1 - y2 : y2, sx = r.hflip ? r.rw - 1 - x2 : x2;
  dst[(((long)b * C + c) * crop + i) * crop + j] = src[b][((long)c * r.H + r.t0 + sy) * r.W + r.l0 + sx];
}

extern "C" int sisr_crop_augment_strided(const float* const* src, const int* params_host, const int* params_dev, float* dst, int B,
                                         int C, int crop, void* stream) {
  if (!src || !params_host || !params_dev || !dst || B <= 0 || C <= 0 || crop <= 0 || B > 65535 || C > 65535) return SISR_ERR_ARG;
  const CropStridedRec* p = reinterpret_cast<const CropStridedRec*>(params_host);
  for (int b = 0; b < B; ++b) {
    const CropStridedRec& r = p[b];
    const int ah = r.rot ? r.rw : r.rh, aw = r.rot ? r.rh : r.rw;  // size of the augmented image
    if (r.rh <= 0 || r.rw <= 0 || r.t0 < 0 || r.l0 < 0 || (long)r.t0 + r.rh > r.H || (long)r.l0 + r.rw > r.W || r.top < 0 ||
        r.left < 0 || (long)r.top + crop > ah || (long)r.left + crop > aw)
      return SISR_ERR_ARG;
  }
  hipLaunchKernelGGL(crop_augment_strided_kernel, dim3((crop * crop + 255) / 256, C, B), dim3(256), 0, (hipStream_t)stream, src,
                     reinterpret_cast<const CropStridedRec*>(params_dev), dst, C, crop);
  return sisr_check_launch();
}
