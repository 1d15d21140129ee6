// Tile-level online degradation for the interpolated-input and the Y-channel models (`online_degradations` + `degrade_tiles`
// with `input = 'interp'` and / or `colorspace = 'ycbcr'`).
// sisr_upsample_tiles: a batch's c x c tiles of the bicubic pre-up-sampled LR images -- Pillow's
// `resize((w * s, h * s), BICUBIC)` of the LR bytes, ToTensor, optionally BT.601 'jpg' YCbCr or Y alone -- from the LR WINDOW
// each tile depends on (sisr_degrade_tiles' output), without the up-sampled image ever existing.  Both passes of
// libImaging/Resample.c are local, so a tile equals the crop of the whole up-sampled image bit for bit when the passes index
// the whole-image coefficient tables at the tile's absolute rows / columns and take their tap addresses relative to the
// window's origin.  A workgroup owns a 32 x 32 block of a tile in all three channels, exactly as interp.hip's kernel owns a
// block of the image (pil_upsample.h holds what the two share); the flips / transpose are applied on the store.
// sisr_rgb_to_ycbcr: the colour conversion on its own, for the HR tiles and for LR tiles that are not up-sampled.
#include "degrade_common.h"
#include "pil_upsample.h"

struct UpsampleTile {  // sisr_upsample_tile of include/sisr_hip.h
  const int *bounds_h, *coef_h, *bounds_v, *coef_v;
  int h, w, H, W, wy, wx, ty, tx, flips, pad;
};

enum { UPT_RGB = 0, UPT_YCBCR = 1, UPT_Y = 2 };

// win [B][C][cw][cw] uint8 -> out [B][C or 3 or 1][c][c] fp32.  grid (ceil(c / 32), ceil(c / 32), B * ceil(C / 3)).
// VEC: c % 4 == 0 and a 16-byte aligned output -- a lane stores its four pixels of a row as one 16-byte word unless the tile
// is transposed (then they lie a row apart).
template <bool VEC>
__global__ __launch_bounds__(256) void upsample_tiles_kernel(const UpsampleTile* __restrict__ recs, const unsigned char* __restrict__ win,
                                                             float* __restrict__ out, int C, int c, int cw, int form) {
  // (+ KS: a zero-weight tap past an output's own taps may read up to KS - 1 bytes / rows beyond the block)
  __shared__ unsigned char in_t[UC * UH * UH + KS];  // [ch][r][q]: the window bytes the block reads
  __shared__ unsigned tmp_t[UC * UH + KS][UT / 4];   // [ch * UH + r][x / 4]: its horizontally resampled rows
  __shared__ int kh[UT][KS], kv[UT][KS];
  __shared__ int fh[UT], fv[UT];
  const int groups = (C + UC - 1) / UC;
  const int b = blockIdx.z / groups, c0 = (blockIdx.z - b * groups) * UC;
  const int cn = C - c0 < UC ? C - c0 : UC;
  const UpsampleTile t = recs[b];
  const int x0 = blockIdx.x * UT, y0 = blockIdx.y * UT;  // in the tile
  const int tw = c - x0 < UT ? c - x0 : UT, th = c - y0 < UT ? c - y0 : UT;
  int clo, nc, rlo, nr;
  tile_extent(t.bounds_h, t.tx + x0, tw, t.w, clo, nc);
  tile_extent(t.bounds_v, t.ty + y0, th, t.h, rlo, nr);
  stage_table(t.bounds_h, t.coef_h, t.tx + x0, tw, clo, nc, fh, kh);
  stage_table(t.bounds_v, t.coef_v, t.ty + y0, th, rlo, nr, fv, kv);
  // the block's bytes, addressed relative to the window's origin (clamped into the window: the host has checked that the
  // window covers the tile's taps, so the clamp changes nothing for the tables of pil_bicubic_table)
  const float rcp_nc = 1.0f / (float)nc;
  const unsigned char* src = win + ((long)b * C + c0) * cw * cw;
  for (int ch = 0; ch < cn; ++ch)
    for (int i = threadIdx.x; i < nr * nc; i += 256) {
      const int r = small_div(i, rcp_nc), q = i - r * nc;
      const int wr = clampi(rlo - t.wy + r, 0, cw - 1), wq = clampi(clo - t.wx + q, 0, cw - 1);
      in_t[(ch * UH + r) * UH + q] = src[((long)ch * cw + wr) * cw + wq];
    }
  __syncthreads();
  pil_pass_h(in_t, tmp_t, fh, kh, cn, nr);
  __syncthreads();
  // vertical pass: a lane owns four neighbouring pixels of one output row, in every channel
  const int y = threadIdx.x / (UT / 4), q = threadIdx.x % (UT / 4);
  if (y >= th || 4 * q >= tw) return;
  const int lo = fv[y];
  int cf[KS];
  for (int k = 0; k < KS; ++k) cf[k] = kv[y][k];
  float px[UC][4];
  pil_pass_v(tmp_t, lo, cf, q, cn, px);
  const long plane = (long)c * c;
  const int ry = y0 + y, rx = x0 + 4 * q, fl = t.flips;
  auto put = [&](long first_plane, const float* v) {
    float* p = out + first_plane * plane;
    if (VEC && !(fl & 4)) {  // c % 4 == 0: the four pixels are inside the tile and stay one aligned word under a flip
      const int a = (fl & 2) ? c - 1 - ry : ry;
      if (fl & 1) *reinterpret_cast<f32x4*>(p + (long)a * c + (c - 4 - rx)) = (f32x4){v[3], v[2], v[1], v[0]};
      else *reinterpret_cast<f32x4*>(p + (long)a * c + rx) = (f32x4){v[0], v[1], v[2], v[3]};
    } else {
      for (int j = 0; j < 4; ++j)
        if (4 * q + j < tw) p[dt_store_index(ry, rx + j, c, fl)] = v[j];
    }
  };
  if (form == UPT_RGB) {
    for (int ch = 0; ch < cn; ++ch) put((long)b * C + c0 + ch, px[ch]);
    return;
  }
  float yy[4], cb[4], cr[4];
  for (int j = 0; j < 4; ++j) ycbcr_jpg(px[0][j], px[1][j], px[2][j], yy[j], cb[j], cr[j]);
  if (form == UPT_Y) {
    put(b, yy);
  } else {
    put((long)b * 3, yy);
    put((long)b * 3 + 1, cb);
    put((long)b * 3 + 2, cr);
  }
}

// first tap and one past the last tap of output o of pil_bicubic_table(in, out), in <= out: Resample.c's precompute_coeffs
// for a full-extent box with the bicubic filter's support of 2, in the same double arithmetic
static void upt_taps(int in, int out, int o, int* first, int* end) {
  const double scale = (double)in / out, center = (o + 0.5) * scale;
  int lo = (int)(center - 2.0 + 0.5), hi = (int)(center + 2.0 + 0.5);
  *first = lo < 0 ? 0 : lo;
  *end = hi > in ? in : hi;
}

extern "C" size_t sisr_upsample_tile_bytes(void) { return sizeof(UpsampleTile); }

extern "C" int sisr_upsample_tiles(const void* tiles_host, const void* tiles_dev, const unsigned char* windows, float* out, int ksize,
                                   int B, int C, int c, int cw, int form, void* stream) {
  if (!tiles_host || !tiles_dev || !windows || !out || ksize <= 0 || B <= 0 || C <= 0 || c <= 0 || cw <= 0 || form < UPT_RGB ||
      form > UPT_Y)
    return SISR_ERR_ARG;
  if (ksize != KS || (form != UPT_RGB && C != 3) || B > 65535) return SISR_ERR_UNSUPPORTED;
  const UpsampleTile* t = static_cast<const UpsampleTile*>(tiles_host);
  for (int b = 0; b < B; ++b) {
    const UpsampleTile& r = t[b];
    if (!r.bounds_h || !r.coef_h || !r.bounds_v || !r.coef_v || r.h <= 0 || r.w <= 0 || r.H <= 0 || r.W <= 0 || (r.flips & ~7))
      return SISR_ERR_ARG;
    if (r.H % r.h || r.W % r.w || r.H / r.h != r.W / r.w) return SISR_ERR_UNSUPPORTED;  // one integer scale for both sides
    if (r.ty < 0 || r.tx < 0 || (long)r.ty + c > r.H || (long)r.tx + c > r.W) return SISR_ERR_ARG;  // the tile leaves the image
    if (r.wy < 0 || r.wx < 0 || (long)r.wy + cw > r.h || (long)r.wx + cw > r.w) return SISR_ERR_ARG;  // the window leaves the LR image
    int first, end, unused;
    upt_taps(r.h, r.H, r.ty, &first, &unused);
    upt_taps(r.h, r.H, r.ty + c - 1, &unused, &end);
    if (first < r.wy || end > r.wy + cw) return SISR_ERR_ARG;  // the window misses a tap of the tile's rows ...
    upt_taps(r.w, r.W, r.tx, &first, &unused);
    upt_taps(r.w, r.W, r.tx + c - 1, &unused, &end);
    if (first < r.wx || end > r.wx + cw) return SISR_ERR_ARG;  // ... or columns
  }
  const long gz = (long)B * ((C + UC - 1) / UC);
  if (gz > 65535 || (c + UT - 1) / UT > 65535) return SISR_ERR_UNSUPPORTED;
  const dim3 grid((c + UT - 1) / UT, (c + UT - 1) / UT, (unsigned)gz);
  const UpsampleTile* td = static_cast<const UpsampleTile*>(tiles_dev);
  hipStream_t st = (hipStream_t)stream;
  if (c % 4 == 0 && sisr_aligned16(out))
    hipLaunchKernelGGL((upsample_tiles_kernel<true>), grid, dim3(256), 0, st, td, windows, out, C, c, cw, form);
  else
    hipLaunchKernelGGL((upsample_tiles_kernel<false>), grid, dim3(256), 0, st, td, windows, out, C, c, cw, form);
  return sisr_check_launch();
}

// ---------------------------------------------------------------- RGB -> BT.601 'jpg' YCbCr / Y of a planar fp32 batch
// rgb [B][3][n] -> out [B][3][n], or [B][1][n] with y_only: ycbcr_jpg's arithmetic, which is data.rgb_to_ycbcr(im_type='jpg')'s
__global__ __launch_bounds__(256) void rgb_to_ycbcr_kernel(const float* __restrict__ rgb, float* __restrict__ out, long n, int y_only) {
  const long b = blockIdx.y;
  const float* src = rgb + b * 3 * n;
  float* dst = out + b * (y_only ? 1 : 3) * n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    float y, cb, cr;
    ycbcr_jpg(src[i], src[n + i], src[2 * n + i], y, cb, cr);
    dst[i] = y;
    if (!y_only) {
      dst[n + i] = cb;
      dst[2 * n + i] = cr;
    }
  }
}

extern "C" int sisr_rgb_to_ycbcr(const float* rgb, float* out, int B, long n, int y_only, void* stream) {
  if (!rgb || !out || rgb == out || B <= 0 || n <= 0 || (y_only != 0 && y_only != 1)) return SISR_ERR_ARG;
  if (B > 65535) return SISR_ERR_UNSUPPORTED;
  const long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(rgb_to_ycbcr_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks), B), dim3(256), 0, (hipStream_t)stream, rgb,
                     out, n, y_only);
  return sisr_check_launch();
}
