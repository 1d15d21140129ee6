// Geometric self-ensemble (the "+" rows of the EDSR / RCAN / HAN / SAN papers) around a network, DESIGN.md 6m:
//   sisr_dihedral_fan    one image batch -> its eight flips / transposes, as two batches the network runs as they are
//   sisr_dihedral_merge  the network's eight outputs, each mapped back, averaged
// Layout: contiguous NCHW fp32.  Batches are variant-major: image i of variant k is entry k * n + i.
//   upright (4n, c, h, w)   k = 0..3: the image, its columns reversed, its rows reversed, both reversed
//   turned  (4n, c, w, h)   k = 0..3: the same four operations applied to the transposed image
// Both kernels only move data (merge adds eight values), so the shape is that of a tiled transpose: a workgroup owns a
// 64 x 64 tile of one plane.  fan reads the tile once, by rows, into LDS and writes it eight times: four times by rows
// (forwards or backwards within a row, rows up or down) and four times by columns, which are the rows of the turned
// planes -- every global access walks a row of the plane it touches.  merge reads four tiles by rows into registers and
// four by rows of the turned planes through LDS, and writes one.  The LDS tile has a pitch of 65 words, so its rows and
// its columns both fall on distinct banks.
// Access width: a plane's rows are 16-byte aligned only where the row length is a multiple of 4 and the base pointer is
// aligned; the 16-byte forms are compiled for exactly that case (per side: VW for the planes with rows of length w, VH
// for those with rows of length h) and every other shape goes lane by lane, one word each.
#include "sisr_common.h"

#define DT 64        // tile edge
#define DP (DT + 1)  // LDS pitch in words: rows AND columns of a tile on distinct banks

// One lane of the 16-byte forms: a 64 x 64 tile is 64 rows x 16 quads, 1024 work items; item idx -> (row, quad).  Four
// neighbouring lanes take four neighbouring ROWS of one quad, so the 32 lanes that share an LDS cycle touch words
// (row 0..3) + 4 * (quad 0..7) [+ 65 * ...]: 32 distinct banks whether the tile is read by rows or by columns.  In memory a
// wave then covers four rows x 256 contiguous bytes.
__device__ __forceinline__ void quad_item(int idx, int& row, int& quad) {
  row = ((idx >> 6) << 2) | (idx & 3);
  quad = (idx >> 2) & 15;
}

// rows of a plane -> tile[r][c], r < nr, c < nc.  V: ld % 4 == 0, nc % 4 == 0, src 16-byte aligned.
template <bool V>
__device__ __forceinline__ void tile_load(float (*tile)[DP], const float* __restrict__ src, long ld, int nr, int nc) {
  if (V) {
    for (int idx = threadIdx.x; idx < DT * DT / 4; idx += 256) {
      int r, q;
      quad_item(idx, r, q);
      if (r < nr && 4 * q < nc) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + r * ld + 4 * q);
        tile[r][4 * q + 0] = v.x;
        tile[r][4 * q + 1] = v.y;
        tile[r][4 * q + 2] = v.z;
        tile[r][4 * q + 3] = v.w;
      }
    }
  } else {
    for (int idx = threadIdx.x; idx < DT * DT; idx += 256) {
      const int r = idx >> 6, c = idx & 63;
      if (r < nr && c < nc) tile[r][c] = src[r * ld + c];
    }
  }
}

// tile rows -> rows of a plane: dst[r * rstep + j] = tile[r][rev ? nc - 1 - j : j], r < nr, j < nc (rstep < 0: rows upwards)
template <bool V>
__device__ __forceinline__ void store_rows(float (*tile)[DP], float* __restrict__ dst, long rstep, int nr, int nc, bool rev) {
  if (V) {
    for (int idx = threadIdx.x; idx < DT * DT / 4; idx += 256) {
      int r, q;
      quad_item(idx, r, q);
      if (r < nr && 4 * q < nc) {
        const int c0 = rev ? nc - 1 - 4 * q : 4 * q, s = rev ? -1 : 1;
        const f32x4 v = {tile[r][c0], tile[r][c0 + s], tile[r][c0 + 2 * s], tile[r][c0 + 3 * s]};
        *reinterpret_cast<f32x4*>(dst + r * rstep + 4 * q) = v;
      }
    }
  } else {
    for (int idx = threadIdx.x; idx < DT * DT; idx += 256) {
      const int r = idx >> 6, j = idx & 63;
      if (r < nr && j < nc) dst[r * rstep + j] = tile[r][rev ? nc - 1 - j : j];
    }
  }
}

// tile columns -> rows of a turned plane: dst[a * rstep + j] = tile[rev ? nr - 1 - j : j][a], a < nc, j < nr
template <bool V>
__device__ __forceinline__ void store_cols(float (*tile)[DP], float* __restrict__ dst, long rstep, int nr, int nc, bool rev) {
  if (V) {
    for (int idx = threadIdx.x; idx < DT * DT / 4; idx += 256) {
      int a, q;
      quad_item(idx, a, q);
      if (a < nc && 4 * q < nr) {
        const int r0 = rev ? nr - 1 - 4 * q : 4 * q, s = rev ? -1 : 1;
        const f32x4 v = {tile[r0][a], tile[r0 + s][a], tile[r0 + 2 * s][a], tile[r0 + 3 * s][a]};
        *reinterpret_cast<f32x4*>(dst + a * rstep + 4 * q) = v;
      }
    }
  } else {
    for (int idx = threadIdx.x; idx < DT * DT; idx += 256) {
      const int a = idx >> 6, j = idx & 63;
      if (a < nc && j < nr) dst[a * rstep + j] = tile[rev ? nr - 1 - j : j][a];
    }
  }
}

// the workgroup's tile: plane p, rows r0 .. r0 + th - 1, columns c0 .. c0 + tw - 1 of an h x w plane
__device__ __forceinline__ void tile_of_block(int tiles_x, int tiles_y, int h, int w, long& p, int& r0, int& c0, int& th, int& tw) {
  const unsigned b = blockIdx.x;
  const unsigned tx = b % (unsigned)tiles_x, rest = b / (unsigned)tiles_x;
  const unsigned ty = rest % (unsigned)tiles_y;
  p = rest / (unsigned)tiles_y;
  r0 = (int)ty * DT;
  c0 = (int)tx * DT;
  th = h - r0 < DT ? h - r0 : DT;
  tw = w - c0 < DT ? w - c0 : DT;
}

// x: planes planes of h x w -> upright: 4 * planes planes of h x w, turned: 4 * planes planes of w x h.  grid: tiles * planes.
template <bool VW, bool VH>
__global__ __launch_bounds__(256) void dihedral_fan_kernel(const float* __restrict__ x, float* __restrict__ upright,
                                                           float* __restrict__ turned, long planes, int h, int w, int tiles_x,
                                                           int tiles_y) {
  __shared__ float tile[DT][DP];
  long p;
  int r0, c0, th, tw;
  tile_of_block(tiles_x, tiles_y, h, w, p, r0, c0, th, tw);
  const long hw = (long)h * w;
  tile_load<VW>(tile, x + p * hw + (long)r0 * w + c0, w, th, tw);
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const bool fc = k & 1, fr = k & 2;  // columns / rows of the variant reversed
    // upright: source row r0 + r -> row (fr ? h - 1 - r0 - r : r0 + r); the tile's columns land on c0 .., or on w - c0 - tw ..
    float* u = upright + (k * planes + p) * hw;
    store_rows<VW>(tile, u + (long)(fr ? h - 1 - r0 : r0) * w + (fc ? w - c0 - tw : c0), fr ? -(long)w : (long)w, th, tw, fc);
    // turned (w rows of h): source column c0 + a -> row (fr ? w - 1 - c0 - a : c0 + a); the tile's rows land on its columns
    float* t = turned + (k * planes + p) * hw;
    store_cols<VH>(tile, t + (long)(fr ? w - 1 - c0 : c0) * h + (fc ? h - r0 - th : r0), fr ? -(long)h : (long)h, th, tw, fc);
  }
}

// out (planes planes of H x W) = (((u0 + u1) + (u2 + u3)) + ((t0 + t1) + (t2 + t3))) * 0.125f with every variant mapped back:
// plain fp32 adds in exactly this order (nothing here can contract: there is no product before a sum), and the last
// factor is a power of two.  A lane owns 16 elements of the tile: 16 rows of one column, or (VW) 4 rows of one quad.
template <bool VW, bool VH>
__global__ __launch_bounds__(256) void dihedral_merge_kernel(const float* __restrict__ upright, const float* __restrict__ turned,
                                                             float* __restrict__ out, long planes, int H, int W, int tiles_x,
                                                             int tiles_y) {
  __shared__ float tile[2][DT][DP];
  long p;
  int r0, c0, th, tw;
  tile_of_block(tiles_x, tiles_y, H, W, p, r0, c0, th, tw);
  const long hw = (long)H * W;
  const int tid = threadIdx.x;
  float acc[16];
  // ---- the upright half, by rows, into registers
  const float* u0 = upright + p * hw;
  const float* u1 = upright + (planes + p) * hw;
  const float* u2 = upright + (2 * planes + p) * hw;
  const float* u3 = upright + (3 * planes + p) * hw;
  if (VW) {
    for (int i = 0; i < 4; ++i) {
      int r, q;
      quad_item(tid + 256 * i, r, q);
      if (r < th && 4 * q < tw) {
        const long row = (long)(r0 + r) * W, rrow = (long)(H - 1 - r0 - r) * W;
        const int col = c0 + 4 * q, rcol = W - c0 - 4 * q - 4;  // columns rcol .. rcol + 3 hold col + 3 .. col mirrored
        const f32x4 a = *reinterpret_cast<const f32x4*>(u0 + row + col);
        const f32x4 b = *reinterpret_cast<const f32x4*>(u1 + row + rcol);
        const f32x4 c = *reinterpret_cast<const f32x4*>(u2 + rrow + col);
        const f32x4 d = *reinterpret_cast<const f32x4*>(u3 + rrow + rcol);
        acc[4 * i + 0] = (a.x + b.w) + (c.x + d.w);
        acc[4 * i + 1] = (a.y + b.z) + (c.y + d.z);
        acc[4 * i + 2] = (a.z + b.y) + (c.z + d.y);
        acc[4 * i + 3] = (a.w + b.x) + (c.w + d.x);
      }
    }
  } else {
    for (int i = 0; i < 16; ++i) {
      const int r = (tid >> 6) + 4 * i, c = tid & 63;
      if (r < th && c < tw) {
        const long row = (long)(r0 + r) * W, rrow = (long)(H - 1 - r0 - r) * W;
        const int col = c0 + c, rcol = W - 1 - c0 - c;
        acc[i] = (u0[row + col] + u1[row + rcol]) + (u2[rrow + col] + u3[rrow + rcol]);
      }
    }
  }
  // ---- the turned half (planes of W rows x H columns), two variants at a time through LDS.  Variant k holds out[r][c] at
  // row (fr ? W - 1 - c : c), column (fc ? H - 1 - r : r): the tile's window starts at row a0, column b0 and is tw x th
  float half[16];
  for (int pair = 0; pair < 2; ++pair) {
    const bool fr = pair;  // k = 2 * pair + {0, 1}: rows reversed in the second pair, columns reversed in each pair's second
    const long a0 = fr ? W - c0 - tw : c0;
    if (pair) __syncthreads();  // the first pair's tiles have been read
    tile_load<VH>(tile[0], turned + (2 * pair * planes + p) * hw + a0 * H + r0, H, tw, th);
    tile_load<VH>(tile[1], turned + ((2 * pair + 1) * planes + p) * hw + a0 * H + (H - r0 - th), H, tw, th);
    __syncthreads();
    if (VW) {
      for (int i = 0; i < 4; ++i) {
        int r, q;
        quad_item(tid + 256 * i, r, q);
        if (r < th && 4 * q < tw) {
          for (int j = 0; j < 4; ++j) {
            const int c = 4 * q + j, a = fr ? tw - 1 - c : c;
            const float s = tile[0][a][r] + tile[1][a][th - 1 - r];
            if (pair) acc[4 * i + j] += half[4 * i + j] + s;
            else half[4 * i + j] = s;
          }
        }
      }
    } else {
      for (int i = 0; i < 16; ++i) {
        const int r = (tid >> 6) + 4 * i, c = tid & 63;
        if (r < th && c < tw) {
          const int a = fr ? tw - 1 - c : c;
          const float s = tile[0][a][r] + tile[1][a][th - 1 - r];
          if (pair) acc[i] += half[i] + s;
          else half[i] = s;
        }
      }
    }
  }
  // ---- the mean
  float* o = out + p * hw;
  if (VW) {
    for (int i = 0; i < 4; ++i) {
      int r, q;
      quad_item(tid + 256 * i, r, q);
      if (r < th && 4 * q < tw) {
        const f32x4 v = {acc[4 * i] * 0.125f, acc[4 * i + 1] * 0.125f, acc[4 * i + 2] * 0.125f, acc[4 * i + 3] * 0.125f};
        *reinterpret_cast<f32x4*>(o + (long)(r0 + r) * W + c0 + 4 * q) = v;
      }
    }
  } else {
    for (int i = 0; i < 16; ++i) {
      const int r = (tid >> 6) + 4 * i, c = tid & 63;
      if (r < th && c < tw) o[(long)(r0 + r) * W + c0 + c] = acc[i] * 0.125f;
    }
  }
}

// tiles of an h x w plane and the 1-D grid over `planes` of them; 0 where the grid would not fit
static inline long dihedral_grid(long planes, int h, int w, int& tiles_x, int& tiles_y) {
  tiles_x = (w + DT - 1) / DT;
  tiles_y = (h + DT - 1) / DT;
  const long blocks = planes * tiles_x * tiles_y;
  return blocks <= 0x7fffffffL ? blocks : 0;
}

#define DIHEDRAL_LAUNCH(kernel, vw, vh, ...)                                                                  \
  do {                                                                                                        \
    if (vw && vh) hipLaunchKernelGGL((kernel<true, true>), dim3((unsigned)blocks), dim3(256), 0, st, __VA_ARGS__);        \
    else if (vw) hipLaunchKernelGGL((kernel<true, false>), dim3((unsigned)blocks), dim3(256), 0, st, __VA_ARGS__);        \
    else if (vh) hipLaunchKernelGGL((kernel<false, true>), dim3((unsigned)blocks), dim3(256), 0, st, __VA_ARGS__);        \
    else hipLaunchKernelGGL((kernel<false, false>), dim3((unsigned)blocks), dim3(256), 0, st, __VA_ARGS__);               \
  } while (0)

extern "C" int sisr_dihedral_fan(const float* x, int n, int c, int h, int w, float* upright, float* turned, void* stream) {
  if (!x || !upright || !turned || n <= 0 || c <= 0 || h <= 0 || w <= 0) return SISR_ERR_ARG;
  const long planes = (long)n * c;
  int tiles_x, tiles_y;
  const long blocks = dihedral_grid(planes, h, w, tiles_x, tiles_y);
  if (!blocks) return SISR_ERR_UNSUPPORTED;
  const bool vw = w % 4 == 0 && sisr_aligned16(x) && sisr_aligned16(upright), vh = h % 4 == 0 && sisr_aligned16(turned);
  hipStream_t st = (hipStream_t)stream;
  DIHEDRAL_LAUNCH(dihedral_fan_kernel, vw, vh, x, upright, turned, planes, h, w, tiles_x, tiles_y);
  return sisr_check_launch();
}

extern "C" int sisr_dihedral_merge(const float* upright, const float* turned, int n, int c, int H, int W, float* out,
                                   void* stream) {
  if (!upright || !turned || !out || n <= 0 || c <= 0 || H <= 0 || W <= 0) return SISR_ERR_ARG;
  const long planes = (long)n * c;
  int tiles_x, tiles_y;
  const long blocks = dihedral_grid(planes, H, W, tiles_x, tiles_y);
  if (!blocks) return SISR_ERR_UNSUPPORTED;
  const bool vw = W % 4 == 0 && sisr_aligned16(upright) && sisr_aligned16(out), vh = H % 4 == 0 && sisr_aligned16(turned);
  hipStream_t st = (hipStream_t)stream;
  DIHEDRAL_LAUNCH(dihedral_merge_kernel, vw, vh, upright, turned, out, planes, H, W, tiles_x, tiles_y);
  return sisr_check_launch();
}
