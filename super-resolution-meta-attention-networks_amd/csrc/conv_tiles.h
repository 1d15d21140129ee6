// Device pieces shared by the 3x3 conv kernels (conv3x3_mfma.hip) and the weight-gradient kernels (wgrad3x3_mfma.hip):
// how a workgroup finds its tile(s) and how the persistent fp32 conv kernels stage a halo.  Every function is inlined into
// its caller; a change here changes every kernel named beside it, so compare their resource usage (profiles/README.md, round
// 12) and time them against the parent.
// The tile geometry below is the conv kernels' (the weight-gradient file has its own WT_H / WT_W and uses none of it).
#pragma once
#include "sisr_common.h"

#define TH 4
#define TW 32
#define HALO_H (TH + 2)
#define HALO_W (TW + 2)

struct ConvParams {
  const float* x;
  View xv;
  float* y;
  View yv;
  const float* res;
  const float* mask;
  const float* w;
  const float* bias;
  const float* in_scale;
  const float* in_shift;
  const float* out_scale;
  float* gap;
  const float* gate_add;  // GATE prologue: input = x * in_scale[b,c] + gate_add (x's layout), ...
  float* gate_out;        // ... whose in-image value is also written here once (by the tile that owns the pixel)
  const float* dot;       // DOT epilogue: gap partials hold sum(v * dot) instead of sum(v) (y's layout)
  float alpha;
  int bias_n, bias_q;
  int B, H, W, cin_chunks, cout_chunks, relu, tiles_w, tiles_h;
  int mask_leaky;  // relu: 0 none, 1 ReLU, 2 LeakyReLU(0.2); mask_leaky: the mask is LeakyReLU's derivative, not ReLU's
  // Gate HEADS (template HEAD of conv3x3_c64_v4_kernel, 64 -> 64 fp32): the CONSUMER of a channel-attention gate computes
  // it -- every workgroup, for its own sample, from the partial sums the previous launch wrote -- instead of a launch of its
  // own on the serial chain.  Same arithmetic and summation order as ca_gate_fwd / ca_gate_bwd (ca_gate.h).  fwd_gate: the
  // gate's operands and outputs (HEAD 1); bwd_gate: the per-sample part of its backward (HEAD 2; the parameter gradients
  // are summed by a launch of their own).
  struct {
    const float *w1, *b1, *w2, *b2, *mul;
    float *s, *hid, *ca, *g;
    float inv_hw;
    int R;
  } fwd_gate;
  struct {
    const float *w1, *w2, *hid, *ca, *mul;
    float *shift, *dmul, *dz2, *dz1;
    float inv_hw;
    int R;
  } bwd_gate;
  const float* head_part;  // [B][head_parts][64]
  int head_parts;
  // Generalised input geometry (template GEO of conv3x3_c64_v4_kernel; all zero elsewhere).  Output pixel (h, w) of the H x W
  // output reads the VIRTUAL input map of geo_h x geo_w pixels at (h + kh - 1 - geo_off, w + kw - 1 - geo_off):
  //   geo_reflect: coordinates outside the virtual map are reflected (-1 -> 1, n -> n - 2: ReflectionPad2d(1)) instead of
  //                reading zeros;  geo_up: the stored map is the virtual one subsampled by 2^geo_up (nearest upsampling read
  //                in place: stored pixel = virtual >> geo_up);  geo_off = 1 with geo_h = H - 2: the transposed ("full")
  //                form, an input-gradient map two pixels larger than the gradient it is computed from.
  int geo_reflect, geo_up, geo_off, geo_h, geo_w;
  int geo_sub;  // with geo_up = 1 and zero padding: the virtual map is the stored one ZERO-STUFFED (value at even coordinates only:
                // the gradient of a stride-2 conv seen at stride 1), not replicated
  int pred_epilogue;  // conv3x3_c64_w4_kernel: the predicated epilogue on every tile, full ones included (select 14; tests)
#ifdef SISR_DIAG
  unsigned* stamp;  // diagnostic library only: per wave {start lo, start hi, staging, K loop, epilogue, HW_ID, XCC_ID, 0}
#endif
};

// ------------------------------------------------------------------ which tile(s) a workgroup computes
// Per-tile launches (one workgroup per tile, gridDim.x = tiles): workgroups are dealt round-robin over the 8 XCDs
// (block b -> b % 8, a speed-only assumption): give each XCD a contiguous run of tiles so vertically adjacent tiles,
// which share two halo rows, meet in one L2.  Returns the tile id of this workgroup, a bijection of blockIdx.x.
__device__ __forceinline__ int sisr_xcd_tile_id() {
  const unsigned nb = gridDim.x, xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const unsigned qn = nb >> 3, rn = nb & 7;
  return (int)((xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + idx);
}

// Persistent launches (nwg workgroups walk `total` tiles): workgroup s lands on XCD s % 8; every XCD gets a contiguous eighth
// of the tiles and its nwg / 8 workgroups sweep it together, so that vertically adjacent tiles are read through the same L2
// at about the same time.  A workgroup count that is no multiple of 8 falls back to the strided walk (tile s, s + nwg, ...).
//   for (int tile = walk.begin; tile < walk.end; tile += walk.step)
struct TileWalk {
  int begin, end, step;
  __device__ __forceinline__ TileWalk(int total, int nwg) : begin(blockIdx.x), end(total), step(nwg) {
    if ((nwg & 7) == 0) {
      const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, per = (total + 7) >> 3;
      begin = xcd * per + idx;
      end = min(total, (xcd + 1) * per);
      step = nwg >> 3;
    }
  }
};

// Tile id -> sample, tile row / column and the tile's first output pixel, tiles ordered (b, th, tw) with tw fastest.  Two
// arithmetic forms of the same map, each kept where it grew: the conv kernels divide by tiles_w first, the weight-gradient
// and bf16-persistent kernels by tiles per image first.  Either costs two integer divisions; they stay side by side because
// swapping one for the other changes the instruction stream of every kernel that calls it and that has not been timed.
struct TileCoord {
  int b, th, tw, h0, w0;
};
template <int TILE_H, int TILE_W = TW>
__device__ __forceinline__ TileCoord sisr_tile_decode(int tile, int tiles_w, int tiles_h) {
  TileCoord t;
  t.tw = tile % tiles_w;
  const int t2 = tile / tiles_w;
  t.b = t2 / tiles_h;
  t.th = t2 - t.b * tiles_h;
  t.h0 = t.th * TILE_H;
  t.w0 = t.tw * TILE_W;
  return t;
}
template <int TILE_H, int TILE_W = TW>
__device__ __forceinline__ TileCoord sisr_tile_decode_by_image(int tile, int tiles_per_img, int tiles_w) {
  TileCoord t;
  t.b = tile / tiles_per_img;
  const int tr = tile - t.b * tiles_per_img;
  t.th = tr / tiles_w;
  t.tw = tr - t.th * tiles_w;
  t.h0 = t.th * TILE_H;
  t.w0 = t.tw * TILE_W;
  return t;
}

// ------------------------------------------------------------------ fp32 halo staging of the persistent conv kernels
// conv3x3_c64_p4_kernel and conv3x3_c64_w4_kernel request the 6 x 34 pixel halo of the NEXT tile before / inside the K loop
// of the current one (halo_issue: global -> registers) and write it to LDS after that loop (halo_commit).  Staging thread
// map: tid -> (16-B piece c4 = tid & 15 of a pixel, halo columns pcol + {0, 16, 32} with pcol = tid >> 4), rows 0..5: 18
// float4 per thread.  Every load is unconditional (clamped address); padding is zeroed when the halo is committed, by
// decisions of the tile (halo_commit).
typedef f32x4 halo_regs_t[HALO_H][3];
// What every staging call of a kernel shares, built once at its top and passed in: with p.H and threadIdx.x read inside the
// calls hipcc ordered the commit's masks differently (18 more s_and_b64 -> vcc -> v_cndmask chains per commit), which cost
// p4's mask + affine form 0.25 % (profiles/README.md, round 12).
struct HaloLane {
  int H, W, c4, pcol;
  // lane-constant: the thread's k = 0 piece is halo column 0, its k = 2 piece is halo column HALO_W - 1 -- the only two pieces
  // of a full-width tile that can lie left / right of the image (halo_commit)
  bool col_first, col_last;
  __device__ __forceinline__ HaloLane(const ConvParams& p, int tid)
      : H(p.H), W(p.W), c4(tid & 15), pcol(tid >> 4), col_first((tid >> 4) == 0), col_last((tid >> 4) == 1) {}
};

// rows [r0, r1) of the halo of tile t, input chunk `chunk` (CHUNKS: the maps have more than one; else chunk 0)
template <bool CHUNKS>
__device__ __forceinline__ void halo_issue(halo_regs_t& v, const ConvParams& p, const HaloLane& ln, const TileCoord& t, int chunk, int r0,
                                           int r1) {
  const int H = ln.H, W = ln.W, c4 = ln.c4, pcol = ln.pcol;
  const sisr_rsrc_t rx = sisr_rsrc(p.x + (long)t.b * p.xv.sB + (CHUNKS ? p.xv.chunk(chunk) : 0L));
#pragma unroll
  for (int r = r0; r < r1; ++r) {
    const unsigned ro = (unsigned)(min(max(t.h0 - 1 + r, 0), H - 1) * (int)p.xv.sH) * 4u;  // scalar, bytes
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < 2 || pcol < 2) {
        const unsigned go = (unsigned)(min(max(t.w0 - 1 + pcol + 16 * k, 0), W - 1) * (int)p.xv.sW + c4 * 4) * 4u;
        v[r][k] = sisr_buf_load4(rx, go, ro);
      }
  }
}

// The staged halo of tile tc -> LDS image `lds` (pixel stride 64 floats, 16-B piece k of halo column c at slot
// k ^ (c & 15)), through the prologue: AFFINE x * in_scale[b, c] + in_shift[b, c]; GATE x * in_scale[b, c] + gate_add, whose
// in-image value the tile that owns the pixel also writes to gate_out.  Zero padding stays zero (+0).  One input chunk.
// Padding is decided per tile, not per element (*Padding decided per tile*): what lies outside the image
// is a scalar fact of the tile for all but two lane groups.
//   halo row r            inside or outside for the whole workgroup: an outside row is written as +0 (over what the
//                         loads brought), under one scalar branch per tile and one per row inside it
//   full-width tile       (w0 + TW <= W) halo column 0 is outside only where w0 == 0, column 33 only where w0 + TW == W:
//                         one select on ln.col_first for the k = 0 piece / on ln.col_last for the k = 2 piece, under a
//                         scalar branch; the k = 1 piece is never outside
//   width-ragged tile     the per-element predicate, as before
// A piece inside the image is written as loaded (or as the prologue left it).  The decisions must reach the ISA as scalar
// branches: hipcc turns `if (uniform) t = keep_if(t, lane)` into a select that every tile pays, and sinks the two sides' LDS
// writes into one fed by selects, so each rarely taken side holds an empty `asm volatile` (neither speculated nor merged).
template <bool AFFINE, bool GATE>
__device__ __forceinline__ void halo_commit(const halo_regs_t& v, const ConvParams& p, const HaloLane& ln, const TileCoord& tc,
                                            float* lds) {
  const int H = ln.H, W = ln.W, c4 = ln.c4, pcol = ln.pcol;
  const int b = tc.b, h0 = tc.h0, w0 = tc.w0;
  f32x4 s4 = {1.f, 1.f, 1.f, 1.f}, t4 = {0.f, 0.f, 0.f, 0.f};
  if (AFFINE || GATE) s4 = *reinterpret_cast<const f32x4*>(p.in_scale + (long)b * 64 + c4 * 4);
  if (AFFINE && p.in_shift) t4 = *reinterpret_cast<const f32x4*>(p.in_shift + (long)b * 64 + c4 * 4);
  const sisr_rsrc_t ro_ = sisr_rsrc(GATE ? p.gate_out + (long)b * p.xv.sB : p.y);
  // GATE: the skip map is fetched here, not a tile ahead (two prefetched maps would not fit 256 registers beside the K
  // loop's); its round trip is covered by the other resident workgroup's K loop
  f32x4 u[GATE ? HALO_H : 1][3];
  if (GATE) {
    const sisr_rsrc_t ru = sisr_rsrc(p.gate_add + (long)b * p.xv.sB);
    // piece by piece, the order in which a full-width tile consumes them below
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < 2 || pcol < 2) {
        const unsigned go = (unsigned)(min(max(w0 - 1 + pcol + 16 * k, 0), W - 1) * (int)p.xv.sW + c4 * 4) * 4u;
#pragma unroll
        for (int r = 0; r < HALO_H; ++r)
          u[r][k] = sisr_buf_load4(ru, go, (unsigned)(min(max(h0 - 1 + r, 0), H - 1) * (int)p.xv.sH) * 4u);
      }
  }
  if (__builtin_expect(w0 + TW > W, 0)) {  // scalar: a width-ragged tile, per-element column predicates
#pragma unroll
    for (int r = 0; r < HALO_H; ++r) {
      const int gh = h0 - 1 + r;
      const bool rok = gh >= 0 && gh < H;               // scalar
      const bool rown = r >= 1 && r <= TH && gh < H;    // scalar: a row this tile owns
      const unsigned ro = (unsigned)(min(max(gh, 0), H - 1) * (int)p.xv.sH) * 4u;
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (k < 2 || pcol < 2) {
          const int col = pcol + 16 * k, gw = w0 - 1 + col;
          const bool cok = gw >= 0 && gw < W && col < HALO_W;
          f32x4 t = v[r][k];
          if (AFFINE) t = t * s4 + t4;
          if (GATE) {
            t = sisr_mul_add4(t, s4, u[r][k]);
            if (rown && cok && col >= 1 && col <= TW)
              sisr_buf_store4(t, ro_, (unsigned)(min(max(gw, 0), W - 1) * (int)p.xv.sW + c4 * 4) * 4u, ro);
          }
          t = sisr_keep_if(t, rok && cok);
          *reinterpret_cast<f32x4*>(lds + r * (HALO_W * 64) + col * 64 + ((c4 ^ (col & 15)) << 2)) = t;
        }
    }
    asm volatile("");
    return;
  }
  // A full-width tile, piece by piece (k outer): one scalar branch per edge around the six rows of its piece, not one per
  // row -- a branch beside the MFMA stream is not free either.  Rows outside the image are overwritten with +0 afterwards
  // (LDS writes of one wave land in program order); they are rare, one tile row in 32 at 128 rows.
  const bool left = w0 == 0, right = w0 + TW == W;  // scalar: halo column 0 / HALO_W - 1 is outside the image
#pragma unroll
  for (int k = 0; k < 3; ++k)
    if (k < 2 || pcol < 2) {
      const int col = pcol + 16 * k;
      float* const dst = lds + col * 64 + ((c4 ^ (col & 15)) << 2);
      f32x4 t[HALO_H];
#pragma unroll
      for (int r = 0; r < HALO_H; ++r) {
        t[r] = v[r][k];
        if (AFFINE) t[r] = t[r] * s4 + t4;
        if (GATE) {
          const int gh = h0 - 1 + r;
          t[r] = sisr_mul_add4(t[r], s4, u[r][k]);
          // the pixels this tile owns: rows 1 .. TH inside the image (scalar), halo columns 1 .. TW -- all of k = 1, k = 0
          // but column 0, of k = 2 column 32 only (lane-constant)
          if (r >= 1 && r <= TH && gh < H && (k == 1 || (k == 0 ? !ln.col_first : ln.col_first)))
            sisr_buf_store4(t[r], ro_, (unsigned)(min(max(w0 - 1 + col, 0), W - 1) * (int)p.xv.sW + c4 * 4) * 4u,
                            (unsigned)(min(max(gh, 0), H - 1) * (int)p.xv.sH) * 4u);
        }
      }
      // each side of an edge branch writes for itself: one write behind the branch would copy t on the side that leaves
      // it alone (a value that leaves a skipped branch in other registers than a taken one)
      if (__builtin_expect((k == 0 && left) || (k == 2 && right), 0)) {
#pragma unroll
        for (int r = 0; r < HALO_H; ++r)
          *reinterpret_cast<f32x4*>(dst + r * (HALO_W * 64)) = sisr_zero_if(t[r], k == 0 ? ln.col_first : ln.col_last);
        asm volatile("");
      } else {
#pragma unroll
        for (int r = 0; r < HALO_H; ++r) *reinterpret_cast<f32x4*>(dst + r * (HALO_W * 64)) = t[r];
      }
    }
  if (__builtin_expect(h0 == 0 || h0 + TH + 1 > H, 0)) {  // scalar: some halo row is outside the image
    // the zero is made here: a zero quad the compiler knows about is hoisted out of the tile loop and held in registers
    f32x4 z;
    asm volatile("v_mov_b32 %0, 0\n\tv_mov_b32 %1, 0\n\tv_mov_b32 %2, 0\n\tv_mov_b32 %3, 0" : "=v"(z.x), "=v"(z.y), "=v"(z.z), "=v"(z.w));
#pragma unroll
    for (int r = 0; r < HALO_H; ++r) {
      const int gh = h0 - 1 + r;
      if (gh < 0 || gh >= H) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
          if (k < 2 || pcol < 2) {
            const int col = pcol + 16 * k;
            *reinterpret_cast<f32x4*>(lds + r * (HALO_W * 64) + col * 64 + ((c4 ^ (col & 15)) << 2)) = z;
          }
      }
    }
    asm volatile("");
  }
}
