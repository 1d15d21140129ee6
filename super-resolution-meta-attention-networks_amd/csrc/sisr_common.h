// Shared device/host definitions for the gfx950 SISR kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// A 64-channel-chunked view of an activation in HBM.  Element (b, h, w, chunk q, c) lives at
//   p + b*sB + h*sH + w*sW + (q / cdiv)*chi + (q % cdiv)*clo + c          (all strides in floats)
// Plain NHWC with C = 64*k channels: sW = C, cdiv = huge, clo = 64.
// PixelShuffle(r) output seen as the conv's (B,H,W,64*r*r) result: physical tensor is
// [B][H*r][W*r][64]; sH = r*(W*r*64), sW = r*64, cdiv = r, chi = W*r*64, clo = 64, and chunk
// q = i*r + j carries original channels {c*r*r + q}.  The shuffle is therefore free: it is only an
// address map (ref: advanced/common.py:28-31 conv -> nn.PixelShuffle).
struct View {
  long sB, sH, sW;
  long chi, clo;
  int cdiv;
  __host__ __device__ long chunk(int q) const { return (long)(q / cdiv) * chi + (long)(q % cdiv) * clo; }
};
// The six int64 of a view argument of the C API (include/sisr_hip.h), in the order of the fields above.
static inline View view_from(const int64_t* v) { return View{v[0], v[1], v[2], v[3], v[4], (int)v[5]}; }

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// Zero a float4 with a lane mask by bitwise AND: exact zeros even if the (clamped-address) load
// returned Inf/NaN, and -- unlike `ok ? t : 0` -- hipcc cannot turn it back into a branch around the
// load (which would serialise the staging loads behind s_waitcnt vmcnt(0)).
__device__ __forceinline__ f32x4 sisr_keep_if(f32x4 t, bool ok) {
  const unsigned m = ok ? 0xffffffffu : 0u;
  u32x4 b = __builtin_bit_cast(u32x4, t);
  b &= (u32x4){m, m, m, m};
  return __builtin_bit_cast(f32x4, b);
}

// +0 where `zero` (a condition that is constant per lane, held as a lane mask: one select per component and no mask
// quad in registers), t elsewhere
__device__ __forceinline__ f32x4 sisr_zero_if(f32x4 t, bool zero) {
  return (f32x4){zero ? 0.f : t.x, zero ? 0.f : t.y, zero ? 0.f : t.z, zero ? 0.f : t.w};
}

// The gated skip t * g + x, with the product rounded BEFORE the sum (no fma contraction) -- the arithmetic of the
// reference's `x * y` followed by `res += x` on fp32 tensors.  It is formed by the stand-alone gate kernel and by the
// GATE prologues of the conv kernels, and all of them must agree to the bit, with each other and with the reference:
// the next block's ReLU mask is taken from this map, an element of it that differs by one ulp flips a mask bit now
// and then, and one flipped bit moves that block's weight gradient by ~3e-3 (found with a float64 run of the oracle).
__device__ __forceinline__ f32x4 sisr_mul_add4(f32x4 a, f32x4 b, f32x4 c) {
#pragma clang fp contract(off)
  const f32x4 p = a * b;
  return p + c;
}

// Two fp32 adds in one instruction (v_pk_add_f32 on a register pair; (lo, hi) = (.x, .y)).  Beside the fp32 MFMA every
// vector instruction costs its full issue time, a packed one about as much as a scalar one (tools/mfma_fill.py --winograd),
// and the Winograd transforms are nothing but adds.  hipcc keeps a packed add only where nobody reads the halves one by
// one -- MFMA operands are read exactly so -- and never a packed subtraction; hence inline assembly.  Each half is the
// IEEE add of the scalar form: a - b is a + (-b), and the source modifiers are exact.
// The compiler's hazard handling does not look inside: keep the result two instructions away from an MFMA that reads it
// as A / B, and a read of an MFMA result behind that MFMA's wait states (8-pass: 11, 16-pass: 19).
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 sisr_pk_add(f32x2 a, f32x2 b) {  // (a.x + b.x, a.y + b.y)
  f32x2 r;
  asm volatile("v_pk_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ f32x2 sisr_pk_sub(f32x2 a, f32x2 b) {  // (a.x - b.x, a.y - b.y)
  f32x2 r;
  asm volatile("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// ... and the f32x4 sum / difference as two of them, on (.xy, .zw)
__device__ __forceinline__ f32x4 sisr_pk4_add(f32x4 a, f32x4 b) {
  const f32x2 lo = sisr_pk_add(a.xy, b.xy), hi = sisr_pk_add(a.zw, b.zw);
  return (f32x4){lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ f32x4 sisr_pk4_sub(f32x4 a, f32x4 b) {
  const f32x2 lo = sisr_pk_sub(a.xy, b.xy), hi = sisr_pk_sub(a.zw, b.zw);
  return (f32x4){lo.x, lo.y, hi.x, hi.y};
}

// ... the product with one scalar s, passed as the pair (s, s), in place
__device__ __forceinline__ void sisr_pk4_scale(f32x4& a, f32x2 s) {
  f32x2 lo = a.xy, hi = a.zw;
  asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(lo) : "v"(s));
  asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(hi) : "v"(s));
  a = (f32x4){lo.x, lo.y, hi.x, hi.y};
}
// max(a, 0), one v_max_f32 per element.  fmaxf(a, 0.f) on a value that comes out of inline assembly costs two: hipcc
// cannot know that it is canonical and puts a self-max in front.  Same bits for every finite a (-0 gives +0, denormals
// stay: the kernels keep fp32 denormals) and for infinities; a quiet NaN gives 0 either way.
__device__ __forceinline__ f32x4 sisr_relu4(f32x4 a) {
  f32x4 r;
  asm volatile("v_max_f32 %0, 0, %1" : "=v"(r.x) : "v"(a.x));
  asm volatile("v_max_f32 %0, 0, %1" : "=v"(r.y) : "v"(a.y));
  asm volatile("v_max_f32 %0, 0, %1" : "=v"(r.z) : "v"(a.z));
  asm volatile("v_max_f32 %0, 0, %1" : "=v"(r.w) : "v"(a.w));
  return r;
}

// Buffer addressing.  Beside the fp32 MFMA stream a vector-memory instruction with a 64-bit per-lane address
// (`global_load_dwordx4 v, v[a:a+1], off`) costs its SIMD 30-40 cycles, and every VALU instruction that builds such an
// address ~4.5 more; the same access as SGPR resource + 32-bit lane offset + SGPR offset (`buffer_load_dwordx4 v, voff,
// s[rsrc], soff offen`) is free at the K loop's density, like SALU work (measured: tools/mfma_fill.py).  So the hot
// kernels address every operand as {wave-uniform base -> resource, lane-constant byte offset, scalar byte offset}.
// Raw resource (stride 0), bounds check off (num_records = 2^32 - 1): the offsets are in range by construction.
typedef __amdgpu_buffer_rsrc_t sisr_rsrc_t;
__device__ __forceinline__ sisr_rsrc_t sisr_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)0xffffffffu, 0x00020000);
}
__device__ __forceinline__ f32x4 sisr_buf_load4(sisr_rsrc_t r, unsigned voff_bytes, unsigned soff_bytes) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff_bytes, (int)soff_bytes, 0));
}
__device__ __forceinline__ float sisr_buf_load1(sisr_rsrc_t r, unsigned voff_bytes, unsigned soff_bytes) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff_bytes, (int)soff_bytes, 0));
}
__device__ __forceinline__ void sisr_buf_store4(f32x4 v, sisr_rsrc_t r, unsigned voff_bytes, unsigned soff_bytes) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, (int)voff_bytes, (int)soff_bytes, 0);
}
__device__ __forceinline__ void sisr_buf_store1(float v, sisr_rsrc_t r, unsigned voff_bytes, unsigned soff_bytes) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)voff_bytes, (int)soff_bytes, 0);
}
// (Write-through stores -- cache policy sc1, so that the bytes leave the XCD's L2 as they are written instead of in the
// write-back burst at the end of the kernel -- were measured for the conv output tiles and not kept: DESIGN.md.)

#define SISR_OK 0
#define SISR_ERR_ARG (-1)
#define SISR_ERR_ALIGN (-2)
#define SISR_ERR_LAUNCH (-3)
#define SISR_ERR_UNSUPPORTED (-4)

static inline int sisr_check_launch() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? SISR_OK : SISR_ERR_LAUNCH - (int)e * 16;
}
// Dynamic LDS above 64 KB needs an explicit opt-in on the kernel (gfx950 has 160 KB per CU).  Idempotent,
// so the unsynchronised once-flag is safe.
#define SISR_ALLOW_LDS(kernel, bytes)                                                                       \
  do {                                                                                                      \
    static bool done_ = false;                                                                              \
    if (!done_) {                                                                                           \
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),                                      \
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes));                  \
      done_ = true;                                                                                         \
    }                                                                                                       \
  } while (0)

static inline bool sisr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
