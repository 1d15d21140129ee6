/* libsisr_hip.so -- C ABI of the MI355X (gfx950) SISR forward/backward kernels.
 *
 * Drop-in boundary.  The reference has no FFI: its hot path is the nn.Module tree built by the
 * model handlers (Code/SISR/models/advanced/architectures.py, attention_manipulators/architectures.py)
 * and executed by BaseModel.run_train / run_eval (Code/SISR/models/__init__.py:466-522).  Each entry
 * point below replaces the ATen kernels one of those modules dispatches to; the citation on each
 * function names the reference module.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - The caller owns every buffer (device pointers unless stated); nothing here allocates, frees,
 *    synchronises or throws.  Workspaces are sized by the *_workspace_bytes() queries.
 *  - All work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *  - Return 0 on success, negative on error: -1 bad argument, -2 misaligned pointer/stride
 *    (16-byte alignment is required for activations), -3-16*hipError launch failure, -4 unsupported
 *    shape (channel counts must be multiples of 64 on the matrix-core kernels).
 *  - Re-entrant and thread-safe: no global state (kernel-variant choices are per-call `select` arguments; the
 *    diagnostic entry points at the end exist only in libsisr_hip_diag.so, built with -DSISR_DIAG).
 *  - fp32 everywhere.  Activations are NHWC in 64-channel chunks described by a 6-element int64
 *    "view": {sB, sH, sW, chi, clo, cdiv}; element (b,h,w,chunk q,c) is at
 *        base + b*sB + h*sH + w*sW + (q / cdiv)*chi + (q % cdiv)*clo + c        (strides in floats)
 *    Plain NHWC with C channels: {H*W*C, W*C, C, 0, 64, 1<<30}.  The output of
 *    conv(64 -> 64 r^2) + PixelShuffle(r) is the view {rH*rW*64, r*rW*64, r*64, rW*64, 64, r} of the
 *    [B][rH][rW][64] tensor, with chunk q holding original channels {c*r*r + q}: the shuffle is an
 *    address map, never a copy (ref: advanced/common.py:28-31).
 *  - Conv weights stay in the reference's OIHW layout in the caller's parameters; kernels take
 *    either a packed copy (sisr_pack_conv3x3) or generic strides: element (o, i, tap) is read at
 *    w[o*so + i*si + (flip ? 8-tap : tap)], with channel maps o = n*perm_n + q*perm_q for in-chunk
 *    index n of chunk q.  Forward: so = Cin*9, si = 9, flip = 0.  Input gradient: roles swapped
 *    (so = 9, si = Cin*9) and flip = 1.
 */
#ifndef SISR_HIP_H
#define SISR_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- 3x3 convolution, Cin and Cout multiples of 64 (fp32 MFMA 32x32x2) ------------------------
 * ref: advanced/common.py:5-8 default_conv -> nn.Conv2d(k=3, pad=1) forward, and (with role-swapped,
 * flipped packed weights) its input gradient.  Fused:  y = mask( relu?( conv(x*in_scale+in_shift) + bias )
 * * alpha * out_scale ) + res, optional per-wave GAP partial sums of y.
 *   bias index    = n*bias_n + q*bias_q   (nullable)
 *   in_scale/shift: [B][cin]  (nullable; applied to in-image pixels only, zero padding stays zero)
 *   out_scale     : [B][cout] (nullable)          res, mask: same view as y (nullable)
 *   gap_partial   : [B][sisr_conv3x3_c64_gap_parts(H,W)][cout] (nullable)
 *   relu          : 0 none, 1 ReLU, 2 LeakyReLU(0.2); + 4: `mask` is LeakyReLU(0.2)'s derivative (slope 0.2 where the
 *                   masking map is <= 0) instead of ReLU's.  Codes 2 and 4 exist on the fp32 kernels only (SFTMD). */
int sisr_pack_conv3x3(const float* w, float* packed, int cout, int cin, int64_t so, int64_t si, int flip_taps,
                      int out_perm_n, int out_perm_q, int in_perm_n, int in_perm_q, void* stream);
/* forward and input-gradient packings of one weight in one launch (shuffle_r > 1: conv feeds PixelShuffle(r)) */
int sisr_pack_conv3x3_both(const float* w, float* packed_fwd, float* packed_dgrad, int cout, int cin, int shuffle_r,
                           void* stream);
/* every conv weight of a network in ONE launch (a training step repacks them all after the optimiser update).
 * jobs_device: device array of n_jobs records {const float* w; void* packed_fwd; void* packed_dgrad; int32 cout, cin,
 * shuffle_r, first_block} (sisr_pack_job_bytes() each; the caller builds it once per network); job j owns blocks
 * [first_block_j, first_block_j+1) of 256 packed elements each; total_blocks = their sum.  bf16 = 1: the bf16
 * packings of sisr_pack_conv3x3_bf16_both; 2: the three-plane packings of sisr_pack_conv3x3_x3_both. */
size_t sisr_pack_job_bytes(void);
int sisr_pack_conv3x3_many(const void* jobs_device, int n_jobs, int total_blocks, int bf16, void* stream);
int sisr_conv3x3_c64_gap_parts(int H, int W);
int sisr_conv3x3_c64(const float* x, const int64_t* xview, const float* wpacked, const float* bias, int bias_n,
                     int bias_q, float* y, const int64_t* yview, const float* res, const float* mask,
                     const float* in_scale, const float* in_shift, const float* out_scale, float alpha, int relu,
                     float* gap_partial, const float* gate_add, float* gate_out, const float* dot, int B, int H,
                     int W, int cin, int cout, const void* ca_tail, int select, void* stream);
/* ca_tail (nullable HOST pointer to a sisr_ca_tail, copied into the launch; 64 -> 64 fp32, select 0 only): a gate HEAD.  The
 * launch that CONSUMES a channel-attention gate computes it first -- every workgroup for its own sample, from the partial
 * sums a previous launch wrote (head_part [B][head_parts][64]) -- instead of a gate launch of its own between the two convs.
 * Same arithmetic and summation order as sisr_ca_gate_fwd / sisr_ca_gate_bwd.  backward = 0 on a gate_add / gate_out launch
 * (in_scale must be g_out: it is filled here, with s_out / hid_out / ca_out); backward = 1 on an in_scale + in_shift + mask
 * launch (in_shift must be `shift`: filled here, with dmul and the workspace, B rows of 80 floats: per sample dz2 [64],
 * then dz1 [hidden <= 16]; parameter gradients: sisr_ca_gate_bwd_params_batch).  head must be nonzero (a record with
 * head = 0 is refused with SISR_ERR_UNSUPPORTED); counter, s and dw1 .. db2 are unused.  The record keeps its layout
 * (sisr_ca_tail_bytes). */
typedef struct {
  int backward, hidden;
  float inv_hw;
  const float *w1, *b1, *w2, *b2, *mul; /* gate parameters (b1, b2 unused backward), optional second factor [B][64] */
  const float *s, *hid, *ca;            /* backward: what the forward kept (s unused) */
  float *s_out, *hid_out, *ca_out, *g_out;       /* forward outputs */
  float *shift, *dmul, *dw1, *db1, *dw2, *db2;   /* backward outputs (dw1 .. db2 unused) */
  float* workspace;
  unsigned* counter;
  const float* head_part;
  int head_parts, head;
} sisr_ca_tail;
size_t sisr_ca_tail_bytes(void);
/* select: 0 (= 4) issue-lean kernel -- per-tile (2-row tiles) below 1024 4 x 32 tiles per launch, persistent from there up
 * (SISR_CONV_PERSISTENT=0: never) -- with the general kernel as fallback; 6 / 7 the same with the per-tile / persistent
 * form forced (bit-identical results; A/B measurements and tests); 2 general kernel only.  1, 3 and 5 are refused.
 * 8 / 9 / 10: the caller asserts structural zeros in the packed weight (SFTMD's merged convs) and the kernel skips them:
 *   8  64 -> 128 block-diagonal (output chunk q contracts input channels 32q .. 32q+31 only), plain epilogue;
 *   9  128 -> 64 whose input channels >= 80 are zero (second chunk: first 16 channels only), LeakyReLU epilogue;
 *  10  128 -> 64, the transpose of 8 (input chunk c feeds output channels 32c .. 32c+31 only), LeakyReLU' mask, no bias.
 * 11 / 12: the Winograd F(2x2,3x3) weights U = G g G^T follow the whole direct packing (wpacked + cin * cout * 9 floats, written
 *   by sisr_pack_conv3x3_many for jobs with r | 0x100); 11 behaves as 0 but runs the Winograd form of the persistent kernel
 *   from more than 8 x 128^2 output pixels per launch on (SISR_CONV_WINOGRAD=0: never), 12 as 7 with the Winograd form forced.
 *   Shapes: 64 -> 64 in every form the persistent kernel serves, and 64 -> 64 r^2 / 64 r^2 -> 64, r >= 2 (the upsampler's
 *   conv stored through a shuffle view and its input gradient read through one: xview and yview may differ) in the plain form: bias or none, alpha, ReLU, and none of res / mask / in_scale / in_shift /
 *   out_scale / gap_partial / gate / dot / head / LeakyReLU; any other combination at those shapes runs the direct form.
 *   Other channel counts: SISR_ERR_ARG.
 *   14: as 12, and the Winograd kernel runs its predicated epilogue (per-element bounds tests, clamped operand addresses) on
 *   every tile.  Under 11 / 12 a tile that lies wholly inside the image (h0 + 4 <= H and w0 + 32 <= W) takes a straight-line
 *   epilogue instead, with the same values in the same order: 14 exists so that tests can compare the two bit for bit.
 *   U layout: one block of 65536 floats per pair of 64-channel chunks, block (q, c) at (q * cin / 64 + c) * 65536 -- the
 *   (output chunk, input chunk) order and the channel maps of the direct packing -- each [xi 16][G 4][q4 4][co 64][e 4] for
 *   transform point xi = 4 xr + xc and input channel 16 G + 4 q4 + e of the chunk. */
/* gate_add / gate_out / dot (all nullable; 64 -> 64, x and y in one layout) fuse the gated-residual chain of
 * RCAB / QRCAB stacks (ref: advanced/architectures.py:68-71, :107-110) into the neighbouring convs:
 *   gate_add + gate_out : the conv reads  x * in_scale[b,c] + gate_add  (the previous block's `res * y + x`) and
 *                         writes that map to gate_out once -- no separate gate pass in forward;
 *   dot                 : gap_partial receives sum(v * dot) instead of sum(v): the gate gradient sum(dY * t) of
 *                         the block below, taken while its dY is being produced -- no separate reduction pass. */

/* ---- 3x3 convolution weight + bias gradient (fp32 MFMA), deterministic two-stage reduction ------
 * ref: autograd's convolution_backward for default_conv (loss.backward(), SISR/models/__init__.py:483).
 *   dW = alpha * sum X (x) dY',  db = alpha * sum dY',  dY' = dY*dy_scale[b][co] + dy_shift[b][co] */
size_t sisr_wgrad3x3_c64_workspace_bytes(int B, int H, int W, int cin, int cout);
int sisr_wgrad3x3_c64(const float* x, const int64_t* xview, const float* dy, const int64_t* dyview,
                      const float* dy_scale, const float* dy_shift, float alpha, float* dw, int64_t so, int64_t si,
                      int flip_taps, int out_perm_n, int out_perm_q, int in_perm_n, int in_perm_q, float* dbias,
                      int bias_n, int bias_q, float* workspace, size_t workspace_bytes, int B, int H, int W, int cin,
                      int cout, unsigned long long active_units, void* stream);
/* active_units: 0 = the whole gradient.  Otherwise bit ((cin_chunk * cout_chunks + cout_chunk) * 4 + ci_half * 2 + co_half)
 * selects the 32 x 32-channel blocks (x 9 taps) to compute; the others are neither computed nor written (a caller whose
 * weight is structurally sparse -- SFTMD's merged convs -- never reads them).  At most 64 blocks; every bias half needs
 * one active block. */
/* Several 64 -> 64 weight gradients of ONE geometry in one launch (plain OIHW dw [64][64][3][3], db [64], alpha 1): at a few
 * tiles per GPU a single gradient's launch is mostly ramp, slab epilogue and drain; batched, every workgroup walks a long
 * run of tiles of its own job.  jobs: HOST array of njobs <= sisr_wgrad3x3_c64_batch_max() records
 * { x, dy, dy_scale (nullable), dy_shift (nullable), dw, dbias (nullable) } of device pointers, all with the views given. */
typedef struct {
  const float* x;
  const float* dy;
  const float* dy_scale;
  const float* dy_shift;
  float* dw;
  float* dbias;
} sisr_wgrad_job;
size_t sisr_wgrad_job_bytes(void);
int sisr_wgrad3x3_c64_batch_max(void);
size_t sisr_wgrad3x3_c64_batch_workspace_bytes(int njobs, int B, int H, int W);
int sisr_wgrad3x3_c64_batch(const void* jobs, int njobs, const int64_t* xview, const int64_t* dyview, float* workspace,
                            size_t workspace_bytes, int B, int H, int W, void* stream);

/* ---- RGB-side 3x3 convolutions (fp32 VALU, HBM-bound) ------------------------------------------
 * ref: head = default_conv(3, n_feats), tail[-1] = default_conv(n_feats, 3)
 * (advanced/architectures.py:141,150-152).  x/y of the 3-channel side are planar NCHW. */
int sisr_conv3x3_cin3(const float* x, const float* w, int64_t so, int64_t si, int flip_taps, const float* bias,
                      float* y, const int64_t* yview, int B, int H, int W, int cout, void* stream);
int sisr_conv3x3_cout3(const float* x, const int64_t* xview, const float* w, int64_t so, int64_t si, int flip_taps,
                       const float* bias, float* y, int B, int H, int W, int cin, void* stream);
size_t sisr_corr3x3_c3_workspace_bytes(int B, int H, int W, int channels);
int sisr_corr3x3_c3(const float* P, const float* Q, const int64_t* qview, float alpha, float* dw, int64_t so,
                    int64_t si, int flip_taps, int a_is_out, float* dbias, float* workspace, size_t workspace_bytes,
                    int B, int H, int W, int channels, void* stream);

/* ---- channel attention gate (64 channels) --------------------------------------------------------
 * ref: advanced/architectures.py:13-32 CALayer; attention_manipulators/architectures.py:125 QCALayer 'standard'.
 * fwd: s = inv_hw*sum(partials); hid = relu(W1 s + b1); ca = sigmoid(W2 hid + b2); g = ca * (mul or 1)
 * bwd: from partial sums of dg = sum_hw dOut*t: shift = dL/ds * inv_hw, dmul = dg*ca, dW1 db1 dW2 db2 */
int sisr_ca_gate_fwd(const float* gap_partial, int parts, int B, float inv_hw, const float* w1, const float* b1,
                     const float* w2, const float* b2, int channels, int hidden, const float* mul, float* s,
                     float* hid, float* ca, float* g, void* stream);
size_t sisr_ca_gate_bwd_workspace_bytes(int B);
int sisr_ca_gate_bwd(const float* dg_partial, int parts, int B, float inv_hw, const float* w1, const float* w2,
                     int channels, int hidden, const float* s, const float* hid, const float* ca, const float* mul,
                     float* shift, float* dmul, float* dw1, float* db1, float* dw2, float* db2, float* workspace,
                     unsigned* counter, void* stream);
/* workspace: B rows of 80 floats (sisr_ca_gate_bwd_workspace_bytes), per sample dz2 [64] then dz1 [hidden].
 * dw1 = db1 = dw2 = db2 = NULL (counter may be NULL too): only the per-sample part (shift, dmul, dz2 / dz1 into the
 * workspace); the parameter gradients of up to sisr_ca_gate_bwd_params_batch_max() such calls are then taken in ONE launch.
 * jobs: HOST array of { that call's workspace, hid, s, dw1, db1, dw2, db2 } (sisr_ca_param_job_bytes() each). */
int sisr_ca_gate_bwd_params_batch_max(void);
size_t sisr_ca_param_job_bytes(void);
int sisr_ca_gate_bwd_params_batch(const void* jobs, int njobs, int B, int hidden, void* stream);
/* counter: one zero-initialised device word owned by the caller and reused across calls on a stream (the kernel
 * returns it to zero): the sample blocks count themselves on it and the last one sums the parameter gradients,
 * so the whole gate backward is ONE launch on the block's serial backward chain. */

/* ---- meta-attention gate --------------------------------------------------------------------------
 * ref: attention_manipulators/q_layer.py:4-43 ParaCALayer: m = sigmoid(V2 act(V1 md + c1) + c2) */
int sisr_meta_gate_fwd(const float* md, int B, int M, int hidden, int channels, const float* v1, const float* c1,
                       const float* v2, const float* c2, int relu, float* hid, float* m, void* stream);
size_t sisr_meta_gate_bwd_workspace_bytes(int B, int hidden, int channels);
int sisr_meta_gate_bwd(const float* dm, const float* m, const float* hid, const float* md, int B, int M, int hidden,
                       int channels, const float* v1, const float* v2, int relu, float* dv1, float* dc1, float* dv2,
                       float* dc2, float* dmd, float* workspace, void* stream);
/* All L meta-attention layers of a network at once (the gates depend on the metadata and each layer's own weights
 * only -- ref: attention_manipulators/architectures.py:172-180 applies q_node to the same `metadata` in every
 * QRCAB): *_table are device arrays of L device pointers to the layers' parameters; hid [L][B][hidden], m and dm
 * [L][B][channels]; gradients come back as [L][hidden*M], [L][hidden], [L][channels*hidden], [L][channels].
 * No metadata gradient. */
int sisr_meta_gate_many_fwd(const float* md, int B, int M, int hidden, int channels, int layers,
                            const float* const* v1_table, const float* const* c1_table, const float* const* v2_table,
                            const float* const* c2_table, int relu, float* hid, float* m, void* stream);
size_t sisr_meta_gate_many_bwd_workspace_bytes(int B, int hidden, int channels, int layers);
int sisr_meta_gate_many_bwd(const float* dm, const float* m, const float* hid, const float* md, int B, int M, int hidden,
                            int channels, int layers, const float* const* v1_table, const float* const* v2_table,
                            int relu, float* dv1, float* dc1, float* dv2, float* dc2, float* workspace, void* stream);
/* the same, with each layer's four gradients written to the addresses in four device tables of `layers` pointers (e.g.
 * slices of an optimiser's flat gradient arena) instead of into [layers][...] arrays */
int sisr_meta_gate_many_bwd_scatter(const float* dm, const float* m, const float* hid, const float* md, int B, int M,
                                    int hidden, int channels, int layers, const float* const* v1_table,
                                    const float* const* v2_table, int relu, float* const* dv1_table, float* const* dc1_table,
                                    float* const* dv2_table, float* const* dc2_table, float* workspace, void* stream);

/* ---- generic gate MLP: the metadata-mixing QCALayer styles ---------------------------------------------
 * ref: attention_manipulators/architectures.py:105-127 (QCALayer.forward after avg_pool: 'modulate', 'max_concat',
 * 'softmax', 'mini_concat', 'extended_attention').  Layer k: z = W_k in_k + b_k with in_k = cat(v_k, metadata if cat[k]),
 * ReLU'd first if relu_in[k]; v_{k+1} = act[k](z), act 0 none / 1 ReLU / 2 sigmoid; final_mode 0 none / 1 softmax over
 * channels / 2 multiply by the metadata (M == C); then an optional per-(b,c) factor `mul` (the meta-attention gate).
 * desc: HOST pointer, copied into the launch; w/b device pointers (Conv2d 1x1 weights, [nout][nin + cat*M]).
 * acts [B][nin[0] + sum nout], yfin [B][C] are kept for the backward; workspace [B][sum nout]; dw/db HOST arrays of L
 * device pointers; dmd, dmul nullable. */
#define SISR_GATE_MLP_MAX_LAYERS 4
typedef struct {
  const float* w[SISR_GATE_MLP_MAX_LAYERS];
  const float* b[SISR_GATE_MLP_MAX_LAYERS];
  int nin[SISR_GATE_MLP_MAX_LAYERS], nout[SISR_GATE_MLP_MAX_LAYERS], cat[SISR_GATE_MLP_MAX_LAYERS],
      relu_in[SISR_GATE_MLP_MAX_LAYERS], act[SISR_GATE_MLP_MAX_LAYERS];
  int L, M, C, final_mode;
} sisr_gate_mlp;
size_t sisr_gate_mlp_desc_bytes(void);
int sisr_gate_mlp_fwd(const float* pool, const float* md, const float* mul, int B, const void* desc, float* acts,
                      float* yfin, float* y, void* stream);
int sisr_gate_mlp_bwd(const float* dy, const float* md, const float* mul, int B, const void* desc, const float* acts,
                      const float* yfin, float* workspace, float* dpool, float* dmd, float* dmul, float* const* dw,
                      float* const* db, void* stream);

/* ---- gated residual: y = t*g[b,c] + shift[b,c] + x  (g, shift, x nullable)
 * ref: the `x * y` / `res += x` tails of CALayer, RCAB, QRCAB, ParamResBlock; with shift it is also the
 * CALayer input gradient dy*g + dL/ds/HW.  gate_dg_partial: per-slice sums of dy*t (t NULL: of dy = GAP). */
int sisr_gate_residual_fwd(const float* t, const float* g, const float* shift, const float* x, float* y, int B,
                           long hw, int channels, void* stream);
int sisr_gate_dg_parts(long hw);
int sisr_gate_dg_partial(const float* dy, const float* t, float* part, int B, long hw, int channels, void* stream);
int sisr_sum_partials(const float* part, int parts, int B, int channels, float scale, float* out, void* stream);

/* ---- pixel attention, 64 channels, hidden 8 (ref: attention_manipulators/architectures.py:13-26 PALayer):
 * y = x * sigmoid(w2 . relu(W1 x + b1) + b2) per pixel; x, y contiguous [npix][64]. */
int sisr_pa_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y, long npix,
                int channels, int hidden, void* stream);
size_t sisr_pa_bwd_workspace_bytes(long npix);
int sisr_pa_bwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2, const float* dy,
                float* dx, float* dw1, float* db1, float* dw2, float* db2, float* workspace, long npix, int channels,
                int hidden, void* stream);

/* ---- HAN attention modules ---------------------------------------------------------------------
 * ref: advanced/HAN_blocks.py:7-37 LAM_Module: x [B][N][chw] (N layer maps, any common layout);
 *      attn = softmax_j(max_j E_ij - E_ij), E = X X^T;  y = gamma*attn X + x.   N in {2..6, 8, 11}.
 * ref: advanced/HAN_blocks.py:40-76 CSAM_Module: x NHWC 64 channels; w27 = Conv3d weight [dc][dh][dw];
 *      y = x*(1 + gamma*sigmoid(conv3d(x) + bias)).  gamma / bias are DEVICE pointers (1-element parameters). */
size_t sisr_lam_workspace_bytes(int B, int N, long chw);
int sisr_lam_fwd(const float* x, const float* gamma, float* y, float* attn, float* workspace, int B, int N, long chw,
                 void* stream);
int sisr_lam_bwd(const float* x, const float* attn, const float* gamma, const float* dy, float* dx, float* dgamma,
                 float* workspace, int B, int N, long chw, void* stream);
int sisr_csam_fwd(const float* x, const float* w27, const float* bias, const float* gamma, float* y, int B, int H,
                  int W, int C, void* stream);
size_t sisr_csam_bwd_workspace_bytes(int B, int H, int W, int C);
int sisr_csam_bwd(const float* x, const float* w27, const float* bias, const float* gamma, const float* dy, float* dx,
                  float* dw27, float* dbias, float* dgamma, float* workspace, int B, int H, int W, int C, void* stream);

/* ---- bf16 matrix-core variants of the 64-channel-chunk conv and its weight gradient ----------------
 * Same arguments, views, prologue / epilogue options and results layout as sisr_conv3x3_c64 / sisr_wgrad3x3_c64
 * (ref: advanced/common.py:5-8 default_conv and its autograd backward).  Feature maps, biases and gradients stay
 * fp32 in HBM; the two MFMA operands are rounded to bf16 (round-to-nearest-even) on their way into LDS --
 * activations after the optional affine prologue, weights once at pack time -- products are exact and
 * accumulation is fp32 (the semantics of a bf16 autocast convolution).  The bias gradient is summed from the
 * unrounded fp32 values.  pack_conv3x3_bf16_both writes cout*cin*9 bf16 elements per packing. */
int sisr_pack_conv3x3_bf16_both(const float* w, void* packed_fwd, void* packed_dgrad, int cout, int cin, int shuffle_r,
                                void* stream);
int sisr_conv3x3_c64_bf16(const float* x, const int64_t* xview, const void* wpacked_bf16, const float* bias, int bias_n,
                          int bias_q, float* y, const int64_t* yview, const float* res, const float* mask,
                          const float* in_scale, const float* in_shift, const float* out_scale, float alpha, int relu,
                          float* gap_partial, const float* gate_add, float* gate_out, const float* dot,
                          int B, int H, int W, int cin, int cout, int select, void* stream);
/* select: 0 persistent double-buffered tile loop where it applies (64 -> 64, >= 1024 tiles), 1 per-tile kernel */
size_t sisr_wgrad3x3_c64_bf16_workspace_bytes(int B, int H, int W, int cin, int cout);
int sisr_wgrad3x3_c64_bf16(const float* x, const int64_t* xview, const float* dy, const int64_t* dyview,
                           const float* dy_scale, const float* dy_shift, float alpha, float* dw, int64_t so, int64_t si,
                           int flip_taps, int out_perm_n, int out_perm_q, int in_perm_n, int in_perm_q, float* dbias,
                           int bias_n, int bias_q, float* workspace, size_t workspace_bytes, int B, int H, int W,
                           int cin, int cout, void* stream);

/* ---- bf16 STORAGE of the maps a residual group keeps (opt-in on top of the bf16 operand mode; BASELINE config 5) -------
 * ref: the maps are the reference's fp32 activations of advanced/architectures.py:48-71, :94-110 (RCAB / ResidualGroup);
 * the reference has no reduced-precision mode -- parity is pinned to the oracle's restatement of exactly this rounding.
 * A bf16 map has the View of its fp32 twin (strides in ELEMENTS) and 2-byte elements; it is passed as float* (16-byte
 * aligned).  storage bits of the conv: 1 = x / gate_add / gate_out, 2 = y, 4 = mask / dot, 8 = res are bf16 maps.  64 -> 64
 * only, always the persistent tile loop; only the combinations the fused group node launches exist (others: unsupported).
 * Weight gradient: storage 1 = x is a bf16 map, 3 = x and dY are.  sisr_f32_to_bf16 rounds a map to nearest even. */
int sisr_conv3x3_c64_bf16s(const float* x, const int64_t* xview, const void* wpacked_bf16, const float* bias, int bias_n,
                           int bias_q, float* y, const int64_t* yview, const float* res, const float* mask,
                           const float* in_scale, const float* in_shift, float alpha, int relu, float* gap_partial,
                           const float* gate_add, float* gate_out, const float* dot, int B, int H, int W, int storage,
                           void* stream);
int sisr_wgrad3x3_c64_bf16s(const float* x, const int64_t* xview, const float* dy, const int64_t* dyview,
                            const float* dy_scale, const float* dy_shift, float alpha, float* dw, int64_t so, int64_t si,
                            int flip_taps, int out_perm_n, int out_perm_q, int in_perm_n, int in_perm_q, float* dbias,
                            int bias_n, int bias_q, float* workspace, size_t workspace_bytes, int B, int H, int W,
                            int cin, int cout, int storage, void* stream);
int sisr_f32_to_bf16(const float* src, void* dst, long n, void* stream); /* n a multiple of 8 */

/* ---- SAN attention modules ---------------------------------------------------------------------
 * Second-order channel attention, ref: advanced/SAN_blocks.py:244-302 SOCA + advanced/mpncov.py:12-112.
 *   covpool_fwd : cov[b] = (1/M) sum_p (x_p - mean[b]) x_p^T      x [B][M][64] channels-last, mean [B][64]
 *                 (= Covpool.forward's X I^ X^T without the M x M matrix)
 *   sqrtm_fwd   : Newton-Schulz square root (trace pre-normalised, `iters` iterations, post-compensated) and the
 *                 column means SOCA feeds to its gate: pooled [B][64]; `saved` keeps the iterates for backward
 *   sqrtm_bwd   : Sqrtm.backward from dL/dpooled; returns G + G^T (the form Covpool.backward consumes)
 *   soca_bwd_apply : dx = dy * gate[b,c] + (1/M) (G + G^T)(x - mean)   -- `y_cov * x` plus Covpool.backward
 * Non-local attention, ref: advanced/SAN_blocks.py:126-141 (_embedded_gaussian: f = theta^T phi, softmax over
 * keys, y = f g): theta [nb][nq][8], phi / g [nb][nk][8]; streaming softmax, lse [nb][nq] kept for backward,
 * dsum [nb][nq] is scratch. */
size_t sisr_covpool_workspace_bytes(int B, long hw);
int sisr_covpool_fwd(const float* x, const float* mean, float* cov, float* workspace, int B, long hw, int channels,
                     void* stream);
size_t sisr_sqrtm_saved_bytes(int B, int dim, int iters);
int sisr_sqrtm_fwd(const float* cov, float* saved, float* pooled, int B, int dim, int iters, void* stream);
int sisr_sqrtm_bwd(const float* cov, const float* saved, const float* dpooled, float* dcov_sym, int B, int dim,
                   int iters, void* stream);
int sisr_soca_bwd_apply(const float* dy, const float* gate, const float* x, const float* mean, const float* dcov_sym,
                        float* dx, int B, long hw, int channels, void* stream);
int sisr_nl_attn_fwd(const float* theta, const float* phi, const float* g, float* y, float* lse, int nb, int nq, int nk,
                     int dim, void* stream);
int sisr_nl_attn_bwd(const float* theta, const float* phi, const float* g, const float* y, const float* lse,
                     const float* dy, float* dtheta, float* dphi, float* dg, float* dsum, int nb, int nq, int nk,
                     int dim, void* stream);

/* ---- loss and optimiser ---------------------------------------------------------------------------
 * ref: SISR/models/__init__.py:268 nn.L1Loss, :299-308 optim.Adam, :481-489 standard_update */
size_t sisr_l1_loss_workspace_bytes(void);
int sisr_l1_loss(const float* a, const float* b, long n, float* loss, float* grad, float* workspace, void* stream);
/* The same loss and gradient with the sums kept in double and divided by n: the value is the mean rounded to fp32 once
 * (sisr_l1_loss multiplies an fp32 sum by a rounded 1 / n).  workspace: 16-byte aligned (SISR_ERR_ALIGN otherwise). */
size_t sisr_l1_loss_mean_workspace_bytes(void);
int sisr_l1_loss_mean(const float* a, const float* b, long n, float* loss, float* grad, double* workspace,
                      void* stream);
/* torch.optim.Adam's update over one flat range (parameters, gradients, exp_avg, exp_avg_sq laid out alike):
 * one_minus_beta*, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t) computed by the host in double;
 * gradients are read as g * grad_scale.  p, g, m and v must be 16-byte aligned (SISR_ERR_ALIGN, -2, otherwise: the
 * body moves float4; a tail of n % 4 floats is updated one by one); a null pointer or n <= 0 is SISR_ERR_ARG. */
int sisr_adam_flat(float* p, const float* g, float* m, float* v, long n, float beta2, float one_minus_beta1,
                   float one_minus_beta2, float eps, float step_size, float bc2_sqrt, float grad_scale, void* stream);

/* ---- the step's optional parts: gradient-norm clipping, decoupled weight decay, weight EMA (csrc/update.hip) ----
 * Global L2 norm of the gradient over several flat fp32 ranges, two stages, no atomics.  Every product g * g (exact in
 * double) and every sum is in double.  sisr_sumsq_partial cuts a range of n floats over sisr_sumsq_workspace_bytes(n) / 8
 * workgroups (at most 1024; a grid-stride loop above 1 048 576 floats) and writes that many double partial sums at `part`;
 * the caller places the partials of its ranges one behind the other.  g must be 16-byte aligned (the body loads float4, a
 * tail of n % 4 floats one by one), part 8-byte aligned.  sisr_clip_coef is one workgroup: it adds the nparts partials in
 * a fixed order and writes  *norm64 = sqrt(sum),  *norm32 = (float)*norm64,
 * *coef = (float)min(1, max_norm / (*norm64 + 1e-6))  -- torch.nn.utils.clip_grad_norm_(error_if_nonfinite=False): the
 * coefficient is computed in double and rounded once; a NaN norm gives a NaN coefficient.  The cut of a range and the order
 * of every sum depend on the range lengths alone: two calls on the same data give the same bits.  One launch per range
 * plus one, no host synchronisation.  A null pointer, n <= 0, nparts <= 0 or max_norm not > 0: SISR_ERR_ARG. */
size_t sisr_sumsq_workspace_bytes(long n);
int sisr_sumsq_partial(const float* g, long n, double* part, void* stream);
int sisr_clip_coef(const double* part, long nparts, double max_norm, double* norm64, float* norm32, float* coef,
                   void* stream);

/* sisr_adam_flat with three additions, in this order per element (no fused multiply-adds):
 *   gg = g * grad_scale, and if grad_scale_dev != NULL  gg = gg * *grad_scale_dev  (a device word the kernel reads, e.g.
 *        sisr_clip_coef's coefficient; the stored gradient is not modified);
 *   p = p * decay_factor  (decoupled / AdamW weight decay: the host passes 1 - lr * weight_decay, computed in double);
 *   exp_avg, exp_avg_sq and p as sisr_adam_flat updates them, on gg;
 *   if ema != NULL  ema = ema + (p_new - ema) * one_minus_decay  (a fifth array laid out like the others).
 * With grad_scale_dev == NULL, decay_factor == 1 and ema == NULL the results are bitwise sisr_adam_flat's.  Alignment
 * and refusals as there (ema 16-byte aligned, grad_scale_dev 4-byte aligned).
 * sisr_ema_flat performs the ema line alone over a range (parameters the step skips); p is only read. */
int sisr_update_flat(float* p, const float* g, float* m, float* v, float* ema, long n, float beta2, float one_minus_beta1,
                     float one_minus_beta2, float eps, float step_size, float bc2_sqrt, float grad_scale,
                     const float* grad_scale_dev, float decay_factor, float one_minus_decay, void* stream);
int sisr_ema_flat(const float* p, float* ema, long n, float one_minus_decay, void* stream);

/* ---- progress words for hipGraph replays (data-parallel reducer; ref: SISR/models/__init__.py:344-347 DataParallel) ----
 * sisr_host_flags_alloc: n zeroed 32-bit words of pinned, host-coherent, device-visible memory (nullptr on failure; the
 * one allocation the library makes on the caller's behalf, returned to sisr_host_flags_free).  sisr_signal_host enqueues
 * a one-thread kernel that adds 1 to *flag once every earlier kernel of the stream has completed; under stream capture it
 * becomes a graph node, so a replay reports how far it has got without host round trips inside the graph. */
void* sisr_host_flags_alloc(int n);
void sisr_host_flags_free(void* flags);
int sisr_signal_host(void* flag, void* stream);
/* device-side wait: work enqueued on `stream` after this call starts once *flag >= value (hipStreamWaitValue32) */
int sisr_stream_wait_flag(void* flag, unsigned value, void* stream);
/* the same as a one-lane polling kernel on `stream` (bounded: after about a minute it stores 1 to *timed_out, nullable) */
int sisr_stream_spin_flag(void* flag, unsigned value, void* timed_out, void* stream);

/* ---- training tiles cut on the device (the step in front of the path) ---------------
 * ref: sr_tools/image_manipulation.py:233-257 random_flip_rotate + random_matched_crop, in the order
 * data_handler.py:500-513 applies them.  src: B device pointers to planar [C][H_b][W_b] fp32 images; params: B records
 * of 8 ints {H, W, top, left, hflip, vflip, transpose, 0} (top / left in the augmented image); dst [B][C][crop][crop]. */
int sisr_crop_augment(const float* const* src, const int* params, float* dst, int B, int C, int crop, void* stream);

/* ---- diagnostics (not on the product path): sustained fp32-MFMA rate and in-kernel clock ---------- */
#ifdef SISR_DIAG /* libsisr_hip_diag.so only (csrc/build.sh diag): not part of the product library */
int sisr_diag_mfma_peak(int blocks, int iters, float* out, unsigned long long* clk, void* stream);
/* resident workgroups per CU the runtime computes for the plain bf16x3 (which = 0) / fp32 (1) conv kernel */
int sisr_diag_conv_occupancy(int which);
/* every later conv3x3_c64_v4_kernel launch writes, per wave, 8 uint32 {start (shader clock), start (100 MHz clock), staging,
 * K loop, epilogue (shader cycles), HW_ID, XCC_ID, lifetime (100 MHz ticks)} into buf (device, workgroups*4*8 words); nullptr switches it off
 * (tools/conv_timeline.py) */
void sisr_diag_conv_stamp(void* buf);
/* the cost of `count` (0 with kind 1, else 8 / 16 / 32) filler instructions of one kind per eight v_mfma_f32_32x32x2_f32
 * (kinds: csrc/diag.hip); clk = {shader cycles, 100 MHz ticks} of block 0's loop (tools/mfma_fill.py) */
int sisr_diag_mfma_fill(int blocks, int iters, int kind, int count, float* out, const float* src, unsigned long long* clk,
                        void* stream);
#endif

/* ---- fp32 through the bf16 matrix cores ("bf16x3", opt-in; the reference has no such mode) -----------------------
 * Same contract as sisr_conv3x3_c64_bf16, but every fp32 operand is split exactly into three bf16 numbers (hi + mid +
 * lo) and the six products of weight >= 2^-16 run on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (hi*hi and the
 * five corrections in separate accumulators): fp32-class error (the dropped products are <= 2^-24 relative each) at
 * 6/16 of the fp32 MFMA's cycles.  Packed weights: three bf16 planes, cout*cin*9 elements apart. */
int sisr_pack_conv3x3_x3_both(const float* w, void* packed_fwd, void* packed_dgrad, int cout, int cin, int shuffle_r,
                              void* stream);
int sisr_conv3x3_c64_x3(const float* x, const int64_t* xview, const void* wpacked_x3, const float* bias, int bias_n,
                        int bias_q, float* y, const int64_t* yview, const float* res, const float* mask,
                        const float* in_scale, const float* in_shift, const float* out_scale, float alpha, int relu,
                        float* gap_partial, const float* gate_add, float* gate_out, const float* dot, int B, int H,
                        int W, int cin, int cout, int select /* must be 0 */, void* stream);

/* weight / bias gradient in the same arithmetic (contract of sisr_wgrad3x3_c64) */
size_t sisr_wgrad3x3_c64_x3_workspace_bytes(int B, int H, int W, int cin, int cout);
int sisr_wgrad3x3_c64_x3(const float* x, const int64_t* xview, const float* dy, const int64_t* dyview,
                         const float* dy_scale, const float* dy_shift, float alpha, float* dw, int64_t so, int64_t si,
                         int flip_taps, int out_perm_n, int out_perm_q, int in_perm_n, int in_perm_q, float* dbias,
                         int bias_n, int bias_q, float* workspace, size_t workspace_bytes, int B, int H, int W, int cin,
                         int cout, void* stream);

/* ---- channel padding and RGB pixel-shuffle (SRMD: conv(3+M -> nc) ... conv(nc -> 3 r^2) + PixelShuffle(r))
 * ref: advanced/architectures.py:380-425, advanced/SRMD_blocks.py:33-126.  The MFMA convs work on 64-channel chunks:
 * the (3+M)-channel NCHW input becomes a zero-padded NHWC map, head / tail weights zero-padded OIHW copies (crop != 0:
 * the inverse, for their gradients), and the tail's NHWC result is shuffled into the NCHW image (adjoint != 0: the
 * gradient map, padded channels zero). */
int sisr_nchw_to_nhwc_pad(const float* x, float* y, int B, int C, int H, int W, int C_padded, void* stream);
int sisr_pad_oihw(const float* src, float* dst, int cout, int cin, int cout_padded, int cin_padded, int taps, int crop,
                  void* stream);
int sisr_shuffle_rgb(const float* src, float* dst, int B, int C, int r, int H, int W, int C_padded, int adjoint,
                     void* stream);
/* HAN's map stack (ref: advanced/architectures.py:357-362 torch.cat of the 11 intermediate maps): map [B][hw][64] -> slot k
 * of stack [B][N][hw][64] (unstack != 0: the reverse, for the stack's gradient). */
int sisr_stack_maps(const float* src, float* dst, int B, long hw, int N, int k, int unstack, void* stream);
/* nn.PixelShuffle(r) on a channels-last map (ref: advanced/common.py:20-45; C = 64 upsamplers fuse it into the conv's store):
 * src [B][H][W][C r^2] -> dst [B][rH][rW][C]; adjoint != 0: dst [B][H][W][C r^2] <- src [B][rH][rW][C]. */
int sisr_pixel_shuffle_cl(const float* src, float* dst, int B, int H, int W, int C, int r, int adjoint, void* stream);

/* ---- on-the-fly LR synthesis (online_degradations) -----------------------------------------------------------
 * ref: sr_tools/gaussian_utils.py:346-368 BatchBlur (reflection pad + per-channel l x l correlation), :52-53
 * ToPILImage quantisation `mul(255).byte()`, sr_tools/image_manipulation.py:32-53 downsample (PIL BICUBIC resize).
 * sisr_blur_quant: planar [C][H][W] fp32, one [l][l] kernel (l <= 21) -> uint8 (and / or the unquantised fp32 blur).
 * sisr_pil_resample: ONE pass of libImaging/Resample.c's 8-bit resampler over a planar uint8 image (vertical = 0:
 * taps along x; 1: along y, optionally written as fp32 / 255 = ToTensor): out = clip8((2^21 + sum in*coef) >> 22);
 * bounds [out][2] (first tap, taps) and coef [out][ksize] int32 are device copies of the host tables. */
int sisr_blur_quant(const float* x, const float* kernel, unsigned char* y_u8, float* y_f32, int C, int H, int W, int l,
                    void* stream);
/* y = byte(255 * clamp(noise * sigma + blur, 0, 1)) over n values: b_GaussianNoising on the blurred image followed by
 * ToPILImage's quantisation (ref: sr_tools/gaussian_utils.py:306-312, 409-411); `noise` is the host-drawn N(0,1) field */
int sisr_noise_quant(const float* blur, const float* noise, float sigma, unsigned char* y_u8, long n, void* stream);
int sisr_pil_resample(const unsigned char* in, void* out, const int* bounds, const int* coef, int ksize, int C, int Hin,
                      int Win, int Hout, int Wout, int vertical, int to_float, void* stream);

/* ---- bicubic pre-up-sampling of an LR batch for the evaluator (csrc/interp.hip) ------------------------------------
 * ref: SISR/evaluation/standard_eval.py:146-164 (_low_res_prep: ToPILImage -> resize(x scale, BICUBIC) -> ToTensor;
 * _high_res_prep: BT.601 'jpg' YCbCr).  One launch for the batch, no workspace: lr [B][C][h][w] fp32 is quantised as
 * ToPILImage does (byte(v * 255), truncating), run through both passes of libImaging/Resample.c's 8-bit resampler (as
 * sisr_pil_resample; the horizontal rows of a 32 x 32 output tile stay in LDS) and written as rgb = byte / 255 and / or
 * ycbcr = metrics.rgb_to_ycbcr_jpg(rgb) with that function's fp32 roundings (no fma), [B][C][H][W] fp32 each; either output
 * may be null, not both.  H = s h and W = s w for one integer s >= 1; bounds_* / coef_* are device copies of the host
 * tables for (w -> W) and (h -> H), whose ksize is 5 at every such scale.  SISR_ERR_ARG: null pointers, non-positive sizes;
 * SISR_ERR_UNSUPPORTED: other size ratios, ycbcr with C != 3, ksize != 5, more than 65535 tile rows or B * ceil(C / 3) > 65535. */
int sisr_pil_upsample(const float* lr, float* rgb, float* ycbcr, const int* bounds_h, const int* coef_h, const int* bounds_v,
                      const int* coef_v, int ksize, int B, int C, int h, int w, int H, int W, void* stream);

/* ---- SPARNet / QSPARNet pieces (csrc/sparnet.hip) --------------------------------------------------------------
 * ref: SPARNet/blocks.py:69-103 ConvLayer ([nearest x2] -> ReflectionPad2d(1) -> Conv2d(3x3, stride 1 | 2) -> [BatchNorm2d]
 * -> [LeakyReLU(0.2)]), :106-174 ResidualBlock, :177-243 HourGlassBlock.  Maps are NHWC with C a multiple of 64 (channels
 * >= C_real zero).  The convs themselves are sisr_conv3x3_c64 / sisr_wgrad3x3_c64 on the padded geometry.
 * sisr_pad_reflect_up: adjoint == 0: x (B,H,W,C) -> y (B, up H + 2, up W + 2, C) = ReflectionPad2d(1)(nearest_up(x)), up 1 | 2;
 *   adjoint != 0: x is the gradient of that padded map, y (B,H,W,C) its fold back (sums in index order).
 * sisr_crop_stride: embed == 0: src (B,Hf,Wf,C) -> dst (B,Ho,Wo,C), dst[h][w] = src[1 + s h][1 + s w], Ho = (Hf-3)/s + 1 --
 *   the interior of the "same" conv over the padded map = the reference's unpadded (strided) conv; embed != 0: the adjoint.
 * sisr_bn_act_fwd: y = act(BatchNorm2d(x)), act = LeakyReLU(slope) (slope 1: none).  training != 0: batch statistics
 *   (biased variance, two passes), mean_out / invstd_out [C] saved for the backward, running_mean / running_var (nullable)
 *   updated with `momentum` and the unbiased variance as torch does; training == 0: the running statistics.
 * sisr_bn_act_bwd: dx, dgamma [C_real], dbeta [C_real] from x, dy (gradient AFTER the activation), mean, invstd.
 *   workspace: sisr_bn_workspace_bytes(npix, C) for both.
 * sisr_spar_combine_fwd: y = identity (nullable) + x * a, a = sigmoid(logits[p][0]) (logits NHWC with C_logits channels),
 *   att[p] = a.  _bwd: dx = dy * a; dlogits[p][0] = (sum_c dy x) a (1 - a), the other channels of dlogits zero. */
/* The stride-1 ConvLayer conv WITHOUT the gathers (round 4): reflection and nearest upsampling as address arithmetic in the
 * MFMA kernels' staging (csrc/conv3x3_mfma.hip template GEO, csrc/wgrad3x3_mfma.hip GEO bodies).
 * sisr_conv3x3_c64_geo  mode 1: y (B,H,W,cout) = Conv2d(3x3, no padding)(ReflectionPad2d(1)(nearest_up^up(x))) + bias,
 *     x (B, H >> up, W >> up, cin), up 0 | 1 (a SHIFT: 1 = nearest x2);
 *   mode 2: y (B,H,W,cout) = zero-padded 3x3 conv of x (B,H-2,W-2,cin) placed at (1,1) of an H x W zero map -- with the
 *     input-gradient packing of the weight, the gradient of mode 1's padded map; sisr_pad_reflect_up(adjoint) folds it back.
 *   wpacked as for sisr_conv3x3_c64; gap_partial (nullable): per-strip channel sums of y in sisr_conv3x3_c64's layout;
 *   kreal > 0 (cin == 64 only): the caller's promise that input channels >= kreal are zero (<= 8 / <= 32 run 1 / 4 of the 8
 *   channel octets per tap).  Results equal the gather -> sisr_conv3x3_c64 -> gather composition bit for bit.
 * sisr_wgrad3x3_c64_geo: dw (co_real, ci_real, 3, 3) and db (co_real, nullable) of mode 1 from x (B, H >> up, W >> up, cin) and
 *   dy (B,H,W,cout); workspace: sisr_wgrad3x3_c64_workspace_bytes(B, H, W, cin, cout); active_units as in sisr_wgrad3x3_c64
 *   (blocks that hold only channel padding may be masked; bias halves >= co_real need no unit). */
int sisr_conv3x3_c64_geo(const float* x, const int64_t* xview, const float* wpacked, const float* bias, float* y,
                         const int64_t* yview, float* gap_partial, int B, int H, int W, int cin, int cout, int mode, int up,
                         int kreal, void* stream);
int sisr_wgrad3x3_c64_geo(const float* x, const int64_t* xview, const float* dy, const int64_t* dyview, float* dw, int co_real,
                          int ci_real, float* dbias, float* workspace, size_t workspace_bytes, int B, int H, int W, int cin,
                          int cout, int up, unsigned long long active_units, void* stream);
/* Any number of such weight gradients of DIFFERENT geometries, eight per launch (plain NHWC maps: x (B, H >> up, W >> up, cin),
 * dy (B, H, W, cout)); jobs: HOST array of njobs records, read before the call returns.  Per job the result is that of
 * sisr_wgrad3x3_c64_geo up to the summation order of its K-split. */
typedef struct sisr_wgrad_geo_job {
  const float* x;
  const float* dy;
  float* dw;
  float* dbias; /* nullable */
  int B, H, W, cin, cout, up, co_real, ci_real;
  unsigned long long active_units;
} sisr_wgrad_geo_job;
size_t sisr_wgrad_geo_job_bytes(void);
size_t sisr_wgrad3x3_c64_geo_batch_workspace_bytes(const void* jobs, int njobs);
int sisr_wgrad3x3_c64_geo_batch(const void* jobs, int njobs, float* workspace, size_t workspace_bytes, void* stream);
/* Non-default ConvLayer options (ref: SPARNet/blocks.py:17-33 norm_type 'in' | 'gn' | 'pixel', :50-64 relu_type 'prelu' | 'selu',
 * :147-151 att_name 'spar3d').  Maps NHWC, C a multiple of 4, channels >= C_real zero padding (written as zero).
 * sisr_group_norm_fwd / _bwd: statistics per (sample, group of cg consecutive real channels) over hw pixels (InstanceNorm2d: cg = 1;
 *   GroupNorm(32, C): cg = C / 32), biased variance, two passes; mean / invstd: [B][C_real / cg]; backward writes dx and the
 *   per-sample sums dgamma_b, dbeta_b [B][C_real] (add them over the batch with sisr_sum_partials).
 * sisr_pixel_norm: backward == 0: out = x / max(||x||_2 over the pixel's channels, 1e-12) (F.normalize(p = 2, dim = 1));
 *   else out = dx from x and dy.  C / 4 a power of two <= 64.
 * sisr_act: mode 0 PReLU (slope [C_real]), 1 SELU; backward == 0: out = act(x); else out = dx and, for PReLU, dyx = dy min(x, 0)
 *   (its per-channel sum is the slope's gradient).
 * sisr_spar3d: backward == 0: out0 = identity (nullable) + x sigmoid(logits); else (third argument = dy) out0 = dx = dy a,
 *   out1 = dlogits = dy x a (1 - a); n elements (a multiple of 4). */
int sisr_group_norm_fwd(const float* x, float* y, const float* gamma, const float* beta, float* mean_out, float* invstd_out, int B,
                        long hw, int C, int C_real, int cg, float eps, void* stream);
int sisr_group_norm_bwd(const float* x, const float* dy, const float* gamma, const float* mean, const float* invstd, float* dx,
                        float* dgamma_b, float* dbeta_b, int B, long hw, int C, int C_real, int cg, void* stream);
int sisr_pixel_norm(const float* x, const float* dy, float* out, long npix, int C, int backward, void* stream);
int sisr_act(const float* x, const float* dy, const float* slope, float* out, float* dyx, long npix, int C, int C_real, int mode,
             int backward, void* stream);
int sisr_spar3d(const float* x, const float* logits, const float* identity_or_dy, float* out0, float* out1, long n, int backward,
                void* stream);
/* sisr_nearest_up: nn.Upsample(scale_factor = up, 'nearest') on an NHWC map, up 1 .. 4 (ref: advanced/SRMD_blocks.py:58-63, the
 * 'upconv' tail of SRMD); adjoint != 0: the gradient summed back over the up x up replicas. */
int sisr_nearest_up(const float* src, float* dst, int B, int H, int W, int C, int up, int adjoint, void* stream);
size_t sisr_bn_workspace_bytes(long npix, int C);
int sisr_pad_reflect_up(const float* x, float* y, int B, int H, int W, int C, int up, int adjoint, void* stream);
int sisr_crop_stride(const float* src, float* dst, int B, int Hf, int Wf, int C, int stride, int embed, void* stream);
int sisr_bn_act_fwd(const float* x, float* y, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, float* mean_out, float* invstd_out, long npix, int C, int C_real, int training,
                    float momentum, float eps, float slope, float* workspace, size_t workspace_bytes, void* stream);
int sisr_bn_act_bwd(const float* x, const float* dy, const float* gamma, const float* beta, const float* mean,
                    const float* invstd, float* dx, float* dgamma, float* dbeta, long npix, int C, int C_real, float slope,
                    float* workspace, size_t workspace_bytes, void* stream);
int sisr_spar_combine_fwd(const float* x, const float* logits, const float* identity, float* y, float* att, long npix, int C,
                          int C_logits, void* stream);
int sisr_spar_combine_bwd(const float* dy, const float* x, const float* att, float* dx, float* dlogits, long npix, int C,
                          int C_logits, void* stream);

/* ---- SFTMD pieces (csrc/sft.hip) ------------------------------------------------------------------------------
 * ref: SFTMD_variants/architectures.py:25-56 StandardSft (x * sigmoid(mul) + add), :110-176 SFTMD (LeakyReLU(0.2),
 * 9x9 64 -> 3 output conv, clamp).  The network's 3x3 convs run on sisr_conv3x3_c64 with `relu` = 2 (LeakyReLU(0.2)
 * epilogue) or `relu` | 4 (the `mask` operand carries LeakyReLU's derivative: slope 0.2 where the map is <= 0).
 * sisr_sft_compose: split == 0: WA [64][128][9] = rows (mul_conv1 | add_conv1) over input channels 0 .. 63 + M (rest
 *   zero), bA [64], WB [128][64][9] = block-diagonal (mul_conv2 on inputs 0..31, add_conv2 on inputs 32..63), bB [128]
 *   from the layer's eight parameters; split != 0: the reverse copy (gradients).  M = metadata maps (<= 64).
 * sisr_sft_combine_fwd: out = [relu](x * sigmoid(y2[:, :64]) + y2[:, 64:]); x / out with pixel strides (floats), y2
 *   [npix][128]; md (nullable) [npix][64] is copied into out's second 64-channel chunk.  _bwd: dx [npix][64], dy2.
 * sisr_map64: 64-channel maps with pixel strides: op 0 copy, 1 a + b, 2 LeakyReLU(a), 3 b * LeakyReLU'(a), 4 a * b,
 *   5 ReLU(a), 6 b * ReLU'(a), 7 a * (b's channel 0, broadcast).  out may be a itself (same stride): op 2 is used so.
 *   Strides are multiples of 4 floats and >= 64, except b's under op 7, which reads one float per pixel.
 * sisr_conv9_*: 9x9 conv 64 -> 3 (OIHW weight), x NHWC [B][H][W][64], y NCHW; dgrad optionally masked by LeakyReLU'
 *   of `leaky_mask` (the activated map that fed the conv); wgrad: ordered two-stage sums (dw OIHW, db).
 * sisr_clamp01: backward == 0: out = clamp(a, 0, 1); else out = grad * [0 <= a <= 1]. */
int sisr_sft_compose(float* mul_w1, float* mul_b1, float* add_w1, float* add_b1, float* mul_w2, float* mul_b2, float* add_w2,
                     float* add_b2, float* WA, float* bA, float* WB, float* bB, int M, int split, void* stream);
/* all SFT layers of a network in one launch: table = n records of 12 device pointers (the arguments of sisr_sft_compose in
 * order) + int M + int split, sisr_sft_compose_record_bytes() each, in device memory.  The record's split field is
 * ignored: this entry point always composes (parameters -> merged tensors). */
size_t sisr_sft_compose_record_bytes(void);
int sisr_sft_compose_many(const void* table, int n, void* stream);
int sisr_sft_combine_fwd(const float* x, long x_stride, const float* y2, const float* md, float* out, long out_stride,
                         long npix, int relu, void* stream);
int sisr_sft_combine_bwd(const float* dout, long dout_stride, const float* x, long x_stride, const float* y2, float* dx,
                         float* dy2, long npix, int relu, void* stream);
int sisr_map64(const float* a, long a_stride, const float* b, long b_stride, float* out, long out_stride, long npix, int op,
               void* stream);
int sisr_conv9_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, void* stream);
int sisr_conv9_dgrad(const float* dy, const float* w, const float* leaky_mask, float* dx, int B, int H, int W, void* stream);
size_t sisr_conv9_wgrad_workspace_bytes(int B, int H, int W);
int sisr_conv9_wgrad(const float* x, const float* dy, float* dw, float* db, float* workspace, size_t workspace_bytes, int B,
                     int H, int W, void* stream);
int sisr_clamp01(const float* a, const float* grad, float* out, long n, int backward, void* stream);

/* ---- around the non-local attention: 1x1 projections, pooling, output projection (csrc/nonlocal.hip) ---------------
 * ref: advanced/SAN_blocks.py:104-148 (theta / phi / g = Conv2d(64, 8, 1), phi and g through MaxPool2d(2), W = Conv2d(8, 64, 1),
 * z = W(y) + x), :305-336 (the block applied per quadrant).  x, z, dz, dx: channels-last [npix][64]; proj, dproj:
 * [npix][24] (theta | phi | g).  `domains`: 9 ints in host memory B, H, W, y0, x0, hq, wq, nqy, nqx = B * nqy * nqx
 * rectangles of hq x wq positions starting at (y0, x0); domain index (b * nqy + iy) * nqx + ix, rows
 * [domain][position][8], pooled rows [domain][(hq / 2) * (wq / 2)][8] (floor mode).
 * sisr_nl_project_bwd: dx = dproj . Wp + dz, and part[sisr_nl_project_bwd_parts(npix)][33][64] ordered partial sums
 *   (rows 0..23 = d(theta | phi | g weight)[n][c], row 32 = the 24 bias gradients): sum with sisr_sum_partials.
 * sisr_nl_output_bwd: dy rows, and part[sisr_nl_output_bwd_parts(domains)][64 * 8 + 64] (dW [64][8], then db [64]). */
int sisr_nl_project_fwd(const float* x, const float* w_theta, const float* b_theta, const float* w_phi, const float* b_phi,
                        const float* w_g, const float* b_g, float* proj, long npix, void* stream);
int sisr_nl_project_bwd_parts(long npix);
int sisr_nl_project_bwd(const float* x, const float* dproj, const float* dz, const float* w_theta, const float* w_phi,
                        const float* w_g, float* dx, float* part, long npix, void* stream);
int sisr_nl_split_pool_fwd(const float* proj, float* theta, float* phi, float* g, const int* domains, void* stream);
int sisr_nl_split_pool_bwd(const float* proj, const float* dtheta, const float* dphi, const float* dg, float* dproj,
                           const int* domains, void* stream);
int sisr_nl_output_fwd(const float* y, const float* x, const float* w, const float* bias, float* z, const int* domains,
                       void* stream);
int sisr_nl_output_bwd_parts(const int* domains);
int sisr_nl_output_bwd(const float* dz, const float* y, const float* w, float* dy, float* part, const int* domains,
                       void* stream);

/* ---- image-quality metrics (csrc/metrics.hip) ----------------------------------------------------------------------
 * ref: sr_tools/metrics.py:64-91 -> skimage.metrics.structural_similarity(a, b, data_range, gaussian_weights=True, sigma=1.5,
 * use_sample_covariance=False), float64 form: Gaussian window (11 taps, sigma 1.5), population covariance, the mean of the SSIM
 * map over the (h - 10) x (w - 10) windows that lie inside the image.  a, b: n contiguous fp32 images [n][channels][h][w];
 * channels == 3: RGB, clipped to [0, 1] and compared on Y = (0.299 R + 0.587 G) + 0.114 B in fp32 (NaN stays NaN);
 * channels == 1: the planes as given.  out: n doubles on the device, one SSIM per image.  Two launches, no atomics: a repeat
 * call is bit-identical.  Refused before any launch (-1): null pointers, n <= 0, h or w < 11, channels other than 1 or 3,
 * data_range not finite or <= 0, workspace_bytes < sisr_ssim_workspace_bytes(n, h, w). */
size_t sisr_ssim_workspace_bytes(int n, int h, int w);
int sisr_ssim(const float* a, const float* b, int n, int channels, int h, int w, double data_range, double* out,
              void* workspace, size_t workspace_bytes, void* stream);

/* ---- structural (SSIM) training loss (csrc/ssim_loss.hip) -------------------------------------------------------------
 * The mean SSIM of two batches and its gradient with respect to the first (no counterpart in the reference; the loss
 * pixel term + alpha (1 - mean SSIM) of structural.StructuralMechanism).  sr, y: `planes` contiguous fp32 planes [planes][h][w]
 * (a (B, C, H, W) batch is B * C planes), each compared as given: no clipping, no Y conversion.  Per plane the quantity of
 * sisr_ssim: Gaussian window (11 taps, sigma 1.5), population covariance, C1 = (0.01 R)^2, C2 = (0.03 R)^2, on the
 * (h - 10) x (w - 10) windows inside the image, all in float64.  value: one float on the device, the mean of S over all
 * windows of all planes -- double sums in a fixed order, divided by the count, rounded to fp32 once.  grad (optional):
 * [planes][h][w] fp32, d value / d sr; y takes none.  Two launches, three with grad; no atomics: a repeat call is
 * bit-identical.  No allocation and no host synchronisation: capturable.  workspace: the tile sums and, with grad, three
 * float64 coefficient maps on the window grid (24 bytes per window).  Refused before any launch: null sr / y / value /
 * workspace, planes <= 0, h or w < 11, data_range not finite or <= 0, workspace_bytes <
 * sisr_ssim_loss_workspace_bytes(planes, h, w, grad != NULL) (-1); a workspace that is not 16-byte aligned or a float
 * pointer that is not 4-byte aligned (-2); more than 2^31 - 1 tiles (-4). */
size_t sisr_ssim_loss_workspace_bytes(int planes, int h, int w, int want_grad);
int sisr_ssim_loss(const float* sr, const float* y, int planes, int h, int w, double data_range, float* value,
                   float* grad /* nullable */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- multi-scale SSIM (csrc/ms_ssim.hip) ---------------------------------------------------------------------------------
 * MS-SSIM of two batches, plane by plane, and the gradient of its batch mean with respect to the first (no counterpart in
 * the reference; the loss term of multiscale.MultiScaleStructuralMechanism and the metric of metrics.batch_ms_ssim).
 * sr, y: [planes][h][w] contiguous fp32, each plane compared as given.  Scale 0 is the plane; scale j + 1 is the 2 x 2 mean
 * of scale j with stride 2, a trailing odd row or column dropped.  On every scale the window maps of sisr_ssim_loss with the
 * same C1, C2; c_j = mean over windows of A2 / B2 for j < levels - 1 and of S at the last scale; the plane's value is
 * prod_j c_j^weights[j], and exactly 0 (with an exactly zero gradient) when any c_j <= 0, a scale of weight 0 included
 * (the rule looks at the means, not at the weights).  weights: `levels` doubles on the HOST, read at call time.
 * per_plane (optional): [planes] doubles on the device.  value (optional): one float on the device, the mean of the
 * planes' values rounded to fp32 once.  At least one of the two is given.  grad (optional): [planes][h][w] fp32,
 * d value / d sr.  Everything in between is float64, pow included.  3 * levels + 1 launches with value and grad (16 for
 * five levels; `levels` fewer without grad, one fewer without value), none depending on planes; no atomics: a repeat
 * call is bit-identical.  No allocation and no host synchronisation: capturable.  Refused before any launch: null sr / y / weights / workspace, neither
 * per_plane nor value, planes <= 0, levels outside 1 .. 8, h or w < 11 * 2^(levels - 1), a weight that is negative or not
 * finite, data_range not finite or <= 0, workspace_bytes < sisr_ms_ssim_workspace_bytes(planes, h, w, levels, grad != NULL)
 * (-1); a workspace that is not 16-byte aligned, a float pointer that is not 4-byte or per_plane that is not 8-byte aligned
 * (-2); more than 2^31 - 1 tiles (-4).  sisr_ms_ssim_workspace_bytes returns 0 for a refused shape. */
size_t sisr_ms_ssim_workspace_bytes(int planes, int h, int w, int levels, int want_grad);
int sisr_ms_ssim(const float* sr, const float* y, int planes, int h, int w, double data_range,
                 const double* weights /* host */, int levels, double* per_plane /* nullable */, float* value /* nullable */,
                 float* grad /* nullable */, void* workspace, size_t workspace_bytes, void* stream);
/* y[n][h][w] = (0.299 R + 0.587 G) + 0.114 B of rgb[n][3][h][w] clipped to [0, 1], in fp32 and in the operation order of
 * sisr_ssim (channels == 3): the planes metrics.batch_ms_ssim hands to sisr_ms_ssim.  One launch. */
int sisr_luma_clip(const float* rgb, int n, int h, int w, float* y, void* stream);

/* ---- frequency-domain (FFT L1) training loss (csrc/freq_loss.hip) ------------------------------------------------------
 * The mean absolute real and imaginary part of the orthonormal 2-D DFT of sr - y over the half spectrum, and its gradient
 * with respect to sr (no counterpart in the reference; the loss base + beta * value of frequency.FrequencyMechanism).
 * sr, y: `planes` contiguous fp32 planes [planes][h][w]; wh = w / 2 + 1; F = rfft2(sr - y, norm = 'ortho') per plane;
 * value = (sum |Re F| + sum |Im F|) / (2 planes h wh): one float on the device, float64 sums of per-workgroup partials in
 * a fixed order, rounded to fp32 once.  grad (optional): [planes][h][w] fp32, d value / d sr with sign(0) = 0; y takes none.
 * The transform runs as matrix products on the fp32 MFMA against four tables that the caller keeps per (h, w):
 *   sisr_freq_loss_tables writes Ch, Sh ([h][h]) and Cw, Sw ([wh][w]) in that order, sisr_freq_loss_table_bytes(h, w)
 *   bytes in all: C[k][j] = cos(2 pi r / N), S[k][j] = sin(2 pi r / N), r = k j mod N, evaluated in float64 and rounded
 *   once; exactly 0 / +-1 at quarter turns, which makes the imaginary parts at the self-conjugate bins exact zeros.
 * Three launches, five with grad; no atomics: a repeat call is bit-identical.  No allocation and no host synchronisation:
 * capturable.  workspace: the partials, two fp32 [planes][h][wh] maps and, with grad, one sign byte per bin.
 * Refused before any launch: null sr / y / tables / value / workspace, planes < 1, h or w outside [2, 4096],
 * workspace_bytes < sisr_freq_loss_workspace_bytes(planes, h, w, grad != NULL) (-1; the size queries return 0 for such
 * extents); a workspace that is not 16-byte aligned or a float pointer that is not 4-byte aligned (-2); planes > 65535 (-4). */
size_t sisr_freq_loss_table_bytes(int h, int w);
int sisr_freq_loss_tables(int h, int w, float* tables, void* stream);
size_t sisr_freq_loss_workspace_bytes(int planes, int h, int w, int want_grad);
int sisr_freq_loss(const float* sr, const float* y, int planes, int h, int w, const float* tables, float* value,
                   float* grad /* nullable */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- SRCNN / VDSR building blocks (csrc/basic.hip) ------------------------------------------------------------------
 * ref: SISR/models/basic/architectures.py (SRCNN, VDSR: K x K convs, padding K/2), basic/handlers.py (nn.MSELoss).
 * K odd, 1..9.  Maps between layers: channels-last, cp = 32 or 64 channels (real channels first, the rest zero); the image
 * ends are planar (B,1,H,W).  Weights keep their OIHW layout with the REAL channel counts.  Refused before any launch:
 * null / empty operands (-1), a K, width or padded width outside these limits (-4), misaligned maps (-2).
 * sisr_convk_y2f: y[b,h,w,c] = act(bias[c] + sum_k x[b,h+kh-K/2,w+kw-K/2] w[c][kh][kw]), channels >= cout written as zero;
 *   flip_taps reads w[c][K-1-kh][K-1-kw] (the input gradient of sisr_convk_f2y); mask (a cp-channel map, optional) zeroes the
 *   result where the map is <= 0.
 * sisr_convk_f2y: y[b,h,w] = bias[0] + sum_{c<cin,k} x[b,h+kh-K/2,w+kw-K/2,c] w[0][c][kh][kw] (+ residual[b,h,w]).
 * sisr_corrk_y: dw[c][kh][kw] = sum_pix P[pix + s (k - K/2)] Q[pix][c], s = -1 with flip_taps (P planar, Q channels-last;
 *   P = x, Q = dy for the 1 -> C end, P = dy, Q = x with flip_taps for the C -> 1 end); qmask (optional) zeroes Q where the
 *   map is <= 0; db_mode 0 none, 1 db[c] = sum Q[.,c], 2 db[0] = sum P.  Ordered two-stage sums: a repeat is bit-identical.
 * sisr_pack_convk: OIHW (cout,cin,K,K) -> the MFMA kernel's order for the forward conv (fwd, K*K*cop*cip floats) and, when
 *   dgrad is given, for its input gradient (taps flipped, channel roles swapped).
 * sisr_convk_mfma: y = act(conv(x [masked by in_mask > 0], packed) + bias[< nbias]) between channels-last maps of cin_p and
 *   cout_p channels on v_mfma_f32_32x32x2_f32; relu, then mask (optional: zero where the map is <= 0).
 * sisr_wgradk_mfma: dw (cout,cin,K,K) and db (cout, optional) from x (cip channels) and dy (cop channels, optionally
 *   masked by dymask > 0), ordered sums.
 * sisr_mse_loss: loss = mean (a - b)^2, grad (optional) = 2 (a - b) / n, ordered two-stage sum. */
int sisr_convk_y2f(const float* x, const float* w, const float* bias, const float* mask, float* y, int B, int H, int W, int K,
                   int cout, int cp, int relu, int flip_taps, void* stream);
int sisr_convk_f2y(const float* x, const float* w, const float* bias, const float* residual, float* y, int B, int H, int W,
                   int K, int cin, int cp, void* stream);
size_t sisr_corrk_y_workspace_bytes(int B, int H, int W, int K, int cp);
int sisr_corrk_y(const float* P, const float* Q, const float* qmask, float* dw, float* db, int B, int H, int W, int K,
                 int channels, int cp, int flip_taps, int db_mode, float* workspace, size_t workspace_bytes, void* stream);
int sisr_pack_convk(const float* w, float* fwd, float* dgrad, int K, int cout, int cin, int cop, int cip, void* stream);
int sisr_convk_mfma(const float* x, const float* in_mask, const float* packed, const float* bias, int nbias, const float* mask,
                    float* y, int B, int H, int W, int K, int cin_p, int cout_p, int relu, void* stream);
size_t sisr_wgradk_mfma_workspace_bytes(int B, int H, int W, int K, int cin_p, int cout_p);
int sisr_wgradk_mfma(const float* x, const float* dy, const float* dymask, float* dw, float* db, int B, int H, int W, int K,
                     int cout, int cin, int cop, int cip, float* workspace, size_t workspace_bytes, void* stream);
size_t sisr_mse_loss_workspace_bytes(void);
int sisr_mse_loss(const float* a, const float* b, long n, float* loss, float* grad, float* workspace, void* stream);

/* ---- degradation-predictor building blocks (csrc/basic.hip) -----------------------------------------------------------
 * LeakyReLU forms of the K x K MFMA conv and its gradients (same tiles, same packing, same refusals as the forms above; a
 * NaN or infinite slope is refused with -1), and the global mean of a map.  The slope is a per-call argument.
 * sisr_convk_mfma_leaky: y = conv(x', packed) + bias[< nbias], then with act != 0  y = y > 0 ? y : slope * y (one fp32
 *   rounding).  x' = x, or with in_mask (the input-gradient form: x is dy, in_mask the saved output of the layer whose
 *   gradient is taken)  x' = in_mask > 0 ? x : slope * x.
 * sisr_wgradk_mfma_leaky: sisr_wgradk_mfma with dy read as dymask > 0 ? dy : slope * dy (dymask required); the workspace is
 *   that of sisr_wgradk_mfma_workspace_bytes.
 * sisr_map_mean: out[b][ch] = (sum_pix x[b][pix][ch]) / (H W), ch < c, of a channels-last map of cp = 32 / 64 channels
 *   (H W <= 2^24).  Ordered two-stage float64 sum: fixed pixel ranges per partial, then the partials in order; the result is
 *   the correctly rounded mean and a repeat is bit-identical.  workspace: 8-byte aligned, sisr_map_mean_workspace_bytes.
 * sisr_map_mean_bwd: dx[b][pix][ch] = g[b][ch] / (H W) for ch < c and 0 for c <= ch < cp. */
int sisr_convk_mfma_leaky(const float* x, const float* in_mask, const float* packed, const float* bias, int nbias, float* y,
                          int B, int H, int W, int K, int cin_p, int cout_p, int act, float slope, void* stream);
int sisr_wgradk_mfma_leaky(const float* x, const float* dy, const float* dymask, float* dw, float* db, int B, int H, int W,
                           int K, int cout, int cin, int cop, int cip, float* workspace, size_t workspace_bytes, float slope,
                           void* stream);
size_t sisr_map_mean_workspace_bytes(int B, int H, int W, int cp);
int sisr_map_mean(const float* x, float* out, int B, int H, int W, int c, int cp, void* workspace, size_t workspace_bytes,
                  void* stream);
int sisr_map_mean_bwd(const float* g, float* dx, int B, int H, int W, int c, int cp, void* stream);

/* ---- stride-2 K x K conv on the fp32 matrix cores (csrc/basic.hip) ------------------------------------------------------
 * nn.Conv2d(cin, cout, K, stride=2, padding=K/2), K odd, 1..9, between channels-last maps of 32 / 64 (padded) channels, with
 * the packings of sisr_pack_convk and the refusals of the stride-1 forms (-1 null operand / bad size / NaN or infinite
 * slope, -4 K or width outside the limits, -2 misaligned map).  H x W is ALWAYS the size of the conv's input x (and of dx);
 * the strided side is Ho x Wo = sisr_convk_s2_out_size(H) x sisr_convk_s2_out_size(W), with
 * sisr_convk_s2_out_size(n) = (n - 1) / 2 + 1 (0 for n < 1).  LeakyReLU family only; the slope is a per-call argument.
 * sisr_convk_s2_mfma_leaky: y[b,ho,wo,co] = bias[co < nbias] + sum x[b,2ho+kh-K/2,2wo+kw-K/2,ci] w[co][ci][kh][kw] with
 *   `packed` the forward packing; then with act != 0  y = y > 0 ? y : slope * y.  Only the outputs' own products are formed.
 * sisr_dgradk_s2_mfma_leaky: dx (B,H,W,cin_p) = the transposed conv of dy' (B,Ho,Wo,cout_p) with `packed_dgrad`, the 'dgrad'
 *   packing; dy' = dy, or with dymask (the layer's saved output)  dymask > 0 ? dy : slope * dy.  Polyphase: each (row parity,
 *   column parity) class of dx is a stride-1 correlation of dy with the taps of that parity; no zero-inserted dy exists.
 * sisr_wgradk_s2_mfma_leaky: dw[co][ci][kh][kw] = sum dy'[b,ho,wo,co] x[b,2ho+kh-K/2,2wo+kw-K/2,ci] and db (optional) =
 *   the ordered column sum of dy'; dymask optional as above; workspace of sisr_wgradk_s2_mfma_workspace_bytes. */
int sisr_convk_s2_out_size(int n);
int sisr_convk_s2_mfma_leaky(const float* x, const float* packed, const float* bias, int nbias, float* y, int B, int H, int W,
                             int K, int cin_p, int cout_p, int act, float slope, void* stream);
int sisr_dgradk_s2_mfma_leaky(const float* dy, const float* dymask, const float* packed_dgrad, float* dx, int B, int H, int W,
                              int K, int cout_p, int cin_p, float slope, void* stream);
size_t sisr_wgradk_s2_mfma_workspace_bytes(int B, int H, int W, int K, int cin_p, int cout_p);
int sisr_wgradk_s2_mfma_leaky(const float* x, const float* dy, const float* dymask, float* dw, float* db, int B, int H, int W,
                              int K, int cout, int cin, int cop, int cip, float* workspace, size_t workspace_bytes,
                              float slope, void* stream);

/* ---- pointwise (1 x 1) layers up to 128 channels wide, with a per-image bias (csrc/basic.hip) --------------------------
 * Channels-last maps of cin_p, cout_p in {32, 64, 128} (padded) channels; refusals as above (a width outside the three: -4).
 * sisr_pack_conv1: (cout,cin[,1,1]) weight -> the MFMA order, fwd (cop*cip floats) and, when given, dgrad (roles swapped).
 * sisr_conv1_mfma_leaky: y[b,pix,co] = bias[co] + ibias[b*nbias + co] (co < nbias; either pointer may be null) +
 *   sum_ci x'[b,pix,ci] w[co][ci], then with act != 0 the LeakyReLU(slope); x' = x, or with in_mask (the input-gradient
 *   form on the dgrad packing: x is dy, in_mask the saved output)  in_mask > 0 ? x : slope * x.
 * sisr_wgrad1_mfma_leaky: dw (cout,cin), and optionally db (cout) and dib (B x cout: the gradient of ibias, the per-image
 *   column sum of dy') from x and dy' = dymask > 0 ? dy : slope * dy (dymask optional).  Every sum is ordered, without
 *   atomics: a repeat is bit-identical.  workspace: sisr_wgrad1_mfma_workspace_bytes. */
int sisr_pack_conv1(const float* w, float* fwd, float* dgrad, int cout, int cin, int cop, int cip, void* stream);
int sisr_conv1_mfma_leaky(const float* x, const float* in_mask, const float* packed, const float* bias, const float* ibias,
                          int nbias, float* y, int B, int H, int W, int cin_p, int cout_p, int act, float slope, void* stream);
size_t sisr_wgrad1_mfma_workspace_bytes(int B, int H, int W, int cin_p, int cout_p);
int sisr_wgrad1_mfma_leaky(const float* x, const float* dy, const float* dymask, float* dw, float* db, float* dib, int B, int H,
                           int W, int cout, int cin, int cop, int cip, float* workspace, size_t workspace_bytes, float slope,
                           void* stream);

/* ---- geometric self-ensemble around a network (csrc/ensemble.hip) -----------------------------------------------------
 * The eight flips / transposes of an image batch as two batches a network runs as they are, and the mean of its eight
 * outputs with each mapped back (the "+" protocol of the EDSR / RCAN / HAN / SAN papers).  All maps contiguous NCHW fp32;
 * batches are variant-major: image i of variant k is entry k * n + i.  upright (4n, c, h, w), k = 0..3: the image, its
 * columns reversed, its rows reversed, both reversed; turned (4n, c, w, h): the same four operations applied to the
 * transposed image.
 * sisr_dihedral_fan: a pure copy, every output element bit-identical to its source.
 * sisr_dihedral_merge: out (n, c, H, W) from upright (4n, c, H, W) and turned (4n, c, W, H), variant k mapped back as u_k / t_k:
 *   out = (((u0 + u1) + (u2 + u3)) + ((t0 + t1) + (t2 + t3))) * 0.125f, plain fp32 adds in this order.
 * One launch each, any h, w, c >= 1 (16-byte accesses where the row length and the pointers allow them).  Refused before
 * any launch: null pointers, n, c, h or w <= 0 (-1); more than 2^31 - 1 tiles of 64 x 64 (-4). */
int sisr_dihedral_fan(const float* x, int n, int c, int h, int w, float* upright, float* turned, void* stream);
int sisr_dihedral_merge(const float* upright, const float* turned, int n, int c, int H, int W, float* out, void* stream);

/* ---- perceptual (VGG19 feature) loss: everything but the convolutions (csrc/perceptual.hip) ---------------------------
 * ref: sr_tools/loss_functions.py:6-22 PerceptualMechanism, SISR/models/feature_extractors/VGGNets.py:118-131
 * VGGFeatureExtractor ((img - mean) / std, then torchvision's vgg19.features[:35]: 3x3 convs + ReLU, four MaxPool2d(2, 2)).
 * The convs run on sisr_conv3x3_c64; these are the streams around them.  Maps are channels-last fp32 with a 64-multiple of
 * channels, images planar (B,3,H,W) fp32; mean3 / std3: three floats on the device.
 * sisr_vgg_prep_fwd: out[b,h,w,c] = (img[b,c,h,w] - mean3[c]) / std3[c] for c < 3 -- an IEEE subtraction, then a correctly
 *   rounded division, bit for bit torch's fp32 expression -- and 0 for 3 <= c < cp.
 * sisr_vgg_prep_bwd: dimg[b,c,h,w] = gmap[b,h,w,c] / std3[c], c < 3 (channels >= 3 of gmap are not read).
 * sisr_maxpool2_fwd: out (B, H/2, W/2, C) = MaxPool2d(2, 2)(y), floor mode: an odd last row / column is dropped.
 * sisr_maxpool2_relu_bwd: the input gradient of maxpool2(y) for a post-ReLU map y with that ReLU's derivative applied:
 *   dy[p] = dout[window(p)] if p holds the first maximum of its window, in the scan order (0,0), (0,1), (1,0), (1,1), and
 *   y[p] > 0; else 0.  Pixels outside every window get 0.  A gather: no atomics, a repeat call is bit-identical.
 * One launch each.  Refused before any launch: null pointers, B, H, W or the channel count <= 0 (-1); a channel count that
 * is not a multiple of 64, H < 2 or W < 2 for the pool (-4); a map that is not 16-byte aligned (-2). */
int sisr_vgg_prep_fwd(const float* img, const float* mean3, const float* std3, float* out, int B, int H, int W, int cp,
                      void* stream);
int sisr_vgg_prep_bwd(const float* gmap, const float* std3, float* dimg, int B, int H, int W, int cp, void* stream);
int sisr_maxpool2_fwd(const float* y, float* out, int B, int H, int W, int C, void* stream);
int sisr_maxpool2_relu_bwd(const float* y, const float* dout, float* dy, int B, int H, int W, int C, void* stream);

/* ---- JPEG degradation (csrc/jpeg.hip) -----------------------------------------------------------------------------------
 * ref: Code/data_converter.py jpeg_compress: `image.save(buf, "JPEG", subsampling=0, quality=q)` then `PIL.Image.open(buf)`.
 * The decoded pixels of that round trip, byte for byte, without the file: libjpeg's integer arithmetic per 8 x 8 block
 * (jccolor, jfdctint, jcdctmgr, jidctint, jdcolor; the lossless entropy coder is left out).  in: planar [C][H][W] uint8 on
 * the device, as sisr_pil_resample writes it; out: [C][H][W] uint8 (to_float = 0) or fp32 = byte / 255 (to_float = 1, the
 * rounding of sisr_pil_resample's to_float).  C = 3: RGB through YCbCr 4:4:4; C = 1: a grey plane on the luminance table
 * (PIL mode L).  The image is padded to whole blocks by edge replication; nothing outside [C][H][W] is written.  The two
 * quantisation tables (Annex K scaled by the quality as jcparam.c scales them) are built inside the call and reach the
 * kernel by value.  One launch, no workspace, no atomics, no state: capturable, a repeat call is bit-identical.  Refused
 * before any launch (-1): null pointers, C other than 1 or 3, H or W < 1, quality outside 1..100, to_float other than 0 or 1;
 * more than 2^31 - 1 blocks (-4). */
int sisr_jpeg_roundtrip(const unsigned char* in, void* out, int C, int H, int W, int quality, int to_float, void* stream);

/* ---- tile-level online degradation (csrc/degrade_tiles.hip; `[data] degrade_tiles = true`) ----------------------------
 * A training batch's LR and HR tiles from device-resident HR images with a constant number of launches, no whole-image
 * intermediate, no workspace, no atomics and no state (capturable; a repeat call is bit-identical).  The LR tile equals, bit
 * for bit, the pixels that sisr_blur_quant (+ sisr_noise_quant) on the WHOLE image, the centre crop and both passes of
 * sisr_pil_resample give at the tile's position: same tap order in the blur, reflection against the image, the whole-image
 * coefficient tables indexed at the tile's absolute LR rows / columns; the HR window a strip of LR rows needs is read off the
 * tables' bounds.  One record per sample: */
typedef struct sisr_degrade_tile {
  const float* image;                        /* [C][H][W] fp32 on the device */
  const int *bounds_h, *coef_h;              /* device tables of (rw -> rw / scale): bounds [out][2], coef [out][ksize_h] */
  const int *bounds_v, *coef_v;              /* ... and of (rh -> rh / scale) */
  int H, W;                                  /* image size */
  int t0, l0, rh, rw;                        /* centre-crop box (image_manipulation.downsample): rh, rw multiples of scale */
  int ty, tx;                                /* the tile's origin in the un-augmented LR image (rh / scale) x (rw / scale) */
  int ksize_h, ksize_v;                      /* row length of the coefficient tables: 4 scale + 1 */
  int flips;                                 /* applied on the store: 1 hflip | 2 vflip | 4 transpose; out(i, j) = tile(ry, rx) with
                                                (a, b) = transpose ? (j, i) : (i, j), ry = vflip ? c-1-a : a, rx = hflip ? c-1-b : b,
                                                which is sisr_crop_augment's index map restricted to the tile */
  int noise;                                 /* 0: byte(255 blur), sisr_blur_quant's; 1: sisr_noise_quant's arithmetic with ... */
  float sigma;                               /* ... this noise level (0 allowed) and the field of `seed` below */
  unsigned seed;
} sisr_degrade_tile;
size_t sisr_degrade_tile_bytes(void);
/* tiles_host: the B records in host memory, checked here before anything is launched; tiles_dev: their device copy, which the
 * kernel reads; kernels [B][l][l] fp32 on the device (l <= 21; odd and even l take sisr_blur_quant's padding rule); out
 * [B][C][c][c] uint8 (to_float = 0) or fp32 = byte / 255.  One launch: a workgroup per (strip of 8 LR rows, channel, sample)
 * keeps the strip's blurred, quantised HR window and the horizontal pass's rows in LDS.  -1: null pointers (records' included:
 * image, or tables not supplied / of another scale's ksize), non-positive sizes, a crop box outside the image or not a
 * multiple of the scale, a tile that leaves the LR image (ty + c > rh / scale, ...), flips outside 0..7, sigma < 0, to_float
 * other than 0 or 1;  -4: scale outside 2..4, l > 21 or l / 2 >= H or W, B or C > 65535, a tile whose window needs more than
 * 64 KB of LDS (c = 64 at x 4 needs 45 KB). */
int sisr_degrade_tiles(const void* tiles_host, const void* tiles_dev, const float* kernels, void* out, int B, int C, int c,
                       int l, int scale, int to_float, void* stream);
/* sisr_jpeg_roundtrip on every tile of a batch, one launch: in [B][C][c][c] uint8 in source orientation, the block grid at
 * the tile's origin (NOT the image's: a crop-level round trip, not a crop of the whole image's), edge replication to whole
 * blocks, quality[b] (device, int32) for sample b, the scaled Annex-K tables built in the kernel; out [B][C][c][c] uint8 or
 * fp32 = byte / 255 through flips[b] (device, the bits of sisr_degrade_tile.flips; NULL: none).  The qualities are device
 * values, which the host cannot check: the kernel clamps them to 1..100 and degrade.degrade_tiles refuses others before the
 * upload.  -1: null in / out / quality, in == out, B < 1, C other than 1 or 3, c < 1, to_float other than 0 or 1;  -4: B >
 * 65535, c > 32768. */
int sisr_jpeg_roundtrip_batch(const unsigned char* in, void* out, const int* quality, const int* flips, int B, int C, int c,
                              int to_float, void* stream);
/* The N(0,1) field of the tile-level noise on its own -- a pure function of (seed, channel, row, column), shared with
 * sisr_degrade_tiles as one device function (csrc/noise_field.h):
 *   words = Philox4x32-10(counter = (column >> 2, row, channel, 0), key = (seed, 0));
 *   u_i = (float(words[i] >> 8) + 0.5f) * 2^-24 in fp32 (exact below 2^23, round-to-even above: u in (0, 1]);
 *   columns 4q, 4q + 1 = r cos(a), r sin(a) with r = sqrtf(-2 logf(u_0)), a = 2 pi u_1; columns 4q + 2, 4q + 3 the same of
 *   (u_2, u_3); precise logf / cosf / sinf.  THIS MAP IS KEPT: seeded runs depend on it.
 * field [C][H][W] fp32 and / or words [C][H][ceil(W / 4)][4] uint32 (either may be null, not both). */
int sisr_normal_field(unsigned seed, float* field, unsigned* words, int C, int H, int W, void* stream);
/* sisr_crop_augment reading a centre-cropped image in place (no copy of the crop): params[b] = {rh, rw, top, left, hflip,
 * vflip, transpose, H, W, t0, l0, 0}: src[b] is the full [C][H][W] image, (t0, l0, rh, rw) its crop box, the rest as
 * sisr_crop_augment's record on the cropped image.  params_host is checked before the launch (box inside the image, tile
 * inside the augmented crop), params_dev is its device copy. */
int sisr_crop_augment_strided(const float* const* src, const int* params_host, const int* params_dev, float* dst, int B, int C,
                              int crop, void* stream);

/* ---- tile-level degradation for interpolated-input and Y-channel models (csrc/interp_tiles.hip) -------------------------
 * sisr_upsample_tiles: the c x c tiles of a batch's bicubic pre-up-sampled LR images -- per sample Pillow's
 * `resize((w * s, h * s), BICUBIC)` of the LR bytes, ToTensor -- from the cw x cw LR WINDOW each tile depends on
 * (sisr_degrade_tiles' uint8 output, source orientation), without the up-sampled image ever existing.  Both passes of
 * libImaging/Resample.c's 8-bit resampler run on the whole-image tables of (h -> H) and (w -> W), indexed at the tile's
 * absolute rows / columns, with the tap addresses taken relative to the window's origin; the horizontal rows of a 32 x 32
 * output block stay in LDS (the block-level resampler of sisr_pil_upsample, one copy).  A tile equals the crop of
 * sisr_pil_upsample's image through the same flips, bit for bit.  One record per sample: */
typedef struct sisr_upsample_tile {
  const int *bounds_h, *coef_h;              /* device tables of (w -> W): bounds [W][2], coef [W][5] */
  const int *bounds_v, *coef_v;              /* ... and of (h -> H) */
  int h, w;                                  /* LR image size */
  int H, W;                                  /* size of the up-sampled image: H = s h, W = s w for one integer s >= 1 */
  int wy, wx;                                /* the window's origin in the LR image */
  int ty, tx;                                /* the tile's origin in the un-augmented up-sampled image (any residue mod s) */
  int flips;                                 /* applied on the store, as sisr_degrade_tile.flips */
  int pad;
} sisr_upsample_tile;
size_t sisr_upsample_tile_bytes(void);
/* tiles_host: the B records in host memory, checked here before anything is launched; tiles_dev: their device copy, which the
 * kernel reads; windows [B][C][cw][cw] uint8 on the device; out fp32 on the device in one of three forms:
 *   0: RGB [B][C][c][c] (any C; a grey source, C = 1, is written as it is);  1: BT.601 'jpg' YCbCr [B][3][c][c];
 *   2: Y alone [B][1][c][c] -- 1 and 2 with the fp32 roundings of sisr_pil_upsample's second output.
 * One launch whatever B is, no workspace, no atomics, no state: capturable, a repeat call is bit-identical.  -1: null pointers
 * (the records' tables included), non-positive sizes, a tile that leaves the up-sampled image, a window that leaves the LR
 * image or does not cover every tap of the tile's rows and columns (the taps are recomputed on the host as Resample.c
 * computes them), flips outside 0..7, form outside 0..2;  -4: ksize != 5, form 1 or 2 with C != 3, H / h != W / w or not
 * an integer, B (or B * ceil(C / 3)) > 65535. */
int sisr_upsample_tiles(const void* tiles_host, const void* tiles_dev, const unsigned char* windows, float* out, int ksize, int B,
                        int C, int c, int cw, int form, void* stream);
/* rgb [B][3][n] fp32 -> out [B][3][n] BT.601 'jpg' YCbCr, or [B][1][n] Y alone with y_only = 1: every product and sum rounded
 * to fp32 on its own in the order data.rgb_to_ycbcr(im_type='jpg') writes them (sisr_pil_upsample's conversion, one copy), so
 * bit-identical to it.  For the HR tiles of a 'ycbcr' batch and for LR tiles that are not up-sampled.  One launch.  -1: null
 * pointers, rgb == out, B or n < 1, y_only other than 0 or 1;  -4: B > 65535. */
int sisr_rgb_to_ycbcr(const float* rgb, float* out, int B, long n, int y_only, void* stream);

/* ---- the output stage of evaluation / validation (csrc/eval_output.hip): Y-MSE against the HR batch and 8-bit RGB bytes -------
 * One streaming pass over n network outputs on the device, either result or both:
 *   mse[i]   the mean over shave <= row < h - shave, shave <= col < w - shave of (Ys - Yh)^2, the difference in fp32, its square
 *            and the sum in float64.  Ys: sr_planes == 3, the Y of the clipped RGB output as metrics.batch_rgb_to_ycbcr forms it
 *            in fp32 ((0.299 R + 0.587 G) + 0.114 B, every operation rounded); sr_planes == 1, the plane itself clipped to [0, 1].
 *            Yh: hr_form 0, the same of hr (n, hr_planes >= 3, h, w) RGB, planes 0 .. 2; hr_form 1, plane 0 of hr (n, hr_planes, h, w)
 *            clipped.  Y-PSNR is 20 log10(max / sqrt(mse)) on the host (metrics.batch_psnr).
 *   rgb8     n x h x w x 3 bytes, HWC.  sr_planes == 3: rint(clip(c) * 255), ties to even as np.round, byte for byte
 *            `(clip(x) * 255).round().astype(uint8)`.  sr_planes == 1: (Y, Cb, Cr) = the clipped (sr, plane 1 of chroma, plane 2 of
 *            chroma), chroma (n, 3, h, w); metrics.ycbcr_to_rgb_jpg in its fp32 operation order; rint(v * 255) CLAMPED to 0 .. 255.
 *            Where the host's rounded value lies in 0 .. 255 the byte equals the host's `(rgb * 255).round().astype(uint8)`;
 *            elsewhere it saturates at 0 or 255 where the host's cast wraps (253 for -0.01, 2 for 1.01).  NaN gives 0.
 * The sum is ordered in two stages (per-block partials in the workspace in block order, then one block per image): no atomics, a
 * repeat call is bit-identical.  Two launches with mse, one without; no allocation, no host synchronisation: capturable.
 * workspace: sisr_eval_output_workspace_bytes(n, h, w) bytes, 16-byte aligned, needed with mse only; 0 for a shape that is refused.
 * -1: null sr; neither mse nor rgb8; mse without hr; sr_planes not 1 or 3; sr_planes == 1 with rgb8 and no chroma; with hr,
 *     hr_form not 0 or 1, hr_planes < 1 (< 3 with hr_form 0); n, h or w <= 0; shave < 0 or 2 shave >= min(h, w); with mse, a null
 *     or too small workspace;  -2: a float pointer not 4-byte aligned, mse not 8-byte or (with mse) the workspace not 16-byte
 *     aligned;  -4: h * w above 2^31 - 2049. */
size_t sisr_eval_output_workspace_bytes(int n, int h, int w);
int sisr_eval_output(const float* sr, int sr_planes, const float* chroma, const float* hr, int hr_form, int hr_planes, int n, int h,
                     int w, int shave, double* mse, unsigned char* rgb8, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the degradation as a differentiable float operator (csrc/consistency.hip): blur + bicubic down-sampling and its adjoint --
 * Away from the image border, blur + Pillow's bicubic down-sampling by scale = 2, 3, 4 is one per-sample stride-`scale`
 * cross-correlation with a composed kernel K (B, n, n) float64 (degrade.compose_degradation):
 *   fwd   y[b][c][i][j]  = sum_ef K[b][e][f] x[b][c][scale i + off + e][scale j + off + f]     y (B, C, ho, wo), x (B, C, H, W)
 *   bwd   dx[b][c][p][q] = sum_ij K[b][p - off - scale i][q - off - scale j] g[b][c][i][j]     dx (B, C, H, W), g (B, C, ho, wo)
 * fp32 maps, float64 accumulation in a fixed order, rounded once.  bwd writes every element of dx exactly once (zeros where no
 * footprint reaches).  No atomics, no workspace, no allocation, no host synchronisation: bit-identical repeats, capturable.
 * sisr_degrade_valid_tile(backward): the edge of a workgroup's tile, in outputs (0) or in pixels of dx (1).
 * -1: a null pointer; B, C, H, W, n, ho or wo < 1; off < 0; a footprint that leaves the image (scale (ho - 1) + off + n > H, or
 *     the same along W);  -2: x, y, g or dx not 4-byte or K not 8-byte aligned;  -4: scale outside 2..4, n > 36, B * C > 65535,
 *     more than 65535 tile rows. */
int sisr_degrade_valid_tile(int backward);
int sisr_degrade_valid_fwd(const float* x, const double* K, float* y, int B, int C, int H, int W, int n, int scale, int off, int ho,
                           int wo, void* stream);
int sisr_degrade_valid_bwd(const float* g, const double* K, float* dx, int B, int C, int H, int W, int n, int scale, int off, int ho,
                           int wo, void* stream);

/* ---- dense-block growth convs (csrc/dense.hip): 3 x 3, cin -> 32, in place in a channel stack ---------------------------------
 * ref: ESRGAN's Residual Dense Block, x_j = lrelu(conv_j(cat(x, x_1 .. x_{j-1}))).  A block works on ONE channels-last stack
 * S[B][H][W][192] fp32: channels 0..63 the block input, slot j = channels 64 + 32 (j - 1) .. 64 + 32 j - 1 the output of layer j.
 * Layer j reads channels [0, cin_j), cin_j = 64 + 32 (j - 1), and writes slot j of the same pixel records: no concatenation.
 * Every map is {pointer to its first channel, pitch = floats per pixel}; zero padding 1; fp32 on v_mfma_f32_32x32x2_f32.
 * cout is always 32; cin in {64, 96, 128, 160}.  Pointers 16-byte aligned, pitches multiples of 32 (<= 4096) that hold the
 * range; slope is any finite float (0.2: ESRGAN; 0: ReLU).  Channels outside the ranges named are neither read nor written.
 *   pack   w (32, cin, 3, 3) OIHW -> packed_fwd and packed_dgrad (32 * cin * 9 floats each; either may be NULL), one launch.
 *   fwd    y[..., 0:32] = act ? (v > 0 ? v : slope * v) : v,  v = conv(x[..., 0:cin]) + bias (nullable).  x and y may lie in the
 *          same pixel records (y = x + cin, equal pitches); ranges that overlap are refused.
 *   dgrad  dx[..., 0:cin] (+)= conv^T(dy'),  dy' = dymask > 0 ? dy : slope * dy (dymask: the layer's saved output, own pitch;
 *          NULL: dy' = dy; zero takes the slope branch as in PyTorch).  accumulate = 1: dx += ..., every element read and
 *          written once by the lane that owns it (the running gradient of a stack, summed in place, deterministic).  dy and
 *          dymask may share pixel records with dx outside [0, cin).
 *   wgrad  dw (32, cin, 3, 3) = sum_pixels dy' (x) x,  db (32, nullable) = sum_pixels dy'.  Ordered two-stage sum, no atomics:
 *          a repeat call is bit-identical.  workspace: sisr_dense3x3_wgrad_workspace_bytes (0 for a shape that is refused).
 * No allocation, no host synchronisation: capturable.  Every check is made before the first device call:
 * -1: a null pointer; B, H or W < 1, B > 65535, H or W > 65536, B * H * W > 2^28; cin <= 0 or no multiple of 32; a pitch that is
 *     no multiple of 32, above 4096 or below its range; a NaN or infinite slope; overlapping read and write ranges; a workspace
 *     that is too small;  -2: a misaligned pointer;  -4: a multiple of 32 other than 64, 96, 128, 160 as cin. */
int sisr_pack_dense3x3(const float* w, float* packed_fwd, float* packed_dgrad, int cin, void* stream);
int sisr_dense3x3_fwd(const float* x, int x_pitch, int cin, const float* packed, const float* bias, int act, float slope,
                      float* y, int y_pitch, int B, int H, int W, void* stream);
int sisr_dense3x3_dgrad(const float* dy, int dy_pitch, const float* dymask, int mask_pitch, float slope,
                        const float* packed_dgrad, float* dx, int dx_pitch, int cin, int accumulate, int B, int H, int W,
                        void* stream);
size_t sisr_dense3x3_wgrad_workspace_bytes(int B, int H, int W, int cin);
int sisr_dense3x3_wgrad(const float* x, int x_pitch, int cin, const float* dy, int dy_pitch, const float* dymask, int mask_pitch,
                        float slope, float* dw, float* db, float* workspace, size_t workspace_bytes, int B, int H, int W,
                        void* stream);
/* The RRDB's skip between two stacks: y[..., 0:64] = t[..., 0:64] * g[b][c] + x[..., 0:64] (x nullable), every map with its own
 * pitch (a multiple of 32 from 64 up), g (B, 64), hw pixels per image; the product is rounded before the sum.  y may be t or x
 * itself.  -1: a null t, g or y; B or hw < 1, B * hw > 2^28; a bad pitch; y overlapping t or x otherwise;  -2: misaligned. */
int sisr_dense_skip(const float* t, int t_pitch, const float* g, const float* x, int x_pitch, float* y, int y_pitch, int B,
                    long hw, void* stream);

#ifdef __cplusplus
}
#endif
#endif
