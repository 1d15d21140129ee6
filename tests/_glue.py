"""Float64 references of the small kernels around the convs (helper module, not collected; torch only, no HIP import):
the flat Adam step and the layout / rounding kernels of csrc/misc.hip, the SFTMD pieces of csrc/sft.hip that are not the
9x9 conv (weight composition and its split, the SFT combine and its backward, the strided 64-channel maps, the clamp), and
the blur / noise quantisers of csrc/degrade.hip.

tests/test_glue_cpu.py checks every one against an independent float64 statement of the same operation (torch.optim.Adam,
float64 autograd, the oracle's BatchBlur, tensor.to(torch.bfloat16)); tests/test_glue_gpu.py compares the kernels with
them.  As in tests/_gates.py, backward and rounding references take a flag `A`: True evaluates the same computation on
absolute values with every subtraction turned into an addition, the magnitude each fp32 rounding of the kernel is relative
to, so a bound reads |got - ref| <= c * 2^-24 * mag.
"""
import math

import torch
import torch.nn.functional as F

import _exact as X

def _d(t):
    return None if t is None else t.detach().double()


def f32(v):
    """the fp32 value of a host float, as ctypes' c_float conversion rounds it"""
    return float(torch.tensor(float(v), dtype=torch.float64).float())


# ----------------------------------------------------------------------------- shared comparison idioms
def untouched(*ts):
    """every element is still the NaN the buffer was filled with"""
    if ts and ts[0].is_cuda:
        torch.cuda.synchronize()
    return all(bool(t.isnan().all()) for t in ts)


def expect_detected(got_map, want_map, what):
    assert bool(want_map.any()), f"{what}: the perturbation changes no output (test bug)"
    assert torch.equal(got_map.cpu(), want_map.cpu()), \
        f"{what}: {int(got_map.sum())} mismatches, {int(want_map.sum())} expected, or at other outputs"


def worst_ratio(got, ref, mag, c):
    """largest |got - ref| / (c * 2^-24 * mag) over the elements with mag > 0 (NaN if any element is NaN)"""
    got, ref, mag = got.detach().double(), ref.to(got.device).double(), mag.to(got.device).double()
    if bool(got.isnan().any()):
        return float("nan")
    live = mag > 0
    if not bool(live.any()):
        return 0.0
    return float(((got - ref).abs()[live] / (c * 2.0 ** -24 * mag[live])).max())


# ----------------------------------------------------------------------------- Adam (csrc/misc.hip: adam_flat_kernel)
def adam_ref(p, g, m, v, beta2, omb1, omb2, eps, step_size, bc2_sqrt, grad_scale, A=False):
    """the kernel's five lines in float64 on the fp32 inputs and scalars as passed:
        gg = g grad_scale;  m' = m + (gg - m) omb1;  v' = v beta2 + gg gg omb2;
        p' = p - step_size (m' / (sqrt(v') / bc2_sqrt + eps))
    A: |m| + (|gg| + |m|) omb1 and |p| + step_size (that / denominator); v' and the denominator are sums of non-negative
    terms already."""
    p, g, m, v = map(_d, (p, g, m, v))
    gg = g * grad_scale
    if A:
        p, gg, m = p.abs(), gg.abs(), m.abs()
    m1 = m + (gg + m if A else gg - m) * omb1
    v1 = v * beta2 + gg * gg * omb2
    upd = step_size * (m1 / (v1.sqrt() / bc2_sqrt + eps))
    return dict(m=m1, v=v1, p=p + upd if A else p - upd)


def adam_scalars(lr, b1, b2, eps, t, grad_scale=1.0, rounded=True):
    """the scalar arguments optim.FlatAdam passes at step count t, in the kernel's order after n; rounded: to fp32, as the
    C call converts them"""
    r = f32 if rounded else float
    return dict(beta2=r(b2), omb1=r(1 - b1), omb2=r(1 - b2), eps=r(eps), step_size=r(lr / (1.0 - b1 ** t)),
                bc2_sqrt=r(math.sqrt(1.0 - b2 ** t)), grad_scale=r(grad_scale))


# ----------------------------------------------------------------------------- SFT weight composition (csrc/sft.hip)
def SFT_PARAM_SHAPES(M):
    return ((32, 64 + M, 3, 3), (32,), (32, 64 + M, 3, 3), (32,), (64, 32, 3, 3), (64,), (64, 32, 3, 3), (64,))


SFT_MERGED_SHAPES = ((64, 128, 3, 3), (64,), (128, 64, 3, 3), (128,))


def sft_compose_ref(params, M):
    """(mw1, mb1, aw1, ab1, mw2, mb2, aw2, ab2) -> WA [64][128][3][3] rows (mul_conv1 | add_conv1) over inputs 0 .. 63 + M,
    bA, WB [128][64][3][3] block-diagonal (mul_conv2 on inputs 0 .. 31 | add_conv2 on 32 .. 63), bB; the rest +0.0"""
    mw1, mb1, aw1, ab1, mw2, mb2, aw2, ab2 = params
    dt = mw1.dtype
    WA, WB = torch.zeros(64, 128, 3, 3, dtype=dt), torch.zeros(128, 64, 3, 3, dtype=dt)
    WA[:32, :64 + M] = mw1
    WA[32:, :64 + M] = aw1
    WB[:64, :32] = mw2
    WB[64:, 32:] = aw2
    return WA, torch.cat([mb1, ab1]), WB, torch.cat([mb2, ab2])


def sft_split_ref(merged, M):
    """the reverse copy: the eight slices of (WA, bA, WB, bB) the parameters sit in"""
    WA, bA, WB, bB = merged
    return (WA[:32, :64 + M], bA[:32], WA[32:, :64 + M], bA[32:], WB[:64, :32], bB[:64], WB[64:, 32:], bB[64:])


def sft_structural(M):
    """bool maps of the structural zeros of WA and WB"""
    za, zb = torch.zeros(64, 128, 3, 3, dtype=torch.bool), torch.ones(128, 64, 3, 3, dtype=torch.bool)
    za[:, 64 + M:] = True
    zb[:64, :32] = zb[64:, 32:] = False
    return za, zb


# ----------------------------------------------------------------------------- SFT combine
def sft_combine_fwd_ref(x, y2, relu, A=False):
    """x [npix][64], y2 [npix][128] -> [relu](x sigmoid(y2[:, :64]) + y2[:, 64:]); A: |x| s + |a|.  Also pre and s."""
    x, y2 = _d(x), _d(y2)
    s, a = torch.sigmoid(y2[:, :64]), y2[:, 64:]
    if A:
        return dict(out=x.abs() * s + a.abs(), s=s)
    pre = x * s + a
    return dict(out=torch.relu(pre) if relu else pre, pre=pre, s=s)


def sft_combine_bwd_ref(dout, x, y2, relu, A=False, pre=None):
    """dx = g s, dm = g x s (1 - s), da = g with g = dout [pre > 0] under ReLU (0 at pre == 0, PyTorch's convention);
    A: (1 - s) -> (1 + s) on absolute values, the mask kept.  pre: the mask's argument if not the float64 x s + a"""
    dout, x, y2 = _d(dout), _d(x), _d(y2)
    s, a = torch.sigmoid(y2[:, :64]), y2[:, 64:]
    pre = x * s + a if pre is None else _d(pre)
    g = dout * (pre > 0) if relu else dout
    if A:
        g, x = g.abs(), x.abs()
        return dict(dx=g * s, dm=g * x * s * (1 + s), da=g)
    return dict(dx=g * s, dm=g * x * s * (1 - s), da=g)


# ----------------------------------------------------------------------------- strided 64-channel maps, clamp
def map64_ref(op, a, b=None):
    """sisr_map64's eight ops on [npix][64] float64 maps; b [npix][64], for op 7 [npix] (b's channel 0).  Ops 2 and 3 use
    the kernel's fp32 slope and its one rounding (tests/_exact.py leaky_ref / leaky_mask)"""
    a, b = _d(a), _d(b)
    if op == 0:
        return a.clone()
    if op == 1:
        return a + b
    if op == 2:
        return X.leaky_ref(a)
    if op == 3:
        return X.fp32_round(b * X.leaky_mask(a))
    if op == 4:
        return a * b
    if op == 5:
        return torch.relu(a)
    if op == 6:
        return b * X.relu_mask(a)
    if op == 7:
        return a * b.reshape(-1, 1)
    raise ValueError(op)


def clamp01_ref(a):
    return _d(a).clamp(0.0, 1.0)


def clamp01_bwd_ref(a, g):
    """g [0 <= a <= 1]: the gradient passes at exactly 0 and 1 (torch.clamp's convention)"""
    a = _d(a)
    return _d(g) * ((a >= 0) & (a <= 1))


# ----------------------------------------------------------------------------- layout kernels (csrc/misc.hip)
def nchw_to_nhwc_pad_ref(x, Cp):
    """(B, C, H, W) -> (B, H, W, Cp), channels >= C zero"""
    return F.pad(x.permute(0, 2, 3, 1), (0, Cp - x.shape[1])).contiguous()


def pad_oihw_ref(w, cop, cip):
    """(co, ci, taps) -> (cop, cip, taps), zero outside the real block"""
    out = torch.zeros((cop, cip, w.shape[2]), dtype=w.dtype)
    out[:w.shape[0], :w.shape[1]] = w
    return out


def crop_oihw_ref(wp, co, ci):
    return wp[:co, :ci].contiguous()


def shuffle_rgb_ref(y, C, r):
    """NHWC (B, H, W, Cp) -> NCHW (B, C, rH, rW): PixelShuffle(r) of the first C r^2 channels"""
    return F.pixel_shuffle(y[..., :C * r * r].permute(0, 3, 1, 2), r).contiguous()


def shuffle_rgb_adjoint_ref(g, C, r, Cp):
    """NCHW (B, C, rH, rW) -> NHWC (B, H, W, Cp): the adjoint, written as a gather; padded channels zero"""
    B, _, Hr, Wr = g.shape
    H, W = Hr // r, Wr // r
    t = g.reshape(B, C, H, r, W, r).permute(0, 2, 4, 1, 3, 5).reshape(B, H, W, C * r * r)
    return F.pad(t, (0, Cp - C * r * r)).contiguous()


def pixel_shuffle_cl_ref(x, C, r):
    """channels-last (B, H, W, C r^2) -> (B, rH, rW, C)"""
    return F.pixel_shuffle(x.permute(0, 3, 1, 2), r).permute(0, 2, 3, 1).contiguous()


def pixel_unshuffle_cl_ref(y, C, r):
    return F.pixel_unshuffle(y.permute(0, 3, 1, 2), r).permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------- fp32 -> bf16, round to nearest even
def f32_bits(x):
    return x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def bf16_bits(t):
    return t.contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def bf16_rne_ref(x):
    """fp32 tensor -> (the 16-bit pattern of its round-to-nearest-even bf16 in integer arithmetic, NaN map).  Adding
    0x7FFF + (bit 16) carries into the exponent by itself: the largest finite values round to infinity, infinities stay.  At
    a NaN the pattern returned is the quieted upper half; only sign and NaN-ness are defined there."""
    b = f32_bits(x)
    isnan = (b & 0x7FFFFFFF) > 0x7F800000
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF
    return torch.where(isnan, (b >> 16) | 0x40, r), isnan


def bf16_is_nan(bits):
    return (bits & 0x7FFF) > 0x7F80


def bf16_patterns():
    """every upper half 0 .. 65535, each with the lower halves {0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF}: exact values, just
    below / at / just above a tie (to even both ways, as the upper half's last bit takes both values), the carry into the
    exponent and into infinity, +-0, subnormals, +-inf and NaNs"""
    hi = torch.arange(65536, dtype=torch.int64)[:, None] << 16
    lo = torch.tensor([0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64)[None, :]
    b = (hi | lo).reshape(-1)
    b = torch.where(b >= 2 ** 31, b - 2 ** 32, b)
    return b.to(torch.int32).view(torch.float32)


# ----------------------------------------------------------------------------- blur / noise quantisers (csrc/degrade.hip)
def blur_ref(x, k):
    """x (C, H, W), k (l, l) -> reflection pad (l // 2 before, l - 1 - l // 2 after) and cross-correlation, float64, as l l
    shifted products"""
    x, k = _d(x), _d(k)
    l = k.shape[-1]
    H, W = x.shape[-2:]
    lo, hi = l // 2, l - 1 - l // 2
    p = F.pad(x[None], (lo, hi, lo, hi), mode="reflect")[0] if l > 1 else x
    y = torch.zeros_like(x)
    for i in range(l):
        for j in range(l):
            if float(k[i, j]) != 0.0:
                y = y + p[:, i:i + H, j:j + W] * k[i, j]
    return y


def blur_mag(x, k):
    return blur_ref(_d(x).abs(), _d(k).abs())


def quant_ref(v32):
    """ToPILImage's byte of an fp32 value in [0, 1], as fp32 evaluates it: byte(int(fl32(v * 255))) (v 255 is exact in
    float64: one rounding)"""
    return X.fp32_round(_d(v32) * 255.0).to(torch.int64).to(torch.uint8)


def noise_quant_ref(blur, noise, sigma32):
    """byte(int(fl32(255 clamp(fl32(fl32(noise sigma) + blur), 0, 1)))): product and sum rounded separately, as the
    kernel's comment states.  The product of two fp32 values is exact in float64; the sum of two fp32 values is rounded
    by fp32's own addition on the host (IEEE), which no double rounding can touch."""
    prod = X.fp32_round(_d(noise) * sigma32).float()
    v = (prod + blur.detach().float()).double().clamp(0.0, 1.0)
    return quant_ref(v), v
