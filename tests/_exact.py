"""Exact-data testing of the conv and weight-gradient kernels (helper module, not collected; torch only, no HIP import).

Every operand is a small dyadic rational (integers in {-2..2} or {-1, 0, 1}, weights k/8, biases k/8, scales in
{0.5, 1, 1.5, 2}, shifts k/4): all are exact in bf16 (8 significant bits), every product is exact in fp32, and as long as
every partial sum of a contraction fits fp32's 24-bit significand, EVERY correct kernel form -- any summation order,
tiling, K-split, fp32 or bf16 MFMA -- returns the exact result.  The float64 references below then equal the kernels'
outputs bit for bit.  `assert_budget` checks the "fits" part before each exact comparison: it evaluates the same
contraction on absolute values, in units of the granule (the largest power of two every term is a multiple of), and
requires < 2**22; the two spare bits cover fused epilogue sums (bias, residual, GATE's t*g + skip, GAP / DOT partials)
and any internal alignment of the bf16 MFMA.  A case over budget is a bug of the test, and is reported as one.

References are nine (k*k) shifted float64 matmuls per conv -- einsum over channels per tap -- so they run on the device at
production size; integer-valued float64 sums are exact there too.
"""
import math

import torch
import torch.nn.functional as F

BUDGET_BITS = 22
ALPHA = 0.5
SLOPE32 = 0.20000000298023224  # float32(0.2): the LeakyReLU slope constant the fp32 kernels multiply by (0.2f)


# ----------------------------------------------------------------------------- seeded generators of exact data
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def ints(shape, seed, lo=-2, hi=2, zeros=None):
    """integers uniform in [lo, hi] (float32, CPU); zeros: share of entries additionally forced to exactly 0"""
    g = _gen(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).float()
    if zeros:
        t[torch.rand(tuple(shape), generator=g) < zeros] = 0.0
    return t


def nonzero_ints(shape, seed, m=2):
    """integers in {-m..-1, 1..m}: data in which every single term of a contraction shows"""
    g = _gen(seed)
    mag = torch.randint(1, m + 1, tuple(shape), generator=g).float()
    sign = torch.randint(0, 2, tuple(shape), generator=g).float() * 2 - 1
    return mag * sign


def weights(shape, seed, kmax=4, nonzero=False):
    """k / 8, |k| <= kmax (nonzero: k != 0)"""
    k = nonzero_ints(shape, seed, kmax) if nonzero else ints(shape, seed, -kmax, kmax)
    return k / 8


def biases(n, seed):
    return ints((n,), seed, -8, 8) / 8


def scales(shape, seed):
    """in_scale / dy_scale / gate values in {0.5, 1, 1.5, 2}"""
    return ints(shape, seed, 1, 4) / 2


def shifts(shape, seed):
    """in_shift / dy_shift values k / 4, |k| <= 4"""
    return ints(shape, seed, -4, 4) / 4


# ----------------------------------------------------------------------------- budget
def granule(*ts):
    """largest power of two (<= 1) that every entry of every tensor is an integer multiple of"""
    g = 1.0
    for t in ts:
        if t is None:
            continue
        t = t.detach().double()
        for e in range(0, 41):
            s = t * float(2 ** e)
            if torch.equal(s, torch.round(s)):
                g = min(g, 2.0 ** -e)
                break
        else:
            raise AssertionError("test bug: operand is not a dyadic rational with <= 40 fraction bits")
    return g


def budget_bits(mag, gran):
    """log2 of the largest |partial sum| of the contraction (mag: the contraction on absolute values) in granules"""
    m = float(mag.detach().max()) if torch.is_tensor(mag) else float(mag)
    return math.log2(max(m / gran, 1.0))


def assert_budget(mag, gran, what=""):
    bits = budget_bits(mag, gran)
    assert bits < BUDGET_BITS, (f"TEST BUG (not a kernel failure): {what} needs {bits:.2f} bits of significand, the exact-data "
                                f"budget is {BUDGET_BITS}; choose smaller / sparser data for this case")
    return bits


def conv_budget(x, w, extras=(), padding=1, what="conv"):
    """budget of y = conv(x, w) [+ extras]: the conv on |x|, |w| plus |extra| terms, in units of the finest granule"""
    mag = conv_ref(x.double().abs(), w.double().abs(), padding=padding)
    gran = granule(x) * granule(w)
    for e in extras:
        if e is None:
            continue
        e = e.to(mag.device).double().abs()
        mag = mag + (e.view(1, -1, 1, 1) if e.dim() == 1 else e)
        gran = min(gran, granule(e))
    return assert_budget(mag, gran, what)


def wgrad_budget(x, dy, padding=1, k=3, what="weight gradient"):
    """budget of dw = sum_pixels x (x) dy (and of db = sum dy)"""
    mag = wgrad_ref(x.double().abs(), dy.double().abs(), padding=padding, k=k)
    gran = granule(x) * granule(dy)
    bits = assert_budget(mag, gran, what)
    return max(bits, assert_budget(dy.double().abs().sum(dim=(0, 2, 3)), granule(dy), what + " (bias)"))


def winograd_budget(u, w, what="Winograd conv"):
    """F(2x2,3x3) on u (the conv's input after any prologue) and w: |V| <= 4 max|u| (B^T d B), |U| <= 9/4 max|w| on the
    granule gw/4 (G g G^T), M sums cin products, the output transform sums <= 9 of them."""
    cin = w.shape[1]
    mag = 9 * cin * 4 * float(u.abs().max()) * 2.25 * float(w.abs().max())
    return assert_budget(mag, granule(u) * granule(w) / 4, what)


# ----------------------------------------------------------------------------- float64 references (shifted matmuls)
def conv_ref(x, w, bias=None, padding=None, stride=1):
    """cross-correlation of x (B, C, H, W) with w (O, C, k, k), zero padding `padding` (default k // 2), as k*k shifted
    einsums over channels in float64.  Differentiable (autograd gives the input / weight gradient references too)."""
    x, w = x.double(), w.double()
    k = w.shape[-1]
    p = k // 2 if padding is None else padding
    xp = F.pad(x, (p, p, p, p)) if p else x
    Ho, Wo = xp.shape[2] - k + 1, xp.shape[3] - k + 1
    y = None
    for ky in range(k):
        for kx in range(k):
            t = torch.einsum("bchw,oc->bohw", xp[:, :, ky:ky + Ho, kx:kx + Wo], w[:, :, ky, kx])
            y = t if y is None else y + t
    if stride > 1:
        y = y[:, :, ::stride, ::stride]
    if bias is not None:
        y = y + bias.double().view(1, -1, 1, 1)
    return y


def dgrad_ref(dy, w):
    """input gradient of the zero-padded stride-1 conv: the conv of dy with the flipped, role-swapped weight"""
    k = w.shape[-1]
    return conv_ref(dy, w.double().flip(2, 3).transpose(0, 1), padding=k // 2)


def wgrad_ref(x, dy, padding=1, k=3):
    """dw[o, c, ky, kx] = sum_{b, h, w} dy[b, o, h, w] x_pad[b, c, h + ky, w + kx] (stride 1)"""
    x, dy = x.double(), dy.double()
    xp = F.pad(x, (padding,) * 4) if padding else x
    H, W = dy.shape[2], dy.shape[3]
    taps = [torch.einsum("bohw,bchw->oc", dy, xp[:, :, ky:ky + H, kx:kx + W]) for ky in range(k) for kx in range(k)]
    return torch.stack(taps, dim=-1).view(dy.shape[1], x.shape[1], k, k)


def geo_input(x, up=1):
    """SPARNet ConvLayer staging: [nearest x up] -> ReflectionPad2d(1), float64"""
    x = x.double()
    if up > 1:
        x = x.repeat_interleave(up, dim=2).repeat_interleave(up, dim=3)
    return F.pad(x, (1, 1, 1, 1), mode="reflect")


def geo_conv_ref(x, w, bias=None, up=1, stride=1):
    """Conv2d(3x3, stride, no padding)(ReflectionPad2d(1)(nearest_up(x)))"""
    return conv_ref(geo_input(x, up), w, bias, padding=0, stride=stride)


def relu_mask(m):
    """PyTorch's ReLU backward convention, taken from its own float64 autograd: grad * (m > 0)"""
    m = m.detach().double().requires_grad_(True)
    (g,) = torch.autograd.grad(F.relu(m), m, torch.ones_like(m))
    return g


def leaky_mask(m, slope=SLOPE32):
    """PyTorch's LeakyReLU backward convention, from its own float64 autograd: 1 where m > 0, `slope` where m <= 0"""
    m = m.detach().double().requires_grad_(True)
    (g,) = torch.autograd.grad(F.leaky_relu(m, slope), m, torch.ones_like(m))
    return g


def fp32_round(t):
    """single round-to-nearest-even of float64 values to fp32 (returned as float64)"""
    return t.float().double()


def leaky_ref(v):
    """LeakyReLU(0.2) as the fp32 kernels compute it on an exact fp32 value v: v > 0 ? v : fl32(0.2f * v).  v * 0.2f is
    exact in float64 (24 + 24 significant bits), so this is ONE rounding -- the kernel's own."""
    return torch.where(v > 0, v, fp32_round(v * SLOPE32))


# ----------------------------------------------------------------------------- comparisons
def mismatch(got, ref):
    """bool map of the elements where the kernel's output differs from the exact value (NaN -- unwritten -- differs)"""
    return got.detach().double() != ref.to(got.device)


def assert_exact(got, ref, what=""):
    ref = ref.to(got.device)
    if torch.equal(got.detach().double(), ref):
        return
    bad = mismatch(got, ref)
    idx = bad.nonzero()[:5].tolist()
    vals = [(float(got.detach().double()[tuple(i)]), float(ref[tuple(i)])) for i in idx]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact float64 value; "
                         f"first at {idx}: (got, exact) = {vals}")


def bf16_of(exact):
    """what a bf16-stored output of an exact (fp32-representable) value must hold: its single round-to-nearest-even"""
    return exact.float().to(torch.bfloat16)
