"""Frequency-domain (FFT L1) loss testing (helper module, not collected; torch only, no HIP import).

The quantity: for (B, C, H, W) operands, d = sr - y, F = rfft2(d, norm='ortho'), value = mean of |Re F| and |Im F| over all
2 * B * C * H * (W // 2 + 1) entries, the structurally zero imaginary parts counted.  `spectral_l1` states it through the
cosine / sine tables the kernels use, in the operands' dtype: in float64 on the host it is the oracle, in fp32 on the device
(tables rounded to fp32 first, torch.matmul) the stock yardstick -- the same function over the same fp32 tables as the
kernels, differing only in summation order.  Beside it the analytic gradient the kernels implement, the criterion
restatement and the input makers.
"""
import functools
import math

import torch

import _ssim_loss as SS


def tables(n, half, dtype=torch.float64, device="cpu"):
    """C[k, j] = cos(2 pi r / n), S[k, j] = sin(2 pi r / n) for k < half, j < n, with r = k j mod n taken in integers;
    evaluated in float64, exactly 0 / +-1 at quarter turns, then rounded once to `dtype`"""
    k = torch.arange(half, dtype=torch.int64)[:, None]
    j = torch.arange(n, dtype=torch.int64)[None, :]
    r = (k * j) % n
    a = 2.0 * math.pi * r.double() / n
    c, s = torch.cos(a), torch.sin(a)
    quarter = (4 * r) % n == 0
    q = (4 * r) // n
    exact_c = torch.tensor([1.0, 0.0, -1.0, 0.0], dtype=torch.float64)[q % 4]
    exact_s = torch.tensor([0.0, 1.0, 0.0, -1.0], dtype=torch.float64)[q % 4]
    c = torch.where(quarter, exact_c, c)
    s = torch.where(quarter, exact_s, s)
    return c.to(device=device, dtype=dtype), s.to(device=device, dtype=dtype)


def spectrum(sr, y):
    """(Re F, Im F) of F = rfft2(sr - y, norm='ortho') through the tables, in the operands' dtype, each (B, C, H, W // 2 + 1):
    Tr = d Cw^T, Ti = -d Sw^T, Fr = Ch Tr + Sh Ti, Fi = Ch Ti - Sh Tr, both times (HW)^-1/2"""
    H, W = sr.shape[2:]
    cw, sw = tables(W, W // 2 + 1, sr.dtype, sr.device)
    ch, sh = tables(H, H, sr.dtype, sr.device)
    d = sr - y
    tr = torch.matmul(d, cw.t())
    ti = -torch.matmul(d, sw.t())
    scale = 1.0 / math.sqrt(H * W)
    fr = (torch.matmul(ch, tr) + torch.matmul(sh, ti)) * scale
    fi = (torch.matmul(ch, ti) - torch.matmul(sh, tr)) * scale
    return fr, fi


def spectral_l1(sr, y):
    """the oracle (float64) / the stock yardstick (fp32 on the device): (sum |Re F| + sum |Im F|) / n"""
    fr, fi = spectrum(sr, y)
    return (fr.abs().sum() + fi.abs().sum()) / (2 * fr.numel())


def fft_l1(sr, y):
    """the definition: the mean of view_as_real(rfft2(sr - y, norm='ortho')).abs()"""
    return torch.view_as_real(torch.fft.rfft2(sr - y, norm="ortho")).abs().mean()


def structural_mask(H, W):
    """(H, W // 2 + 1) bool: the bins whose imaginary part is zero by structure"""
    m = torch.zeros(H, W // 2 + 1, dtype=torch.bool)
    us = [0] + ([H // 2] if H % 2 == 0 else [])
    vs = [0] + ([W // 2] if W % 2 == 0 else [])
    for u in us:
        for v in vs:
            m[u, v] = True
    return m


def analytic_grad(sr, y):
    """d spectral_l1 / d sr by the formula the kernels implement, with s_r = sign(Fr), s_i = sign(Fi):
         [(Ch s_r - Sh s_i) Cw - (Sh s_r + Ch s_i) Sw] / (n sqrt(HW))"""
    H, W = sr.shape[2:]
    cw, sw = tables(W, W // 2 + 1, sr.dtype, sr.device)
    ch, sh = tables(H, H, sr.dtype, sr.device)
    fr, fi = spectrum(sr, y)
    s_r, s_i = torch.sign(fr), torch.sign(fi)
    gr = torch.matmul(ch, s_r) - torch.matmul(sh, s_i)
    gi = torch.matmul(sh, s_r) + torch.matmul(ch, s_i)
    return (torch.matmul(gr, cw) - torch.matmul(gi, sw)) / (2 * fr.numel() * math.sqrt(H * W))


def autograd_grad(sr, y, fn=spectral_l1, scale=1.0):
    """(value, d (scale * value) / d sr) of `fn` by autograd, in sr's dtype"""
    sr = sr.detach().clone().requires_grad_(True)
    v = fn(sr, y)
    (g,) = torch.autograd.grad(scale * v, sr)
    return v.detach(), g


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm())


def criterion(sr, y, base, alpha, beta):
    """base(sr, y) + alpha * (1 - SSIM(sr, y)) + beta * spectral_l1(sr, y) in sr's dtype; base: 'l1' or 'mse'"""
    pix = (sr - y).abs().mean() if base == "l1" else ((sr - y) ** 2).mean()
    if alpha:
        pix = pix + alpha * (1 - SS.ssim_mean(sr, y))
    return pix + beta * spectral_l1(sr, y)


# the smallest shapes at which the tiling (64 x 64 bins or pixels per workgroup, 32 x 32 per wave, K in steps of 32) can go wrong
SHAPES = [(2, 3, 2, 2),      # K = 2, every imaginary part structural
          (2, 3, 8, 8),      # even x even, smaller than one MFMA tile, Nyquist row and column
          (1, 1, 11, 85),    # odd x odd, short beside long, Wh = 43
          (2, 1, 32, 64),    # exact tile multiples, Wh = 33
          (1, 1, 33, 65),    # one past the K step and the wave tile in both stages, Wh = 33
          (1, 3, 43, 75),    # ragged everywhere
          (1, 1, 65, 63),    # H one past the workgroup tile, Wh = 32 exactly
          (1, 2, 66, 34),    # H > W, two tiles + 2
          (1, 1, 128, 128)]  # the smallest real tile size, multi-step K loops, Wh = 65: one past the workgroup tile
NEAR = (1, 3, 43, 75)
CASES = [(s, 0.05) for s in SHAPES] + [(NEAR, 0.002)]
KINK = 2e-5  # times the noise: the least |Re F|, |Im F| of a non-structural bin (the fp32 coefficient error is ~1e-7 x noise)


def kink_margin(sr, y):
    """the least |Re F|, |Im F| over the non-structural entries, in float64"""
    fr, fi = spectrum(sr.double(), y.double())
    m = structural_mask(*sr.shape[2:])
    return min(float(fr.abs().min()), float(fi.abs()[..., ~m].min()) if not bool(m.all()) else math.inf)


@functools.lru_cache(maxsize=None)
def make_pair(shape, noise):
    """y = rand, sr = y + noise * randn, unclamped, fp32 on the host, seeded from 2000 + prod(shape): the first seed (at most
    50 tried) for which every non-structural |Re F|, |Im F| is at least KINK * noise.  Returns (sr, y, margin); the
    tensors are shared between tests and must not be modified."""
    for k in range(50):
        g = torch.Generator().manual_seed(2000 + math.prod(shape) + k)
        y = torch.rand(shape, generator=g)
        sr = y + noise * torch.randn(shape, generator=g)
        margin = kink_margin(sr, y)
        if margin >= KINK * noise:
            return sr, y, margin
    raise AssertionError(f"no kink-free input for {shape} at noise {noise} in 50 seeds")


@functools.lru_cache(maxsize=None)
def kink_free_pair(shape, seed=300):
    """sr = y + n with 0.01 <= |n| <= 0.05 (every pixel difference away from L1's kink) and every non-structural spectral
    coefficient at least 1e-6 (KINK * 0.05) in magnitude; the first such seed from `seed` on"""
    for k in range(50):
        sr, y = SS.kink_free_pair(shape, seed=seed + k)
        if kink_margin(sr, y) >= KINK * 0.05:
            return sr, y
    raise AssertionError(f"no kink-free input for {shape} in 50 seeds")
