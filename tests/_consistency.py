"""Shared by the degradation-consistency tests: the float64 twin of the operator, the stock-torch composition that serves as
the fp32 yardstick, inputs and cases.

The twin is the degradation as the pipeline performs it, step by step, in torch float64 on the host: the blur as BatchBlur's
cross-correlation without its reflection padding (so only where the l x l window lies inside the tile), then the horizontal
tap pass, then the vertical one, each output with the row that precompute_coeffs (libImaging/Resample.c) gives it in the table
of the WHOLE tile -- the weights w / ww before the fixed-point rounding, computed here from the formula, not taken from
degrade.bicubic_interior_taps or from a composed kernel.  Every step is a torch operation, so autograd gives the adjoint."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from sisr_amd import degrade


def float_row(in_size, out_size, xx):
    """Row xx of precompute_coeffs for a full-extent box: -> (first input index, float64 weights w / ww), clipped at the image
    ends exactly as Pillow clips it."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    center = (xx + 0.5) * scale
    xmin = max(int(center - support + 0.5), 0)
    xmax = min(int(center + support + 0.5), in_size) - xmin
    w = [degrade._bicubic_filter((x + xmin - center + 0.5) * ss) for x in range(xmax)]
    ww = 0.0
    for v in w:
        ww += v
    return xmin, np.array([v / ww for v in w], np.float64)


def margin(scale, l):
    """the kept outputs by the definition: output i of an h-row tile is kept when its unclipped taps, widened by the blur radius,
    lie inside the tile; found by search on a 64-row tile, the same at both sides"""
    h, pl = 64, l // 2
    keep = []
    for i in range(h):
        center, support = (i + 0.5) * scale, 2.0 * scale
        lo, hi = math.floor(center - support + 0.5), math.floor(center + support + 0.5)  # unclipped (int() rounds towards 0)
        while degrade._bicubic_filter((hi - 1 - center + 0.5) / scale) == 0.0:
            hi -= 1
        if lo - pl >= 0 and hi - 1 + pl <= scale * h - 1:
            keep.append(i)
    assert keep == list(range(keep[0], h - keep[0]))
    return keep[0]


def pass_matrix(in_size, out_size, m, shift):
    """(out_size - 2m, in_size - 2 shift) float64: rows m .. out_size - m - 1 of the tile's table as a matrix over the blurred
    samples shift .. in_size - shift - 1 (the ones whose blur window lies inside the tile)"""
    R = np.zeros((out_size - 2 * m, in_size - 2 * shift), np.float64)
    for i in range(m, out_size - m):
        lo, w = float_row(in_size, out_size, i)
        for a, v in enumerate(w):
            if v != 0.0:  # (at s = 3 the row ends in a tap of weight 0, which may lie past the last blurred sample)
                assert 0 <= lo + a - shift < R.shape[1], (i, lo, a)
                R[i - m, lo + a - shift] = v
    return torch.from_numpy(R)


def twin(x, kernels, scale):
    """x (B, C, s h, s w), kernels (B, l, l), both float64 on the host -> (B, C, h - 2m, w - 2m) float64"""
    assert x.dtype == torch.float64 and kernels.dtype == torch.float64 and not x.is_cuda
    B, C, H, W = x.shape
    l = kernels.shape[-1]
    h, w = H // scale, W // scale
    m = margin(scale, l)
    blurred = F.conv2d(x.reshape(1, B * C, H, W), kernels.repeat_interleave(C, 0)[:, None], groups=B * C)  # cross-correlation
    blurred = blurred.reshape(B, C, H - l + 1, W - l + 1)       # blurred[p, q] of the pipeline at [p - l // 2, q - l // 2]
    across = blurred @ pass_matrix(W, w, m, l // 2).T           # horizontal pass
    return pass_matrix(H, h, m, l // 2) @ across                # vertical pass


def stock(x, kernels, scale):
    """The same three steps as stock torch would run them in x's dtype on x's device: a per-sample grouped conv2d, then the two
    tap passes as strided convolutions -- the fp32 yardstick of the GPU tests, and what tools/consistency_bench.py times."""
    B, C, H, W = x.shape
    l = kernels.shape[-1]
    first, taps = degrade.bicubic_interior_taps(scale)
    m = degrade.consistency_margin(scale, l)
    off = scale * m + first - l // 2
    ho, wo = H // scale - 2 * m, W // scale - 2 * m
    t = torch.as_tensor(taps).to(x)
    k = kernels.to(x).repeat_interleave(C, 0)[:, None]
    b = F.conv2d(x.reshape(1, B * C, H, W), k, groups=B * C).reshape(B * C, 1, H - l + 1, W - l + 1)
    b = b[:, :, :, off:off + scale * (wo - 1) + len(taps)]
    b = F.conv2d(b, t.reshape(1, 1, 1, -1), stride=(1, scale))
    b = b[:, :, off:off + scale * (ho - 1) + len(taps)]
    return F.conv2d(b, t.reshape(1, 1, -1, 1), stride=(scale, 1)).reshape(B, C, ho, wo)


def strided_correlation(x, K, scale, first, m):
    """D_k(x) at the kept outputs from a composed kernel K (B, n, n), by the definition, in x's dtype"""
    B, C, H, W = x.shape
    n = K.shape[-1]
    off = scale * m + first
    ho, wo = H // scale - 2 * m, W // scale - 2 * m
    xs = x[:, :, off:off + scale * (ho - 1) + n, off:off + scale * (wo - 1) + n]
    return F.conv2d(xs.reshape(1, B * C, xs.shape[2], xs.shape[3]), K.to(x).repeat_interleave(C, 0)[:, None], stride=scale,
                    groups=B * C).reshape(B, C, ho, wo)


def augment(img, flips):
    """data.random_flip_rotate's transform of a (..., H, W) image for (hflip, vflip, transpose)"""
    hf, vf, tr = flips
    if hf:
        img = torch.flip(img, [-1])
    if vf:
        img = torch.flip(img, [-2])
    if tr:
        img = img.transpose(-1, -2)
    return img


def kernels(B, l, seed):
    """B different anisotropic Gaussian kernels (l, l), float64, rotated and skewed by a linear ramp (a Gaussian alone is its own
    point reflection) so that no flip, transpose or combination of them leaves one unchanged; they sum to 1.  l = 1: [[1]]"""
    if l == 1:
        return torch.ones(B, 1, 1, dtype=torch.float64)
    rng = np.random.RandomState(seed)
    out = []
    for b in range(B):
        sx, sy = 0.6 + 0.35 * l / 7 * (1 + rng.rand()), 0.3 + 0.1 * l / 7 * (1 + rng.rand())
        k = degrade.anisotropic_gaussian_kernel(l, degrade.cal_sigma(sx, sy, 0.4 + 0.5 * b + 0.2 * rng.rand()))
        ramp = 1.0 + 0.5 * np.arange(-(l // 2), l // 2 + 1) / l
        k = k * ramp[None, :] * (ramp ** 2)[:, None]
        out.append(k / k.sum())
    return torch.from_numpy(np.stack(out))


def image(B, C, H, W, seed):
    return torch.rand(B, C, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def max_abs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def abs_tap_sum(scale):
    """A: the absolute tap sum of an interior row, from the fixed-point table itself"""
    _, coef, _ = degrade.pil_bicubic_table(64 * scale, 64)
    return float(np.abs(coef[8].astype(np.float64)).sum() / 2.0 ** degrade.PRECISION_BITS)
