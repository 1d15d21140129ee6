"""Geometric self-ensemble for evaluation: the "+" rows (EDSR+, RCAN+ ...) of the EDSR / RCAN / HAN / SAN papers.

The network runs on the eight flips and transposes of its input, every output is mapped back and the eight are averaged.
The eight variants of an h x w image are four of shape h x w and four of shape w x h, so the whole ensemble of a batch of n
is two forwards at batch 4n, one launch that makes the variants (`dihedral_fan`) and one that folds the outputs back
(`dihedral_merge`); csrc/ensemble.hip, DESIGN.md 6m.

Layout (contiguous NCHW fp32, variant-major: image i of variant k is entry k * n + i):
    upright (4n, c, h, w)   k = 0..3: x, x.flip(-1), x.flip(-2), x.flip(-2, -1)
    turned  (4n, c, w, h)   k = 0..3: the same four operations applied to x.transpose(-1, -2)
    merge   (((u0 + u1) + (u2 + u3)) + ((t0 + t1) + (t2 + t3))) * 0.125 with every variant mapped back, fp32 adds in this order

Tensors on a HIP device go through the kernels; CPU tensors through the host form below, written with torch.flip /
transpose in the same variant order and the same summation order.  The host form is the specification the kernels are
tested against, bit for bit.  Evaluation only: there is no backward.
"""
import torch

from . import hip


def _four(t):
    """t and its three flips, in variant order"""
    return [t, t.flip(-1), t.flip(-2), t.flip(-2, -1)]


def _checked(t, what):
    if t.dim() != 4 or t.dtype != torch.float32:
        raise ValueError(f"{what} takes (N, C, H, W) fp32 batches; got {tuple(t.shape)} {t.dtype}")
    if t.requires_grad:
        raise RuntimeError(f"{what} is an evaluation operator without a backward; got a tensor that requires grad")
    if 0 in t.shape:
        raise ValueError(f"{what}: empty batch {tuple(t.shape)}")
    return t.contiguous()


def dihedral_fan(x):
    """x (n, c, h, w) -> (upright (4n, c, h, w), turned (4n, c, w, h)): a pure copy of every element."""
    x = _checked(x, "dihedral_fan")
    n, c, h, w = x.shape
    if not x.is_cuda:
        return torch.cat(_four(x)).contiguous(), torch.cat(_four(x.transpose(-1, -2))).contiguous()
    upright, turned = x.new_empty((4 * n, c, h, w)), x.new_empty((4 * n, c, w, h))
    with torch.cuda.device(x.device):
        hip.check(hip.lib().sisr_dihedral_fan(hip.ptr(x), n, c, h, w, hip.ptr(upright), hip.ptr(turned), hip.stream()),
                  "sisr_dihedral_fan")
    return upright, turned


def dihedral_merge(upright, turned):
    """upright (4n, c, H, W), turned (4n, c, W, H) -> (n, c, H, W): every variant mapped back, the eight averaged."""
    upright, turned = _checked(upright, "dihedral_merge"), _checked(turned, "dihedral_merge")
    m, c, H, W = upright.shape
    if m % 4 or tuple(turned.shape) != (m, c, W, H) or turned.device != upright.device:
        raise ValueError(f"dihedral_merge takes (4n, c, H, W) and (4n, c, W, H) on one device; got {tuple(upright.shape)} on "
                         f"{upright.device} and {tuple(turned.shape)} on {turned.device}")
    n = m // 4
    if not upright.is_cuda:
        # a flip is its own inverse; the transposed variants are flipped back first, then transposed back
        u = [a.flip(*d) if d else a for a, d in zip(upright.view(4, n, c, H, W), ((), (-1,), (-2,), (-2, -1)))]
        t = [(a.flip(*d) if d else a).transpose(-1, -2)
             for a, d in zip(turned.view(4, n, c, W, H), ((), (-1,), (-2,), (-2, -1)))]
        return ((((u[0] + u[1]) + (u[2] + u[3])) + ((t[0] + t[1]) + (t[2] + t[3]))) * 0.125).contiguous()
    out = upright.new_empty((n, c, H, W))
    with torch.cuda.device(upright.device):
        hip.check(hip.lib().sisr_dihedral_merge(hip.ptr(upright), hip.ptr(turned), n, c, H, W, hip.ptr(out), hip.stream()),
                  "sisr_dihedral_merge")
    return out


def fan_extra_channels(extra_channels, x):
    """The metadata that accompanies `x`, for the two passes of the ensemble -> (for upright, for turned).
    (B, M, 1, 1) vectors (the meta-attention inputs) are repeated four times along the batch, variant-major; maps of x's
    spatial size (SFTMD / SRMD) go through dihedral_fan like the image; None stays None.  The VALUES are handed on as they
    are: a degradation code describes the un-flipped image, which is exact for isotropic blur codes and for QPI and the
    usual caveat of the protocol for anisotropic kernels (a flipped image was blurred by the flipped kernel)."""
    if extra_channels is None:
        return None, None
    e = extra_channels
    if e.dim() == 4 and e.shape[0] == x.shape[0] and tuple(e.shape[2:]) == (1, 1):
        rep = e.repeat(4, 1, 1, 1)
        return rep, rep
    if e.dim() == 4 and e.shape[0] == x.shape[0] and tuple(e.shape[2:]) == tuple(x.shape[2:]):
        return dihedral_fan(e.to(device=x.device, dtype=torch.float32))
    raise NotImplementedError(f"self-ensemble: metadata of shape {tuple(e.shape)} beside an input of shape {tuple(x.shape)} "
                              f"(supported: (B, M, 1, 1) vectors and maps of the input's spatial size)")


def self_ensemble(forward, x, extra_channels=None):
    """forward(batch, extra) applied to the eight variants of `x` as two batches of 4n, and the mean of its outputs mapped
    back.  `forward` is whatever the handler would have run on `x` itself (run_model; forward_chop around the network for
    the chopped SAN path); the output geometry is read from what it returns, (H, W) for the upright pass and (W, H) for
    the turned one."""
    upright, turned = dihedral_fan(x)
    e_up, e_tu = fan_extra_channels(extra_channels, x)
    return dihedral_merge(forward(upright, e_up), forward(turned, e_tu))
