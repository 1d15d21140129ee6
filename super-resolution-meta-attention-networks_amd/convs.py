"""The stride-2 K x K convolution and the pointwise (1 x 1) layer of up to 128 channels with a per-image bias, both ways
(csrc/basic.hip: sisr_convk_s2_*, sisr_dgradk_s2_*, sisr_wgradk_s2_*, sisr_conv1_*, sisr_wgrad1_*): the layers IKC's predictor
and corrector add to the stride-1 K x K conv of ops.py.  ops.conv_kxk(stride=2) and ops.conv_1x1 are this module's operators.
Both follow the weight-gradient buffer contract of the neighbouring nodes (ops._grad_buf: frozen inputs, kept and shared
gradients, GRAD_SINK) and capture into a hipGraph: workspaces from hip.workspace, no host synchronisation."""
import math

import torch
from torch.autograd import Function

from . import hip, ops


def conv_s2_out_size(n):
    """output size of a stride-2 K x K conv with padding K // 2 (K odd) along an axis of n pixels"""
    return hip.lib().sisr_convk_s2_out_size(int(n))


class _ConvKxKS2(Function):
    """nn.Conv2d(K, stride=2, padding=K // 2) + bias (+ LeakyReLU(slope); slope None: no activation) between channels-last
    maps on the fp32 matrix cores.  Backward: the input gradient is the polyphase transposed conv on the 'dgrad' packing, the
    weight gradient the stride-1 kernel with a strided x index; both read dy through the saved output."""

    @staticmethod
    def forward(ctx, x, weight, bias, slope):
        ops._fp32_only("conv_kxk")
        B, cip, H, W = x.shape
        co, ci = weight.shape[0], weight.shape[1]
        K, cop = ops._check_k(weight), ops._pad_width(co)
        x = ops._check_map(x, "conv_kxk")
        if ops._pad_width(ci) != cip:
            raise RuntimeError(f"conv_kxk: weight takes {ci} channels, the map has {cip}")
        pf, pd = ops.pack_convk(weight, need_dgrad=ctx.needs_input_grad[0])
        y = ops._empty_cl(B, cop, conv_s2_out_size(H), conv_s2_out_size(W), x.device)
        hip.check(hip.lib().sisr_convk_s2_mfma_leaky(hip.ptr(x), hip.ptr(pf), hip.ptr(bias), co if bias is not None else 0,
                                                     hip.ptr(y), B, H, W, K, cip, cop, int(slope is not None),
                                                     float(slope or 0.0), hip.stream()), "sisr_convk_s2_mfma_leaky")
        ctx.save_for_backward(x, y if slope is not None else None, weight, pd)
        ctx.cfg = (B, H, W, K, co, ci, cop, cip)
        ctx.bias, ctx.slope = bias, float(slope or 0.0)
        return y

    @staticmethod
    def backward(ctx, dy):
        ops.IN_BACKWARD = True
        try:
            x, y, weight, pd = ctx.saved_tensors
            B, H, W, K, co, ci, cop, cip = ctx.cfg
            dy = ops._cl(dy)
            L = hip.lib()
            dx = dw = db = None
            want_db = ctx.bias is not None and ctx.needs_input_grad[2]
            if ctx.needs_input_grad[1] or want_db:  # one call makes both; a frozen weight's gradient is dropped
                dwb = ops._grad_buf(weight) if ctx.needs_input_grad[1] else torch.empty_like(weight)
                db = ops._grad_buf(ctx.bias) if want_db else None
                nb = L.sisr_wgradk_s2_mfma_workspace_bytes(B, H, W, K, cip, cop)
                ws = hip.workspace(dy.device, nb)
                hip.check(L.sisr_wgradk_s2_mfma_leaky(hip.ptr(x), hip.ptr(dy), hip.ptr(y), hip.ptr(dwb), hip.ptr(db), B, H, W, K,
                                                      co, ci, cop, cip, hip.ptr(ws), nb, ctx.slope, hip.stream()),
                          "sisr_wgradk_s2_mfma_leaky")
                dw = dwb if ctx.needs_input_grad[1] else None
            if ctx.needs_input_grad[0]:
                dx = ops._empty_cl(B, cip, H, W, dy.device)
                hip.check(L.sisr_dgradk_s2_mfma_leaky(hip.ptr(dy), hip.ptr(y), hip.ptr(pd), hip.ptr(dx), B, H, W, K, cop, cip,
                                                      ctx.slope, hip.stream()), "sisr_dgradk_s2_mfma_leaky")
            return dx, dw, db, None
        finally:
            ops.IN_BACKWARD = False


def conv_kxk_s2(x, weight, bias, slope):
    """ops.conv_kxk(stride=2) after its argument checks"""
    return _ConvKxKS2.apply(x, weight, bias, slope)


def _pw_width(c):
    if c > 128:
        raise NotImplementedError(f"the pointwise kernels take maps of at most 128 channels, got {c}")
    return 32 if c <= 32 else 64 if c <= 64 else 128


class _Conv1x1(Function):
    """1 x 1 conv + bias + per-image bias (+ LeakyReLU(slope); slope None: no activation) between channels-last maps of
    32 / 64 / 128 (padded) channels on the fp32 matrix cores.  image_bias (B, cout) is added to every pixel of its image: the
    part of a layer that acts on spatially constant input channels, without those channels in the map.  Backward: the input
    gradient is the same kernel on the role-swapped packing; d image_bias is the per-image ordered column sum of dy."""

    @staticmethod
    def forward(ctx, x, weight, bias, image_bias, slope):
        ops._fp32_only("conv_1x1")
        B, cip, H, W = x.shape
        co, ci = weight.shape[0], weight.shape[1]
        if weight.dim() == 4 and tuple(weight.shape[2:]) != (1, 1):
            raise NotImplementedError(f"conv_1x1 takes a (cout, cin, 1, 1) weight, got {tuple(weight.shape)}")
        cop = _pw_width(co)
        if cip not in (32, 64, 128):
            raise NotImplementedError(f"conv_1x1: the input map must be zero-padded to 32, 64 or 128 channels, got {cip}")
        if _pw_width(ci) != cip:
            raise RuntimeError(f"conv_1x1: weight takes {ci} channels, the map has {cip}")
        if image_bias is not None and tuple(image_bias.shape) != (B, co):
            raise RuntimeError(f"conv_1x1: image_bias must be (B, cout) = ({B}, {co}), got {tuple(image_bias.shape)}")
        x = ops._cl(x)
        L = hip.lib()
        need_dgrad = ctx.needs_input_grad[0]
        buf = torch.empty((2 if need_dgrad else 1, cop * cip), device=weight.device, dtype=torch.float32)
        hip.check(L.sisr_pack_conv1(hip.ptr(weight.contiguous()), hip.ptr(buf[0]), hip.ptr(buf[1]) if need_dgrad else None, co,
                                    ci, cop, cip, hip.stream()), "sisr_pack_conv1")
        ib = image_bias.contiguous() if image_bias is not None else None
        y = ops._empty_cl(B, cop, H, W, x.device)
        nbias = co if (bias is not None or ib is not None) else 0
        hip.check(L.sisr_conv1_mfma_leaky(hip.ptr(x), None, hip.ptr(buf[0]), hip.ptr(bias), hip.ptr(ib), nbias, hip.ptr(y), B, H,
                                          W, cip, cop, int(slope is not None), float(slope or 0.0), hip.stream()),
                  "sisr_conv1_mfma_leaky")
        ctx.save_for_backward(x, y if slope is not None else None, weight, buf[1] if need_dgrad else None)
        ctx.cfg = (B, H, W, co, ci, cop, cip)
        ctx.bias, ctx.has_ib, ctx.slope = bias, image_bias is not None, float(slope or 0.0)
        return y

    @staticmethod
    def backward(ctx, dy):
        ops.IN_BACKWARD = True
        try:
            x, y, weight, pd = ctx.saved_tensors
            B, H, W, co, ci, cop, cip = ctx.cfg
            dy = ops._cl(dy)
            L = hip.lib()
            dx = dw = db = dib = None
            want_db = ctx.bias is not None and ctx.needs_input_grad[2]
            want_dib = ctx.has_ib and ctx.needs_input_grad[3]
            if ctx.needs_input_grad[1] or want_db or want_dib:  # one call makes all three; a frozen weight's gradient is dropped
                dwb = ops._grad_buf(weight) if ctx.needs_input_grad[1] else torch.empty_like(weight)
                db = ops._grad_buf(ctx.bias) if want_db else None
                dib = torch.empty((B, co), device=dy.device, dtype=torch.float32) if want_dib else None
                nb = L.sisr_wgrad1_mfma_workspace_bytes(B, H, W, cip, cop)
                ws = hip.workspace(dy.device, nb)
                hip.check(L.sisr_wgrad1_mfma_leaky(hip.ptr(x), hip.ptr(dy), hip.ptr(y), hip.ptr(dwb), hip.ptr(db), hip.ptr(dib),
                                                   B, H, W, co, ci, cop, cip, hip.ptr(ws), nb, ctx.slope, hip.stream()),
                          "sisr_wgrad1_mfma_leaky")
                dw = dwb if ctx.needs_input_grad[1] else None
            if ctx.needs_input_grad[0]:
                dx = ops._empty_cl(B, cip, H, W, dy.device)
                hip.check(L.sisr_conv1_mfma_leaky(hip.ptr(dy), hip.ptr(y), hip.ptr(pd), None, None, 0, hip.ptr(dx), B, H, W, cop,
                                                  cip, 0, ctx.slope, hip.stream()), "sisr_conv1_mfma_leaky(dgrad)")
            return dx, dw, db, dib, None
        finally:
            ops.IN_BACKWARD = False


def conv_1x1(x, weight, bias=None, slope=None, image_bias=None):
    """pointwise layer on maps of up to 128 channels; image_bias: (B, cout), added with bias before the LeakyReLU(slope)"""
    if slope is not None:
        slope = float(slope)
        if not (math.isfinite(slope) and slope >= 0):  # (the backward reads the sign of the pre-activation off the saved output)
            raise ValueError(f"conv_1x1: the LeakyReLU slope must be finite and >= 0, got {slope}")
    return _Conv1x1.apply(x, weight, bias, image_bias, slope)
