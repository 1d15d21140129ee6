"""Every convolution of csrc/basic.hip, both ways: SRCNN's and VDSR's K x K convs at stride 1 (sisr_convk_*, sisr_wgradk_*) with
their Y-channel ends (sisr_convk_y2f / _f2y, sisr_corrk_y), and the layers IKC's predictor and corrector add: the stride-2
K x K conv (sisr_convk_s2_*, sisr_dgradk_s2_*, sisr_wgradk_s2_*) and the pointwise (1 x 1) layer of up to 128 channels with a
per-image bias (sisr_conv1_*, sisr_wgrad1_*).  ops re-exports the operators: ops.conv_kxk, ops.conv_y2f, ops.conv_1x1, ...
All follow the weight-gradient buffer contract of the neighbouring nodes (ops._grad_buf: frozen inputs, kept and shared
gradients, GRAD_SINK) and capture into a hipGraph: workspaces from hip.workspace, no host synchronisation.
Reaches the core as ops.NAME at call time (the access rule at the top of ops.py)."""
import math

import torch
from torch.autograd import Function

from . import hip, ops


# K x K convolutions (odd K <= 9, padding K // 2).  Maps between layers are channels-last with 32 or 64 channels (real channels
# first, the rest zero); the image ends are contiguous (B, 1, H, W).  Every operator with a ReLU applies its own mask to the
# gradient it receives (on the operand loads of its gradient kernels), so the operators compose freely with conv_chain.
def _pad_width(c):
    if c > 64:
        raise NotImplementedError(f"the K x K kernels take maps of at most 64 channels, got {c}")
    return 32 if c <= 32 else 64


def _check_k(weight):
    K = weight.shape[2]
    if weight.shape[3] != K or K % 2 == 0 or K > 9:
        raise NotImplementedError(f"the K x K kernels take square odd kernels up to 9 x 9, got {tuple(weight.shape[2:])}")
    return K


def _check_map(x, what):
    if x.shape[1] not in (32, 64):
        raise NotImplementedError(f"{what}: the input map must be zero-padded to 32 or 64 channels, got {x.shape[1]}")
    return ops._cl(x)


def _corrk_y(P_, Q, qmask, dw, db, B, H, W, K, channels, cp, flip, db_mode):
    L = hip.lib()
    nb = L.sisr_corrk_y_workspace_bytes(B, H, W, K, cp)
    ws = hip.workspace(Q.device, nb)
    hip.check(L.sisr_corrk_y(hip.ptr(P_), hip.ptr(Q), hip.ptr(qmask), hip.ptr(dw), hip.ptr(db), B, H, W, K, channels, cp,
                             int(flip), int(db_mode), hip.ptr(ws), nb, hip.stream()), "sisr_corrk_y")


class _ConvY2F(Function):
    """(B,1,H,W) image -> channels-last map of _pad_width(cout) channels: conv K x K + bias (+ ReLU).  The first layer of a
    network: it returns no input gradient (ref: basic/architectures.py:45-52 conv_0)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        ops._fp32_only("conv_y2f")
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("conv_y2f is the network-input layer and returns no input gradient")
        B, one, H, W = x.shape
        co = weight.shape[0]
        if one != 1 or weight.shape[1] != 1:
            raise NotImplementedError("conv_y2f takes a one-channel image and a (cout, 1, K, K) weight")
        K, cp = _check_k(weight), _pad_width(co)
        x, w = x.contiguous(), weight.contiguous()
        y = ops._empty_cl(B, cp, H, W, x.device)
        hip.check(hip.lib().sisr_convk_y2f(hip.ptr(x), hip.ptr(w), hip.ptr(bias), None, hip.ptr(y), B, H, W, K, co, cp,
                                           int(relu), 0, hip.stream()), "sisr_convk_y2f")
        ctx.save_for_backward(x, y if relu else None, weight)
        ctx.cfg = (B, H, W, K, co, cp)
        ctx.bias = bias
        return y

    @staticmethod
    @ops._in_backward
    def backward(ctx, dy):
        x, y, weight = ctx.saved_tensors
        B, H, W, K, co, cp = ctx.cfg
        dy = ops._cl(dy)
        dw = ops._grad_buf(weight)
        db = ops._grad_buf(ctx.bias) if ctx.bias is not None else None
        _corrk_y(x, dy, y, dw, db, B, H, W, K, co, cp, 0, 1 if db is not None else 0)
        return None, dw, db, None


def conv_y2f(x, weight, bias=None, relu=False):
    return _ConvY2F.apply(x, weight, bias, bool(relu))


class _ConvF2Y(Function):
    """Channels-last map (32 or 64 channels) -> (B,1,H,W) image: conv K x K + bias (+ residual image, VDSR's `out + x`;
    ref: basic/architectures.py:67-77).  Input gradient: sisr_convk_y2f with flipped taps."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual):
        ops._fp32_only("conv_f2y")
        B, cp, H, W = x.shape
        ci = weight.shape[1]
        if weight.shape[0] != 1 or ci > cp:
            raise NotImplementedError("conv_f2y takes a (1, cin, K, K) weight with cin within the map's channels")
        K = _check_k(weight)
        x, w = _check_map(x, "conv_f2y"), weight.contiguous()
        res = residual.contiguous() if residual is not None else None
        y = torch.empty((B, 1, H, W), device=x.device, dtype=torch.float32)
        hip.check(hip.lib().sisr_convk_f2y(hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(res), hip.ptr(y), B, H, W, K, ci, cp,
                                           hip.stream()), "sisr_convk_f2y")
        ctx.save_for_backward(x, weight)
        ctx.cfg = (B, H, W, K, ci, cp)
        ctx.bias = bias
        return y

    @staticmethod
    @ops._in_backward
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        B, H, W, K, ci, cp = ctx.cfg
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops._empty_cl(B, cp, H, W, dy.device)
            hip.check(hip.lib().sisr_convk_y2f(hip.ptr(dy), hip.ptr(weight.contiguous()), None, None, hip.ptr(dx), B, H, W,
                                               K, ci, cp, 0, 1, hip.stream()), "sisr_convk_y2f(dgrad)")
        want_db = ctx.bias is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:  # one launch makes both (ops._wb_grad_bufs)
            dwb, db, dw = ops._wb_grad_bufs(weight, ctx.bias, ctx.needs_input_grad[1], want_db)
            _corrk_y(dy, x, None, dwb, db, B, H, W, K, ci, cp, 1, 2 if want_db else 0)
        return dx, dw, db, (dy if ctx.needs_input_grad[3] else None)


def conv_f2y(x, weight, bias=None, residual=None):
    return _ConvF2Y.apply(x, weight, bias, residual)


def pack_convk(weight, need_dgrad=True):
    """OIHW weight -> (forward packing, input-gradient packing | None) of sisr_convk_mfma, zero-padded to 32 / 64 channels."""
    co, ci = weight.shape[0], weight.shape[1]
    K, cop, cip = _check_k(weight), _pad_width(co), _pad_width(ci)
    n = K * K * cop * cip
    buf = torch.empty((2 if need_dgrad else 1, n), device=weight.device, dtype=torch.float32)
    hip.check(hip.lib().sisr_pack_convk(hip.ptr(weight.contiguous()), hip.ptr(buf[0]), hip.ptr(buf[1]) if need_dgrad else None,
                                        K, co, ci, cop, cip, hip.stream()), "sisr_pack_convk")
    return buf[0], (buf[1] if need_dgrad else None)


def convk_mfma(x, packed, bias, nbias, y, B, H, W, K, cin_p, cout_p, relu=False, mask=None, in_mask=None):
    hip.check(hip.lib().sisr_convk_mfma(hip.ptr(x), hip.ptr(in_mask), hip.ptr(packed), hip.ptr(bias), int(nbias), hip.ptr(mask),
                                        hip.ptr(y), B, H, W, K, cin_p, cout_p, int(relu), hip.stream()), "sisr_convk_mfma")


def _kxk_operands(ctx, x, weight):
    """The argument checks and the weight packing the stride-1 and stride-2 nodes of conv_kxk share
    -> (channels-last x, forward packing, input-gradient packing | None, (B, H, W, K, co, ci, cop, cip): the nodes' ctx.cfg)."""
    ops._fp32_only("conv_kxk")
    B, cip, H, W = x.shape
    co, ci = weight.shape[0], weight.shape[1]
    K, cop = _check_k(weight), _pad_width(co)
    x = _check_map(x, "conv_kxk")
    if _pad_width(ci) != cip:
        raise RuntimeError(f"conv_kxk: weight takes {ci} channels, the map has {cip}")
    pf, pd = pack_convk(weight, need_dgrad=ctx.needs_input_grad[0])
    return x, pf, pd, (B, H, W, K, co, ci, cop, cip)


class _ConvKxK(Function):
    """K x K conv + bias (+ ReLU, or LeakyReLU(slope)) between channels-last maps of 32 / 64 (padded) channels on the fp32
    matrix cores (ref: basic/architectures.py:45-52, the inner layers).  Backward: the input gradient is the same kernel on
    the flipped / transposed packing; both gradient kernels read dy through the activation's mask (the saved output)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, slope):
        x, pf, pd, (B, H, W, K, co, ci, cop, cip) = _kxk_operands(ctx, x, weight)
        y = ops._empty_cl(B, cop, H, W, x.device)
        if slope is None:
            convk_mfma(x, pf, bias, co if bias is not None else 0, y, B, H, W, K, cip, cop, relu=relu)
        else:
            convk_mfma_leaky(x, pf, bias, co if bias is not None else 0, y, B, H, W, K, cip, cop, slope, act=True)
        ctx.save_for_backward(x, y if (relu or slope is not None) else None, weight, pd)
        ctx.cfg = (B, H, W, K, co, ci, cop, cip)
        ctx.bias, ctx.slope = bias, slope
        return y

    @staticmethod
    @ops._in_backward
    def backward(ctx, dy):
        x, y, weight, pd = ctx.saved_tensors
        B, H, W, K, co, ci, cop, cip = ctx.cfg
        slope = ctx.slope
        dy = ops._cl(dy)
        L = hip.lib()
        dx = dw = db = None
        want_db = ctx.bias is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:  # one call makes both (ops._wb_grad_bufs)
            dwb, db, dw = ops._wb_grad_bufs(weight, ctx.bias, ctx.needs_input_grad[1], want_db)
            nb = L.sisr_wgradk_mfma_workspace_bytes(B, H, W, K, cip, cop)
            ws = hip.workspace(dy.device, nb)
            if slope is None:
                hip.check(L.sisr_wgradk_mfma(hip.ptr(x), hip.ptr(dy), hip.ptr(y), hip.ptr(dwb), hip.ptr(db), B, H, W, K, co,
                                             ci, cop, cip, hip.ptr(ws), nb, hip.stream()), "sisr_wgradk_mfma")
            else:
                hip.check(L.sisr_wgradk_mfma_leaky(hip.ptr(x), hip.ptr(dy), hip.ptr(y), hip.ptr(dwb), hip.ptr(db), B, H, W,
                                                   K, co, ci, cop, cip, hip.ptr(ws), nb, slope, hip.stream()),
                          "sisr_wgradk_mfma_leaky")
        if ctx.needs_input_grad[0]:
            dx = ops._empty_cl(B, cip, H, W, dy.device)
            if slope is None:
                convk_mfma(dy, pd, None, 0, dx, B, H, W, K, cop, cip, in_mask=y)
            else:
                convk_mfma_leaky(dy, pd, None, 0, dx, B, H, W, K, cop, cip, slope, in_mask=y)
        return dx, dw, db, None, None


def convk_mfma_leaky(x, packed, bias, nbias, y, B, H, W, K, cin_p, cout_p, slope, act=False, in_mask=None):
    hip.check(hip.lib().sisr_convk_mfma_leaky(hip.ptr(x), hip.ptr(in_mask), hip.ptr(packed), hip.ptr(bias), int(nbias),
                                              hip.ptr(y), B, H, W, K, cin_p, cout_p, int(act), float(slope), hip.stream()),
              "sisr_convk_mfma_leaky")


def conv_kxk(x, weight, bias=None, relu=False, slope=None, stride=1):
    """slope: LeakyReLU(slope) after the conv, through the leaky entry points (the ReLU path keeps its own selects).
    stride: 1, or 2 (output (H - 1) // 2 + 1 rows; LeakyReLU or no activation -- there is no ReLU form at stride 2)."""
    if stride not in (1, 2):
        raise ValueError(f"conv_kxk: strides 1 and 2 only, got {stride!r}")
    if slope is not None:
        if relu:
            raise ValueError("conv_kxk: relu and slope are two activations; give one of them")
        slope = float(slope)
        if not (math.isfinite(slope) and slope >= 0):  # (the backward reads the sign of the pre-activation off the saved output)
            raise ValueError(f"conv_kxk: the LeakyReLU slope must be finite and >= 0, got {slope}")
    if stride == 2:
        if relu:
            raise ValueError("conv_kxk: stride 2 is built for the LeakyReLU family only; relu=True needs stride 1")
        return conv_kxk_s2(x, weight, bias, slope)
    return _ConvKxK.apply(x, weight, bias, bool(relu), slope)


def conv_s2_out_size(n):
    """output size of a stride-2 K x K conv with padding K // 2 (K odd) along an axis of n pixels"""
    return hip.lib().sisr_convk_s2_out_size(int(n))


class _ConvKxKS2(Function):
    """nn.Conv2d(K, stride=2, padding=K // 2) + bias (+ LeakyReLU(slope); slope None: no activation) between channels-last
    maps on the fp32 matrix cores.  Backward: the input gradient is the polyphase transposed conv on the 'dgrad' packing, the
    weight gradient the stride-1 kernel with a strided x index; both read dy through the saved output."""

    @staticmethod
    def forward(ctx, x, weight, bias, slope):
        x, pf, pd, (B, H, W, K, co, ci, cop, cip) = _kxk_operands(ctx, x, weight)
        y = ops._empty_cl(B, cop, conv_s2_out_size(H), conv_s2_out_size(W), x.device)
        hip.check(hip.lib().sisr_convk_s2_mfma_leaky(hip.ptr(x), hip.ptr(pf), hip.ptr(bias), co if bias is not None else 0,
                                                     hip.ptr(y), B, H, W, K, cip, cop, int(slope is not None),
                                                     float(slope or 0.0), hip.stream()), "sisr_convk_s2_mfma_leaky")
        ctx.save_for_backward(x, y if slope is not None else None, weight, pd)
        ctx.cfg = (B, H, W, K, co, ci, cop, cip)
        ctx.bias, ctx.slope = bias, float(slope or 0.0)
        return y

    @staticmethod
    @ops._in_backward
    def backward(ctx, dy):
        x, y, weight, pd = ctx.saved_tensors
        B, H, W, K, co, ci, cop, cip = ctx.cfg
        dy = ops._cl(dy)
        L = hip.lib()
        dx = dw = db = None
        want_db = ctx.bias is not None and ctx.needs_input_grad[2]
        if ctx.needs_input_grad[1] or want_db:  # one call makes both (ops._wb_grad_bufs)
            dwb, db, dw = ops._wb_grad_bufs(weight, ctx.bias, ctx.needs_input_grad[1], want_db)
            nb = L.sisr_wgradk_s2_mfma_workspace_bytes(B, H, W, K, cip, cop)
            ws = hip.workspace(dy.device, nb)
            hip.check(L.sisr_wgradk_s2_mfma_leaky(hip.ptr(x), hip.ptr(dy), hip.ptr(y), hip.ptr(dwb), hip.ptr(db), B, H, W, K,
                                                  co, ci, cop, cip, hip.ptr(ws), nb, ctx.slope, hip.stream()),
                      "sisr_wgradk_s2_mfma_leaky")
        if ctx.needs_input_grad[0]:
            dx = ops._empty_cl(B, cip, H, W, dy.device)
            hip.check(L.sisr_dgradk_s2_mfma_leaky(hip.ptr(dy), hip.ptr(y), hip.ptr(pd), hip.ptr(dx), B, H, W, K, cop, cip,
                                                  ctx.slope, hip.stream()), "sisr_dgradk_s2_mfma_leaky")
        return dx, dw, db, None


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
    @ops._in_backward
    def backward(ctx, dy):
        x, y, weight, pd = ctx.saved_tensors
        B, H, W, co, ci, cop, cip = ctx.cfg
        dy = ops._cl(dy)
        L = hip.lib()
        dx = dw = db = dib = None
        want_db = ctx.bias is not None and ctx.needs_input_grad[2]
        want_dib = ctx.has_ib and ctx.needs_input_grad[3]
        if ctx.needs_input_grad[1] or want_db or want_dib:  # one call makes all three (ops._wb_grad_bufs)
            dwb, db, dw = ops._wb_grad_bufs(weight, ctx.bias, ctx.needs_input_grad[1], want_db)
            dib = torch.empty((B, co), device=dy.device, dtype=torch.float32) if want_dib else None
            nb = L.sisr_wgrad1_mfma_workspace_bytes(B, H, W, cip, cop)
            ws = hip.workspace(dy.device, nb)
            hip.check(L.sisr_wgrad1_mfma_leaky(hip.ptr(x), hip.ptr(dy), hip.ptr(y), hip.ptr(dwb), hip.ptr(db), hip.ptr(dib),
                                               B, H, W, co, ci, cop, cip, hip.ptr(ws), nb, ctx.slope, hip.stream()),
                      "sisr_wgrad1_mfma_leaky")
        if ctx.needs_input_grad[0]:
            dx = ops._empty_cl(B, cip, H, W, dy.device)
            hip.check(L.sisr_conv1_mfma_leaky(hip.ptr(dy), hip.ptr(y), hip.ptr(pd), None, None, 0, hip.ptr(dx), B, H, W, cop,
                                              cip, 0, ctx.slope, hip.stream()), "sisr_conv1_mfma_leaky(dgrad)")
        return dx, dw, db, dib, None


def conv_1x1(x, weight, bias=None, slope=None, image_bias=None):
    """pointwise layer on maps of up to 128 channels; image_bias: (B, cout), added with bias before the LeakyReLU(slope)"""
    if slope is not None:
        slope = float(slope)
        if not (math.isfinite(slope) and slope >= 0):  # (the backward reads the sign of the pre-activation off the saved output)
            raise ValueError(f"conv_1x1: the LeakyReLU slope must be finite and >= 0, got {slope}")
    return _Conv1x1.apply(x, weight, bias, image_bias, slope)
