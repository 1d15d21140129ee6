"""Conv chains over ops.py's core: differentiable parameter padding, SRMD's conv(+ReLU) chains as one node, the
network-input layout step, and the frozen feature extractor of the perceptual loss (csrc/perceptual.hip).
Reaches the core as ops.NAME at call time (the access rule at the top of ops.py); ops re-exports the operators."""
import torch
from torch.autograd import Function

from . import hip, ops


class _PadAxis(Function):
    """Zero-pad ONE axis of a contiguous tensor seen as [outer][n][inner] to [outer][P][inner] (one sisr_pad_oihw launch);
    backward crops.  The building block of pad_param."""

    @staticmethod
    def forward(ctx, t, outer, n, inner, P):
        ctx.in_shape = tuple(t.shape)
        t = t.contiguous()
        ctx.geo = (outer, n, inner, P)
        out = torch.empty(outer * P * inner, device=t.device, dtype=torch.float32)
        hip.check(hip.lib().sisr_pad_oihw(hip.ptr(t), hip.ptr(out), outer, n, outer, P, inner, 0, hip.stream()), "sisr_pad_oihw")
        return out

    @staticmethod
    def backward(ctx, g):
        outer, n, inner, P = ctx.geo
        g = g.contiguous()
        out = torch.empty(outer * n * inner, device=g.device, dtype=torch.float32)
        hip.check(hip.lib().sisr_pad_oihw(hip.ptr(g), hip.ptr(out), outer, n, outer, P, inner, 1, hip.stream()),
                  "sisr_pad_oihw(crop)")
        return out.reshape(ctx.in_shape), None, None, None, None


def pad_param(t, steps, shape):
    """Differentiable zero-padding of a parameter for a network whose feature count is not a multiple of 64 (architectures.
    ChannelPadded): steps = [(outer, n, inner, P)] applied in order, the result viewed as `shape`.  Gradients come back cropped."""
    for outer, n, inner, P in steps:
        t = _PadAxis.apply(t, outer, n, inner, P)
    return t.reshape(shape)


class _ConvChain(Function):
    """y_k = act_k(conv3x3_k(y_{k-1}) + b_k), act = ReLU or identity, as ONE autograd node (ref: the C / CR stacks of
    advanced/SRMD_blocks.py:33-126 behind advanced/architectures.py:380-425 SRMD).  Input: channels-last map whose channel
    count is a multiple of 64 (zero-padded); weights keep their OIHW shapes and are zero-padded to 64-multiples per step;
    the output has the last layer's padded channel count.  Backward: the ReLU mask of layer k-1 is applied by the epilogue
    of layer k's input-gradient conv, so no gradient map is touched by an elementwise pass."""

    @staticmethod
    def forward(ctx, x, relus, *params):
        n = len(relus)
        B, C0, H, W = x.shape
        if C0 % 64:
            raise NotImplementedError("conv chain input must be zero-padded to a multiple of 64 channels")
        dev = x.device
        x = ops._cl(x)
        ops._join_pending.clear()
        cur, cin_p = x, C0
        maps, packs, geo = [], [], []
        for k in range(n):
            w, b = params[2 * k], params[2 * k + 1]
            co, ci = w.shape[0], w.shape[1]
            cop = ops._pad64(co)
            if ci > cin_p:
                raise RuntimeError(f"conv chain layer {k}: weight takes {ci} channels, the map has {cin_p}")
            wp = ops._pad_oihw(w, cop, cin_p)
            bp = ops._pad_oihw(b.reshape(co, 1), cop, 1).reshape(cop) if b is not None else None
            pf, pd = ops.pack_pair(wp)
            y = ops._empty_cl(B, cop, H, W, dev)
            ops.conv_c64(cur, hip.view_plain(H, W, cin_p), pf, bp, (1, 64), y, hip.view_plain(H, W, cop), B, H, W, cin_p, cop,
                         relu=int(relus[k]))  # 0 linear, 1 ReLU, 2 LeakyReLU(0.2)
            maps.append(cur)
            packs.append(pd)
            geo.append((cin_p, cop, tuple(w.shape), b is not None))
            cur, cin_p = y, cop
        if relus[-1]:  # an activated last layer: its mask is applied to the incoming gradient by one elementwise pass
            maps.append(cur)
        ctx.save_for_backward(*maps, *[params[2 * k] for k in range(n)])
        ctx.cfg = (n, tuple(relus), (B, H, W), geo)
        ctx.packs = packs
        return cur

    @staticmethod
    @ops._in_backward
    def backward(ctx, dy):
        n, relus, (B, H, W), geo = ctx.cfg
        sv = list(ctx.saved_tensors)
        nm = n + (1 if relus[-1] else 0)
        maps, ws = sv[:nm], sv[nm:]
        dev = dy.device
        g = ops._cl(dy)
        if relus[-1]:  # g <- dy * act'(last output): ReLU' (op 6) or LeakyReLU' (op 3) over the 64-channel blocks
            gm = torch.empty_like(g)
            ops._map64(maps[n], 64, g, 64, gm, 64, g.numel() // 64, 3 if relus[-1] == 2 else 6)
            g = gm
        side = ops._side_ok(*ws)
        grads = [None] * (2 * n)
        for k in range(n - 1, -1, -1):
            cin_p, cop, wshape, has_b = geo[k]
            xin = maps[k]
            padded = (cop, cin_p) != (wshape[0], wshape[1])
            dwp = torch.empty((cop, cin_p, 3, 3), device=dev) if padded else ops._grad_buf(ws[k])
            dbp = torch.empty(cop, device=dev) if has_b else None

            def wg(xin=xin, g=g, dwp=dwp, dbp=dbp, cin_p=cin_p, cop=cop):
                ops.wgrad_c64(xin, hip.view_plain(H, W, cin_p), g, hip.view_plain(H, W, cop), dwp, dbp, B, H, W, cin_p, cop)

            ops._side_launch(dev, wg, (xin, g, dwp, dbp), side)
            if k > 0 or ctx.needs_input_grad[0]:
                gin = ops._empty_cl(B, cin_p, H, W, dev)
                ops.conv_c64(g, hip.view_plain(H, W, cop), ctx.packs[k], None, (1, 64), gin, hip.view_plain(H, W, cin_p), B, H,
                             W, cop, cin_p, mask=(xin if (k > 0 and relus[k - 1]) else None),
                             relu=(ops.LEAKY_MASK if (k > 0 and relus[k - 1] == 2) else 0))
            else:
                gin = None
            if padded:  # the crop reads what the (possibly side-stream) weight gradient wrote
                def crop(dwp=dwp, dbp=dbp, k=k, wshape=wshape, has_b=has_b):
                    grads[2 * k] = ops._crop_oihw(dwp, wshape)
                    grads[2 * k + 1] = ops._crop_oihw(dbp.reshape(-1, 1), (wshape[0], 1)).reshape(wshape[0]) if has_b else None
                if side:
                    with torch.cuda.stream(ops.side_stream(dev)):
                        crop()
                        for t in (grads[2 * k], grads[2 * k + 1]):
                            if t is not None:
                                t.record_stream(torch.cuda.current_stream(dev))
                else:
                    crop()
            else:
                grads[2 * k], grads[2 * k + 1] = dwp, dbp
            g = gin
        return (g if ctx.needs_input_grad[0] else None, None, *grads)


def conv_chain(x, layers):
    """layers: [(weight, bias, act)] with act 0 / False linear, 1 / True ReLU, 2 LeakyReLU(0.2) -> channels-last map with the
    last layer's (64-padded) channel count."""
    flat = []
    for w, b, _ in layers:
        flat += [w, b]
    return _ConvChain.apply(x, tuple(int(r) for _, _, r in layers), *flat)


def nchw_to_nhwc_pad(x, cp=None):
    """(B, C, H, W) contiguous NCHW -> channels-last (B, cp, H, W) map, channels >= C zero (no gradient: network input)."""
    if x.requires_grad:
        raise NotImplementedError("nchw_to_nhwc_pad is the network-input layout step and returns no gradient")
    B, C, H, W = x.shape
    cp = ops._pad64(C) if cp is None else cp
    y = ops._empty_cl(B, cp, H, W, x.device)
    hip.check(hip.lib().sisr_nchw_to_nhwc_pad(hip.ptr(x.contiguous()), hip.ptr(y), B, C, H, W, cp, hip.stream()),
              "sisr_nchw_to_nhwc_pad")
    return y


# ----------------------------------------------------------------------------- frozen feature extractor (csrc/perceptual.hip)
class FrozenChain:
    """The device-side form of a frozen stack of 3x3 convs with 2x2 max-pools between its blocks (VGG19's features[:35] for
    the perceptual loss, perceptual.VGGFeatureExtractor): forward and input-gradient packings of every weight, zero-padded to
    64-channel multiples, built ONCE from the weights as they are now and owned by whoever holds this object -- they are not
    entries of the step-level packing, so invalidate_packs() (which follows every optimiser step of the trainable network)
    leaves them alone.  blocks: [[(weight, bias), ...], ...], a pool after every block but the last; ReLU after every conv but
    the very last.  mean / std: the three input-normalisation constants each (None: the image goes in as it is)."""

    def __init__(self, blocks, mean=None, std=None):
        ops._fp32_only("the frozen feature extractor")
        first = blocks[0][0][0]
        dev = first.device
        if first.shape[1] != 3:
            raise NotImplementedError(f"the feature extractor reads RGB images; its first conv takes {first.shape[1]} channels")
        self.device = dev
        self.mean = torch.as_tensor([0.0] * 3 if mean is None else mean, dtype=torch.float32).reshape(3).to(dev).contiguous()
        self.std = torch.as_tensor([1.0] * 3 if std is None else std, dtype=torch.float32).reshape(3).to(dev).contiguous()
        self.blocks = []
        cin_p = 64
        with torch.no_grad():
            for convs in blocks:
                layers = []
                for w, b in convs:
                    if w.requires_grad or (b is not None and b.requires_grad):
                        raise RuntimeError("FrozenChain takes frozen weights (requires_grad == False); trainable stacks go "
                                           "through conv_chain")
                    co, ci = w.shape[0], w.shape[1]
                    if tuple(w.shape[2:]) != (3, 3) or ci > cin_p:
                        raise RuntimeError(f"frozen chain: a {tuple(w.shape)} weight does not follow a {cin_p}-channel map")
                    cop = ops._pad64(co)
                    wp = ops._pad_oihw(w.detach(), cop, cin_p)
                    bp = ops._pad_oihw(b.detach().reshape(co, 1), cop, 1).reshape(cop) if b is not None else None
                    pf, pd = ops.pack_pair(wp)
                    layers.append((pf, pd, bp, cin_p, cop))
                    cin_p = cop
                self.blocks.append(layers)
        self.channels = blocks[-1][-1][0].shape[0]


def _maxpool2(y, B, H, W, C):
    out = ops._empty_cl(B, C, H // 2, W // 2, y.device)
    hip.check(hip.lib().sisr_maxpool2_fwd(hip.ptr(y), hip.ptr(out), B, H, W, C, hip.stream()), "sisr_maxpool2_fwd")
    return out


class _FrozenFeatures(Function):
    """phi(img) for a FrozenChain as ONE autograd node: normalise + lay out channels-last (sisr_vgg_prep_fwd), the blocks'
    convs with their ReLU epilogues, sisr_maxpool2_fwd between blocks.  No weight gradients exist, so the backward is the
    chain of input-gradient convs alone -- inside a block with the ReLU-mask epilogue, across a pool through
    sisr_maxpool2_relu_bwd (pool routing and the ReLU in front of it in one pass over the saved map), sisr_vgg_prep_bwd at
    the end -- and all it keeps from the forward pass are the post-ReLU conv outputs.  Without a gradient to return (the
    target's features, evaluation) nothing is kept at all."""

    @staticmethod
    def forward(ctx, img, chain):
        B, C, H, W = img.shape
        if C != 3:
            raise RuntimeError(f"the feature extractor reads (B, 3, H, W) RGB images, got {tuple(img.shape)}")
        dev = img.device
        if dev != chain.device:
            raise RuntimeError(f"feature extractor packed on {chain.device}, image on {dev}")
        L = hip.lib()
        keep = ctx.needs_input_grad[0]
        cur = ops._empty_cl(B, 64, H, W, dev)
        hip.check(L.sisr_vgg_prep_fwd(hip.ptr_c(img), hip.ptr(chain.mean), hip.ptr(chain.std), hip.ptr(cur), B, H, W,
                                      64, hip.stream()), "sisr_vgg_prep_fwd")
        saved, geo = [], []
        nb = len(chain.blocks)
        for bi, layers in enumerate(chain.blocks):
            for li, (pf, _, bp, cin_p, cop) in enumerate(layers):
                last = bi == nb - 1 and li == len(layers) - 1
                y = ops._empty_cl(B, cop, H, W, dev)
                ops.conv_c64(cur, hip.view_plain(H, W, cin_p), pf, bp, (1, 64), y, hip.view_plain(H, W, cop), B, H, W, cin_p, cop,
                             relu=0 if last else 1)
                if keep and not last:
                    saved.append(y)
                cur = y
            geo.append((H, W))
            if bi < nb - 1:
                cur = _maxpool2(cur, B, H, W, layers[-1][4])
                H, W = H // 2, W // 2
        if keep:
            ctx.save_for_backward(*saved)
            ctx.chain, ctx.geo, ctx.B = chain, geo, B
        return cur

    @staticmethod
    @ops._in_backward
    def backward(ctx, dy):
        chain, geo, B = ctx.chain, ctx.geo, ctx.B
        saved = list(ctx.saved_tensors)  # post-ReLU outputs of every conv but the last, in forward order
        dev = dy.device
        L = hip.lib()
        g = ops._cl(dy)
        k = len(saved)  # index of the current conv's output among `saved` (the last conv's is not there)
        for bi in range(len(chain.blocks) - 1, -1, -1):
            H, W = geo[bi]
            layers = chain.blocks[bi]
            for li in range(len(layers) - 1, -1, -1):
                _, pd, _, cin_p, cop = layers[li]
                k -= 1  # saved[k]: the map this conv read, where that is a conv output of the same block
                gin = ops._empty_cl(B, cin_p, H, W, dev)
                ops.conv_c64(g, hip.view_plain(H, W, cop), pd, None, (1, 64), gin, hip.view_plain(H, W, cin_p), B, H, W, cop,
                             cin_p, mask=saved[k] if li > 0 else None)
                g = gin
            if bi > 0:  # g: gradient of the pooled map -> gradient of the previous block's last conv, before its ReLU
                Hp, Wp = geo[bi - 1]
                y = saved[k]
                gy = torch.empty_like(y)
                hip.check(L.sisr_maxpool2_relu_bwd(hip.ptr(y), hip.ptr(g), hip.ptr(gy), B, Hp, Wp, y.shape[1], hip.stream()),
                          "sisr_maxpool2_relu_bwd")
                g = gy
        H, W = geo[0]
        dimg = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32)
        hip.check(L.sisr_vgg_prep_bwd(hip.ptr(g), hip.ptr(chain.std), hip.ptr(dimg), B, H, W, 64, hip.stream()),
                  "sisr_vgg_prep_bwd")
        return dimg, None


def frozen_features(img, chain):
    """(B, 3, H, W) RGB image -> channels-last feature map of `chain` (a FrozenChain); differentiable in the image only."""
    return _FrozenFeatures.apply(img, chain)
