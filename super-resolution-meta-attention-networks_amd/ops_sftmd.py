"""SFTMD's operators over ops.py's core (csrc/sft.hip): the SFT layer in its merged and concat forms, the network's head
and tail nodes, and the whole-network forward.  The step-level composition of the merged weights (ops._sft_plan) stays in
ops.py, where pack_all drives it.
Reaches the core as ops.NAME at call time (the access rule at the top of ops.py); ops re-exports the operators."""
import torch
from torch.autograd import Function

from . import hip, ops


def _sft_compose(params, merged, M, split=0):
    """params: the eight parameter (or gradient) tensors of a StandardSft; merged: (WA, bA, WB, bB)."""
    hip.check(hip.lib().sisr_sft_compose(*[hip.ptr_c(t) for t in params], *[hip.ptr(t) for t in merged], int(M), int(split),
                                         hip.stream()), "sisr_sft_compose")


class _SftLayer(Function):
    """out = [relu](x * sigmoid(mul(cat)) + add(cat)), cat = (x, metadata maps); mul / add = conv3x3 -> LeakyReLU(0.2) ->
    conv3x3 with 32 hidden channels each (ref: SFTMD_variants/architectures.py:25-56 StandardSft; the F.relu of
    SFT_Residual_Block.forward :100-102 folded in).  Two MFMA convs instead of four: A = [mul_conv1 | add_conv1] merged
    along the outputs (128 -> 64, LeakyReLU epilogue), B = block-diagonal [mul_conv2, add_conv2] (64 -> 128); the merged
    weights are composed per call from the four parameters and their gradients split back.  md: channels-last
    [B, 64, H, W], the M metadata maps zero-padded (no gradient); torch.cat((x, maps)) is never materialised: conv A and its
    weight gradient read the pair through a view whose second chunk points at md (hip.view_pair)."""

    @staticmethod
    def forward(ctx, x, md, relu, M, mw1, mb1, aw1, ab1, mw2, mb2, aw2, ab2):
        ops._fp32_only("SFT layer")
        B, C, H, W = x.shape
        if C != 64 or md.shape != (B, 64, H, W) or tuple(mw1.shape) != (32, 64 + M, 3, 3) or tuple(mw2.shape) != (64, 32, 3, 3):
            raise NotImplementedError("SFT layer: 64 features, 32 hidden channels, at most 64 metadata maps")
        dev, npix = x.device, B * H * W
        x, md = ops._cl(x), ops._cl(md)
        # cat(x, maps) is never built: the conv reads chunk 0 from x and chunk 1 from the (shared) metadata map through the
        # view's chunk offset -- two allocations, one logical 128-channel input
        diff = md.data_ptr() - x.data_ptr()
        if diff % 16:
            raise RuntimeError("SFT layer: feature and metadata maps must be 16-byte aligned relative to each other")
        vcat = hip.view_pair(H, W, diff // 4)
        hit = ops._SFT_STEP.get(id(mw1))
        if hit is not None and hit[0] is mw1:  # composed (and packed) once for the whole step by pack_all
            WA, bA, WB, bB = hit[1:]
        else:
            WA = torch.empty((64, 128, 3, 3), device=dev)
            bA = torch.empty(64, device=dev)
            WB = torch.empty((128, 64, 3, 3), device=dev)
            bB = torch.empty(128, device=dev)
            _sft_compose((mw1, mb1, aw1, ab1, mw2, mb2, aw2, ab2), (WA, bA, WB, bB), M)
        pfA, pdA = ops.pack_pair(WA)
        pfB, pdB = ops.pack_pair(WB)
        t = ops._empty_cl(B, 64, H, W, dev)
        ops.conv_c64(x, vcat, pfA, bA, (1, 64), t, hip.view_plain(H, W, 64), B, H, W, 128, 64, relu=ops.LEAKY,
                     select=ops.SPARSE_SECOND_CHUNK if M <= 16 else 0)
        y2 = ops._empty_cl(B, 128, H, W, dev)
        ops.conv_c64(t, hip.view_plain(H, W, 64), pfB, bB, (1, 64), y2, hip.view_plain(H, W, 128), B, H, W, 64, 128,
                     select=ops.SPARSE_BLOCK_DIAGONAL)
        out = ops._empty_cl(B, 64, H, W, dev)
        hip.check(hip.lib().sisr_sft_combine_fwd(hip.ptr(x), 64, hip.ptr(y2), None, hip.ptr(out), 64, npix, int(relu),
                                                 hip.stream()), "sisr_sft_combine_fwd")
        ctx.save_for_backward(x, md, t, y2)
        ctx.packs = (pdA, pdB)
        ctx.cfg = (B, H, W, int(relu), M)
        return out

    @staticmethod
    @ops._in_backward
    def backward(ctx, dout):
        x, md, t, y2 = ctx.saved_tensors
        pdA, pdB = ctx.packs
        B, H, W, relu, M = ctx.cfg
        vcat = hip.view_pair(H, W, (md.data_ptr() - x.data_ptr()) // 4)
        dev, npix = dout.device, B * H * W
        dout = ops._cl(dout)
        v64, v128 = hip.view_plain(H, W, 64), hip.view_plain(H, W, 128)
        dx0 = ops._empty_cl(B, 64, H, W, dev)
        dy2 = ops._empty_cl(B, 128, H, W, dev)
        hip.check(hip.lib().sisr_sft_combine_bwd(hip.ptr(dout), 64, hip.ptr(x), 64, hip.ptr(y2), hip.ptr(dx0),
                                                 hip.ptr(dy2), npix, relu, hip.stream()), "sisr_sft_combine_bwd")
        dWB = torch.empty((128, 64, 3, 3), device=dev)
        dbB = torch.empty(128, device=dev)
        ops.wgrad_c64(t, v64, dy2, v128, dWB, dbB, B, H, W, 64, 128, active_units=0xC3)  # the two diagonal 64 x 32 blocks
        dt = ops._empty_cl(B, 64, H, W, dev)
        ops.conv_c64(dy2, v128, pdB, None, (1, 64), dt, v64, B, H, W, 128, 64, mask=t, relu=ops.LEAKY_MASK, select=ops.SPARSE_HALVES)
        dWA = torch.empty((64, 128, 3, 3), device=dev)
        dbA = torch.empty(64, device=dev)
        # input channels >= 96 are padding when M <= 32: the last ci half of the second chunk is never read back
        ops.wgrad_c64(x, vcat, dt, v64, dWA, dbA, B, H, W, 128, 64, active_units=0x3F if M <= 32 else 0)
        dx = None
        if ctx.needs_input_grad[0]:
            # input gradient of A for the 64 feature channels only (output chunk 0 of the packing) + the direct term
            dx = ops._empty_cl(B, 64, H, W, dev)
            ops.conv_c64(dt, v64, pdA, None, (1, 64), dx, v64, B, H, W, 64, 64, res=dx0)
        g = [torch.empty(s, device=dev) for s in ((32, 64 + M, 3, 3), (32,), (32, 64 + M, 3, 3), (32,), (64, 32, 3, 3),
                                                  (64,), (64, 32, 3, 3), (64,))]
        _sft_compose(g, (dWA, dbA, dWB, dbB), M, split=1)
        return (dx, None, None, None, *g)


def sft_layer(x, md, module, relu):
    """module: sftmd.StandardSft (parameter holder)."""
    M = module.mul_conv1.weight.shape[1] - 64
    return _SftLayer.apply(x, md, bool(relu), int(M), *module.params())


class _Map64(Function):
    """Elementwise pieces of the non-default SFT types on channels-last 64-channel maps (csrc/sft.hip map64):
    mode 'relu': relu(x); 'mul': x * md (WeakSft, 64 maps); 'mul0': x * md[:, 0:1] (WeakSft, one map).  md has no gradient."""

    @staticmethod
    def forward(ctx, x, md, mode):
        B, C, H, W = x.shape
        if C != 64:
            raise NotImplementedError("64-channel maps")
        x = ops._cl(x)
        out = ops._empty_cl(B, 64, H, W, x.device)
        npix = B * H * W
        if mode == "relu":
            ops._map64(x, 64, None, 0, out, 64, npix, 5)
            ctx.save_for_backward(out)
        else:
            md = ops._cl(md)
            ops._map64(x, 64, md, 64, out, 64, npix, 4 if mode == "mul" else 7)
            ctx.save_for_backward(md)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, dy):
        (t,) = ctx.saved_tensors
        B, C, H, W = dy.shape
        dy = ops._cl(dy)
        dx = ops._empty_cl(B, 64, H, W, dy.device)
        if ctx.mode == "relu":
            ops._map64(t, 64, dy, 64, dx, 64, B * H * W, 6)
        else:
            ops._map64(dy, 64, t, 64, dx, 64, B * H * W, 4 if ctx.mode == "mul" else 7)
        return dx, None, None


class _ConcatSft(Function):
    """conv3x3(cat(x, maps)) (ref: SFTMD_variants/architectures.py:8-14) as one 128 -> 64 MFMA conv over the (features | maps)
    map, weight zero-padded per call; only the feature half of the input gradient is computed."""

    @staticmethod
    def forward(ctx, x, md, w, b):
        ops._fp32_only("SFT layer")
        B, C, H, W = x.shape
        M = w.shape[1] - 64
        if C != 64 or tuple(w.shape) != (64, 64 + M, 3, 3) or not 0 <= M <= 64:
            raise NotImplementedError("ConcatSft: 64 features, at most 64 metadata maps")
        dev = x.device
        x, md = ops._cl(x), ops._cl(md)
        diff = md.data_ptr() - x.data_ptr()
        if diff % 16:
            raise RuntimeError("ConcatSft: feature and metadata maps must be 16-byte aligned relative to each other")
        pf, pd = ops.pack_pair(ops._pad_oihw(w, 64, 128))
        y = ops._empty_cl(B, 64, H, W, dev)
        ops.conv_c64(x, hip.view_pair(H, W, diff // 4), pf, b, (1, 64), y, hip.view_plain(H, W, 64), B, H, W, 128, 64)
        ctx.save_for_backward(x, md)
        ctx.pd, ctx.cfg = pd, (B, H, W, tuple(w.shape), b is not None)
        return y

    @staticmethod
    @ops._in_backward
    def backward(ctx, dy):
        x, md = ctx.saved_tensors
        B, H, W, wshape, has_b = ctx.cfg
        dev = dy.device
        dy = ops._cl(dy)
        v64 = hip.view_plain(H, W, 64)
        dwp = torch.empty((64, 128, 3, 3), device=dev)
        db = torch.empty(64, device=dev) if has_b else None
        ops.wgrad_c64(x, hip.view_pair(H, W, (md.data_ptr() - x.data_ptr()) // 4), dy, v64, dwp, db, B, H, W, 128, 64)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops._empty_cl(B, 64, H, W, dev)
            ops.conv_c64(dy, v64, ctx.pd, None, (1, 64), dx, v64, B, H, W, 64, 64)  # output chunk 0 of the packing = d features
        return dx, None, ops._crop_oihw(dwp, wshape), db


def sft_apply(x, md, layer, relu):
    """One SFT_Layer (sftmd.SFT_Layer: 'standard' / 'concat' / 'weak' / 'none', ref: SFTMD_variants/architectures.py:59-77)
    followed by the block's F.relu when `relu`."""
    kind = layer.kind
    if kind == "standard":
        return sft_layer(x, md, layer.sft_module, relu)
    if kind == "concat":
        y = _ConcatSft.apply(x, md, layer.sft_module.conv.weight, layer.sft_module.conv.bias)
    elif kind == "weak":
        y = _Map64.apply(x, md, "mul0" if layer.maps == 1 else "mul")
    else:
        y = x
    return _Map64.apply(y, None, "relu") if relu else y


class _SftmdHead(Function):
    """fea_bef = conv3(leaky(conv2(leaky(conv1(x))))) (ref: SFTMD_variants/architectures.py:162): x NCHW RGB."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3):
        ops._fp32_only("SFTMD")
        B, C, H, W = x.shape
        if (C > 64 or tuple(w1.shape) != (64, C, 3, 3) or tuple(w2.shape) != (64, 64, 3, 3) or
                tuple(w3.shape) != (64, 64, 3, 3)):
            raise NotImplementedError("SFTMD head: (RGB [+ metadata maps, at most 64 channels]) -> 64 -> 64 -> 64")
        dev, npix = x.device, B * H * W
        x = x.contiguous()
        v64 = hip.view_plain(H, W, 64)
        y1 = ops._empty_cl(B, 64, H, W, dev)
        if C == 3:
            hip.check(hip.lib().sisr_conv3x3_cin3(hip.ptr(x), hip.ptr(w1.contiguous()), 27, 9, 0, hip.ptr(b1), hip.ptr(y1), v64,
                                                  B, H, W, 64, hip.stream()), "sisr_conv3x3_cin3")
            ops._map64(y1, 64, None, 0, y1, 64, npix, 2)
        else:
            # concat_strategy (ref: SFTMD_variants/handlers.py:12-14, attention_manipulators/__init__.py:97-98): the metadata
            # maps ride in the input, conv1 is (3 + M) -> 64.  The NCHW input is laid out once as a zero-padded channels-last
            # 64-channel map and conv1 runs on the MFMA kernel with zero-padded weights (exact zeros: same sums)
            x = ops.nchw_to_nhwc_pad(x.detach(), 64)
            ops.conv_c64(x, v64, ops.pack_weight(ops._pad_oihw(w1, 64, 64), "fwd"), b1, (1, 64), y1, v64, B, H, W, 64, 64, relu=ops.LEAKY)
        pf2, pd2 = ops.pack_pair(w2.contiguous())
        pf3, pd3 = ops.pack_pair(w3.contiguous())
        y2 = ops._empty_cl(B, 64, H, W, dev)
        ops.conv_c64(y1, v64, pf2, b2, (1, 64), y2, v64, B, H, W, 64, 64, relu=ops.LEAKY)
        y3 = ops._empty_cl(B, 64, H, W, dev)
        ops.conv_c64(y2, v64, pf3, b3, (1, 64), y3, v64, B, H, W, 64, 64)
        ctx.rgb = C == 3
        ctx.save_for_backward(x, y1, y2, w1, w2, w3)
        ctx.packs = (pd2, pd3)
        return y3

    @staticmethod
    @ops._in_backward
    def backward(ctx, d3):
        x, y1, y2, w1, w2, w3 = ctx.saved_tensors
        pd2, pd3 = ctx.packs
        B, _, H, W = x.shape
        dev = x.device
        L = hip.lib()
        d3 = ops._cl(d3)
        v64 = hip.view_plain(H, W, 64)
        dw3, db3 = ops._grad_buf(w3), torch.empty(64, device=dev)
        ops.wgrad_c64(y2, v64, d3, v64, dw3, db3, B, H, W, 64, 64, owner=w3)
        d2 = ops._empty_cl(B, 64, H, W, dev)
        ops.conv_c64(d3, v64, pd3, None, (1, 64), d2, v64, B, H, W, 64, 64, mask=y2, relu=ops.LEAKY_MASK)
        dw2, db2 = ops._grad_buf(w2), torch.empty(64, device=dev)
        ops.wgrad_c64(y1, v64, d2, v64, dw2, db2, B, H, W, 64, 64, owner=w2)
        d1 = ops._empty_cl(B, 64, H, W, dev)
        ops.conv_c64(d2, v64, pd2, None, (1, 64), d1, v64, B, H, W, 64, 64, mask=y1, relu=ops.LEAKY_MASK)
        db1 = torch.empty(64, device=dev)
        if ctx.rgb:
            dw1 = torch.empty_like(w1)
            nbytes = L.sisr_corr3x3_c3_workspace_bytes(B, H, W, 64)
            ws = hip.workspace(dev, nbytes)
            hip.check(L.sisr_corr3x3_c3(hip.ptr(x), hip.ptr(d1), v64, 1.0, hip.ptr(dw1), 27, 9, 0, 0, hip.ptr(db1),
                                        hip.ptr(ws), nbytes, B, H, W, 64, hip.stream()), "sisr_corr3x3_c3(head)")
        else:  # x is the padded 64-channel input map: full 64 x 64 weight gradient, cropped to the (3 + M) real inputs
            dw1p = torch.empty((64, 64, 3, 3), device=dev)
            ops.wgrad_c64(x, v64, d1, v64, dw1p, db1, B, H, W, 64, 64)
            dw1 = ops._crop_oihw(dw1p, tuple(w1.shape))
        return None, dw1, db1, dw2, db2, dw3, db3


class _SftmdTail(Function):
    """clamp(conv_output(upscale(conv_mid(fea)))) (ref: SFTMD_variants/architectures.py:137-176): conv_mid, then one
    (x2, x3: PixelShuffle(scale)) or two (x4: PixelShuffle(2) twice) conv -> shuffle -> LeakyReLU(0.2) stages with the
    shuffle as the conv's output view and the activation as its epilogue, the 9x9 64 -> 3 conv and the clamp to [0, 1]."""

    @staticmethod
    def forward(ctx, fea, n_up, *params):
        ops._fp32_only("SFTMD")
        B, C, H, W = fea.shape
        dev = fea.device
        wm, bm = params[0], params[1]
        ups = [(params[2 + 2 * k], params[3 + 2 * k]) for k in range(n_up)]
        wo, bo = params[2 + 2 * n_up], params[3 + 2 * n_up]
        if C != 64 or tuple(wo.shape) != (3, 64, 9, 9):
            raise NotImplementedError("SFTMD tail: 64 features, 9x9 64 -> 3 output conv")
        fea = ops._cl(fea)
        v64 = hip.view_plain(H, W, 64)
        pfm, pdm = ops.pack_pair(wm.contiguous())
        m = ops._empty_cl(B, 64, H, W, dev)
        ops.conv_c64(fea, v64, pfm, bm, (1, 64), m, v64, B, H, W, 64, 64)
        maps, geo, packs = [fea, m], [], [pdm]
        cur, h, w = m, H, W
        for wu, bu in ups:
            rr = wu.shape[0] // 64
            r = int(round(rr ** 0.5))
            if r * r != rr or wu.shape[1] != 64 or r < 2:
                raise NotImplementedError("SFTMD upscale conv: 64 -> 64 r^2 feeding PixelShuffle(r)")
            pf, pd = ops.pack_pair(wu.contiguous(), r)
            y = ops._empty_cl(B, 64, h * r, w * r, dev)
            ops.conv_c64(cur, hip.view_plain(h, w, 64), pf, bu, (rr, 1), y, hip.view_shuffle(h, w, r), B, h, w, 64, 64 * rr,
                         relu=ops.LEAKY)
            geo.append((h, w, r))
            packs.append(pd)
            maps.append(y)
            cur, h, w = y, h * r, w * r
        pre = torch.empty((B, 3, h, w), device=dev)
        hip.check(hip.lib().sisr_conv9_fwd(hip.ptr(cur), hip.ptr(wo.contiguous()), hip.ptr(bo), hip.ptr(pre), B, h, w,
                                           hip.stream()), "sisr_conv9_fwd")
        out = torch.empty_like(pre)
        hip.check(hip.lib().sisr_clamp01(hip.ptr(pre), None, hip.ptr(out), pre.numel(), 0, hip.stream()), "sisr_clamp01")
        ctx.save_for_backward(pre, *maps, wm, *[u[0] for u in ups], wo)
        ctx.cfg = (B, H, W, n_up, geo)
        ctx.packs = packs
        return out

    @staticmethod
    @ops._in_backward
    def backward(ctx, dout):
        B, H, W, n_up, geo = ctx.cfg
        sv = list(ctx.saved_tensors)
        pre, maps, ws_ = sv[0], sv[1:3 + n_up], sv[3 + n_up:]
        wm, wus, wo = ws_[0], ws_[1:1 + n_up], ws_[1 + n_up]
        dev = pre.device
        L = hip.lib()
        h, w = pre.shape[2], pre.shape[3]
        dpre = torch.empty_like(pre)
        hip.check(L.sisr_clamp01(hip.ptr(pre), hip.ptr(dout.contiguous()), hip.ptr(dpre), pre.numel(), 1, hip.stream()),
                  "sisr_clamp01(backward)")
        top = maps[-1]  # the activated map the 9x9 conv read
        dwo, dbo = torch.empty_like(wo), torch.empty(3, device=dev)
        nbytes = L.sisr_conv9_wgrad_workspace_bytes(B, h, w)
        ws = hip.workspace(dev, nbytes)
        hip.check(L.sisr_conv9_wgrad(hip.ptr(top), hip.ptr(dpre), hip.ptr(dwo), hip.ptr(dbo), hip.ptr(ws), nbytes, B, h, w,
                                     hip.stream()), "sisr_conv9_wgrad")
        g = ops._empty_cl(B, 64, h, w, dev)
        hip.check(L.sisr_conv9_dgrad(hip.ptr(dpre), hip.ptr(wo.contiguous()), hip.ptr(top) if n_up else None, hip.ptr(g), B,
                                     h, w, hip.stream()), "sisr_conv9_dgrad")
        grads = [None] * (4 + 2 * n_up)
        grads[2 + 2 * n_up], grads[3 + 2 * n_up] = dwo, dbo
        for k in range(n_up - 1, -1, -1):
            hk, wk, r = geo[k]
            rr = r * r
            xin = maps[1 + k]  # m for k == 0, else the previous stage's activated output
            dyv = hip.view_shuffle(hk, wk, r)
            vin = hip.view_plain(hk, wk, 64)
            dwu, dbu = ops._grad_buf(wus[k]), torch.empty(64 * rr, device=dev)
            ops.wgrad_c64(xin, vin, g, dyv, dwu, dbu, B, hk, wk, 64, 64 * rr, shuffle=r)
            gin = ops._empty_cl(B, 64, hk, wk, dev)
            if k > 0:  # the map below is a LeakyReLU output
                ops.conv_c64(g, dyv, ctx.packs[1 + k], None, (1, 64), gin, vin, B, hk, wk, 64 * rr, 64, mask=xin,
                             relu=ops.LEAKY_MASK)
            else:
                ops.conv_c64(g, dyv, ctx.packs[1 + k], None, (1, 64), gin, vin, B, hk, wk, 64 * rr, 64)
            grads[2 + 2 * k], grads[3 + 2 * k] = dwu, dbu
            g = gin
        v64 = hip.view_plain(H, W, 64)
        dwm, dbm = ops._grad_buf(wm), torch.empty(64, device=dev)
        ops.wgrad_c64(maps[0], v64, g, v64, dwm, dbm, B, H, W, 64, 64, owner=wm)
        grads[0], grads[1] = dwm, dbm
        dfea = None
        if ctx.needs_input_grad[0]:
            dfea = ops._empty_cl(B, 64, H, W, dev)
            ops.conv_c64(g, v64, ctx.packs[0], None, (1, 64), dfea, v64, B, H, W, 64, 64)
        return (dfea, None, *grads)


def sftmd_forward(net, x, metadata):
    """The whole SFTMD network (sftmd.SFTMD holds the parameters; ref: SFTMD_variants/architectures.py:161-176).  metadata:
    (B, M, H, W) maps -- or, with q_injection, the (B, M, 1, 1) vectors the reference's handler then supplies (:19-22)."""
    ops._fp32_only("SFTMD")
    B, _, H, W = x.shape
    if metadata.device != x.device:
        # concat_strategy: the handler concatenates the maps to the input on the host and hands the network the host copy
        # (ref: attention_manipulators/__init__.py:94-98 moves them only when they are NOT concatenated)
        metadata = metadata.to(x.device)
    if net.uses_maps:
        if metadata.dim() != 4 or metadata.shape[0] != B or metadata.shape[1] != net.para or tuple(metadata.shape[2:]) != (H, W):
            raise RuntimeError(f"SFTMD: metadata maps must be (B, {net.para}, H, W); got {tuple(metadata.shape)}")
        maps = metadata.detach().float()
        if net.repeats is not None:
            maps = maps.repeat(1, net.repeats, 1, 1)  # input formatting (ref: StandardSft.forward :46-47)
        md = ops.nchw_to_nhwc_pad(maps, 64)
    else:  # the SFT layers never look at the maps: a zero map stands in for the (all-zero-weight) metadata chunk
        md = ops._empty_cl(B, 64, H, W, x.device).zero_()
    q = net.q_injection
    if q and (metadata.dim() != 4 or tuple(metadata.shape[1:]) != (net.para, 1, 1)):
        raise RuntimeError(f"SFTMD with q_injection: metadata must be (B, {net.para}, 1, 1) vectors; got {tuple(metadata.shape)}")
    fea_bef = _SftmdHead.apply(x, net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias, net.conv3.weight,
                               net.conv3.bias)
    fea = fea_bef
    for blk in net.blocks():
        f1 = sft_apply(fea, md, blk.sft1, True)
        if q:
            f1 = ops.gate_mul(f1, blk.q_1.gate(metadata))
        f2 = sft_apply(ops.conv3x3(f1, blk.conv1.weight, blk.conv1.bias), md, blk.sft2, True)
        if q:
            f2 = ops.gate_mul(f2, blk.q_2.gate(metadata))
        fea = ops.conv3x3(f2, blk.conv2.weight, blk.conv2.bias, residual=fea)
    fea_fin = sft_apply(ops.add_residual(fea, fea_bef), md, net.sft, False)
    if q:
        fea_fin = ops.gate_mul(fea_fin, net.final_injection.gate(metadata))
    convs = [m for m in net.upscale if isinstance(m, torch.nn.Conv2d)]
    params = [net.conv_mid.weight, net.conv_mid.bias]
    for c in convs:
        params += [c.weight, c.bias]
    params += [net.conv_output.weight, net.conv_output.bias]
    return _SftmdTail.apply(fea_fin, len(convs), *params)
