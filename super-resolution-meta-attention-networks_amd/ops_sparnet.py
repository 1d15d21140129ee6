"""SPARNet's operators over ops.py's core (csrc/sparnet.hip): the reflection / nearest-upsampling convs, norms, activations,
the attention combines and the RGB shuffle.  The switches REFL_GEO and REFL_BATCH live in ops.py with every other switch.
Reaches the core as ops.NAME at call time (the access rule at the top of ops.py); ops re-exports the operators."""
import torch
from torch.autograd import Function

from . import hip, ops


# ----------------------------------------------------------------------------- SPARNet pieces (csrc/sparnet.hip)
def _padded_packs(weight, cop, cip, need_dgrad):
    """(forward packing, input-gradient packing | None) of `weight` zero-padded to (cop, cip, 3, 3): the step-level packing
    when the handler has run pack_all (the padding is part of that one launch), else pad + pack here."""
    hit = ops._step_pack(weight, 1)
    if hit is not None and hit[0].numel() - cop * cip * 9 in (0, ops.WINOGRAD_FLOATS):  # the Winograd transform may follow
        return hit[0], (hit[1] if need_dgrad else None)
    wp = ops._pad_oihw(weight, cop, cip)
    if need_dgrad:
        return ops.pack_pair(wp)
    return ops.pack_weight(wp, "fwd"), None


class _ReflConv(Function):
    """The conv of one reference ConvLayer as one autograd node (ref: SPARNet/blocks.py:69-103):
    [nearest x2] -> ReflectionPad2d(1) -> Conv2d(3x3, stride 1 | 2, no padding).  x: channels-last map zero-padded to a
    multiple of 64 channels; weight / bias keep their reference shapes (zero-padded per call); y: (B, pad64(cout), Ho, Wo).
    The padded, upsampled map is materialised by one gather; the zero-padded MFMA conv over it equals the reference's conv on
    its interior, which a second gather takes (every stride-th pixel).  Backward: the adjoint gathers around the MFMA
    input-gradient / weight-gradient kernels on the padded geometry."""

    @staticmethod
    def forward(ctx, x, weight, bias, up, stride):
        B, Cp, H, W = x.shape
        co, ci = weight.shape[0], weight.shape[1]
        if Cp % 64 or ci > Cp or tuple(weight.shape[2:]) != (3, 3):
            raise NotImplementedError(f"reflection-padded conv: 3x3 weights on a 64-multiple map (got {tuple(weight.shape)} on {Cp})")
        if H < 2 or W < 2:
            raise NotImplementedError("ReflectionPad2d(1) needs at least 2 x 2 pixels")
        dev, L = x.device, hip.lib()
        x = ops._cl(x)
        cop = ops._pad64(co)
        ctx.geo = ops.REFL_GEO and stride == 1 and up in (1, 2) and ops.PRECISION == "fp32"
        if ctx.geo:
            # reflection / nearest upsampling as address arithmetic of the conv's own staging: no padded copy, no ring of
            # throw-away outputs, no crop (csrc/conv3x3_mfma.hip GEO); channels >= ci of a 64-channel input are zero padding
            # and their octets of the K loop are skipped
            Hv, Wv = up * H, up * W
            pf, ctx.pd = _padded_packs(weight, cop, Cp, ctx.needs_input_grad[0])
            bp = ops._pad_oihw(bias.reshape(co, 1), cop, 1).reshape(cop) if bias is not None else None
            y = ops._empty_cl(B, cop, Hv, Wv, dev)
            hip.check(L.sisr_conv3x3_c64_geo(hip.ptr(x), hip.view_plain(H, W, Cp), ops._wptr(pf), hip.ptr(bp), hip.ptr(y),
                                             hip.view_plain(Hv, Wv, cop), None, B, Hv, Wv, Cp, cop, 1, up - 1,
                                             ci if Cp == 64 else 0, hip.stream()), "sisr_conv3x3_c64_geo")
            ctx.save_for_backward(x, weight)
            ctx.bias = bias
            ctx.geom = (B, H, W, Cp, cop, Hv, Wv, up, stride)
            return y
        Hp, Wp = up * H + 2, up * W + 2
        ctx.s2 = ops.REFL_GEO and stride == 2 and up == 1 and ops.PRECISION == "fp32"
        if ctx.s2:
            # the stride-2 conv computed at its output pixels (a quarter of the stride-1 arithmetic, no gathers).  The backward
            # pass still runs on the padded geometry: it rebuilds the padded map there instead of keeping it
            pf, ctx.pd = _padded_packs(weight, cop, Cp, ctx.needs_input_grad[0])
            bp = ops._pad_oihw(bias.reshape(co, 1), cop, 1).reshape(cop) if bias is not None else None
            Ho, Wo = (H + 1) // 2, (W + 1) // 2
            y = ops._empty_cl(B, cop, Ho, Wo, dev)
            hip.check(L.sisr_conv3x3_c64_geo(hip.ptr(x), hip.view_plain(H, W, Cp), ops._wptr(pf), hip.ptr(bp), hip.ptr(y),
                                             hip.view_plain(Ho, Wo, cop), None, B, H, W, Cp, cop, 3, 0,
                                             ci if Cp == 64 else 0, hip.stream()), "sisr_conv3x3_c64_geo(stride 2)")
            ctx.save_for_backward(x, weight)
            ctx.bias = bias
            ctx.geom = (B, H, W, Cp, cop, Hp, Wp, up, stride)
            return y
        xp = ops._empty_cl(B, Cp, Hp, Wp, dev)
        hip.check(L.sisr_pad_reflect_up(hip.ptr(x), hip.ptr(xp), B, H, W, Cp, up, 0, hip.stream()), "sisr_pad_reflect_up")
        wp = ops._pad_oihw(weight, cop, Cp)
        bp = ops._pad_oihw(bias.reshape(co, 1), cop, 1).reshape(cop) if bias is not None else None
        if ctx.needs_input_grad[0]:
            pf, ctx.pd = ops.pack_pair(wp)
        else:
            pf, ctx.pd = ops.pack_weight(wp, "fwd"), None
        yf = ops._empty_cl(B, cop, Hp, Wp, dev)
        ops.conv_c64(xp, hip.view_plain(Hp, Wp, Cp), pf, bp, (1, 64), yf, hip.view_plain(Hp, Wp, cop), B, Hp, Wp, Cp, cop)
        Ho, Wo = (Hp - 3) // stride + 1, (Wp - 3) // stride + 1
        y = ops._empty_cl(B, cop, Ho, Wo, dev)
        hip.check(L.sisr_crop_stride(hip.ptr(yf), hip.ptr(y), B, Hp, Wp, cop, stride, 0, hip.stream()), "sisr_crop_stride")
        ctx.save_for_backward(xp, weight)
        ctx.bias = bias
        ctx.geom = (B, H, W, Cp, cop, Hp, Wp, up, stride)
        return y

    @staticmethod
    def backward(ctx, dy):
        xp, weight = ctx.saved_tensors
        B, H, W, Cp, cop, Hp, Wp, up, stride = ctx.geom
        dev, L = dy.device, hip.lib()
        dy = ops._cl(dy)
        if ctx.geo or ctx.s2:
            x, (co, ci) = xp, tuple(weight.shape[:2])
            if ctx.geo:    # stride 1: saved geometry holds the conv's (= dy's) grid
                Hv, Wv, Hd, Wd, tmode, wup = Hp, Wp, Hp, Wp, 2, up - 1
            else:          # stride 2: the grid is the input's; dy has every second pixel of it and is read zero-stuffed
                Hv, Wv, Hd, Wd, tmode, wup = H, W, (H + 1) // 2, (W + 1) // 2, 4, 2
            dx = dw = db = None
            if ctx.needs_input_grad[0]:
                # gradient of the padded map: the transposed conv, two pixels larger than the grid, straight from dy (no embedding
                # into a zero map); then the reflection / upsampling folded back
                dxp = ops._empty_cl(B, Cp, Hv + 2, Wv + 2, dev)
                hip.check(L.sisr_conv3x3_c64_geo(hip.ptr(dy), hip.view_plain(Hd, Wd, cop), ops._wptr(ctx.pd), None, hip.ptr(dxp),
                                                 hip.view_plain(Hv + 2, Wv + 2, Cp), None, B, Hv + 2, Wv + 2, cop, Cp, tmode, 0,
                                                 co if cop == 64 else 0, hip.stream()), "sisr_conv3x3_c64_geo(transposed)")
                dx = ops._empty_cl(B, Cp, H, W, dev)
                hip.check(L.sisr_pad_reflect_up(hip.ptr(dxp), hip.ptr(dx), B, H, W, Cp, up, 1, hip.stream()), "sisr_pad_reflect_up(adjoint)")
            has_b = ctx.bias is not None
            if ctx.needs_input_grad[1] or (has_b and ctx.needs_input_grad[2]):
                dw = ops._grad_buf(weight)
                db = ops._grad_buf(ctx.bias) if has_b else None
                # 32 x 32-channel blocks of the gradient that hold real channels (the others: zero padding of the maps)
                units, n_in, n_out = 0, Cp // 64, cop // 64
                for cc in range(n_in):
                    for cq in range(n_out):
                        for cih in range(2):
                            for coh in range(2):
                                if cc * 64 + cih * 32 < ci and cq * 64 + coh * 32 < co:
                                    units |= 1 << ((cc * n_out + cq) * 4 + cih * 2 + coh)
                if units == (1 << (n_in * n_out * 4)) - 1 or n_in * n_out * 4 > 64:
                    units = 0
                # small launches (fewer 8 x 32-pixel tiles than half the CUs) inside a deferred_wgrads() block: queued, eight per
                # launch when the block closes
                tiles = B * ((Hv + 7) // 8) * ((Wv + 31) // 32) * n_in * n_out
                owners = (weight, ctx.bias) if has_b else (weight,)
                if (ops.REFL_BATCH and ops._DEFERRED is not None and hip.stream() == ops._DEFERRED_STREAM and tiles < 128 and
                        all(o.requires_grad and o.grad is None and o.data_ptr() not in ops._PASS_SHARED for o in owners)):
                    if id(weight) in ops._DEFERRED_OWNERS:
                        ops._flush_deferred()  # second gradient of one weight in this pass: the first must be written first
                    else:
                        ops._DEFERRED_OWNERS.add(id(weight))
                        q = ops._DEFERRED.get(("geo", dev.index))
                        if q is None:
                            q = ops._DEFERRED[("geo", dev.index)] = ops.WgradGeoQueue(dev)
                        q.add(x, dy, dw, db, (B, Hv, Wv, Cp, cop, wup, co, ci), units, tiles)
                        return dx, dw, db, None, None
                nbytes = L.sisr_wgrad3x3_c64_workspace_bytes(B, Hv, Wv, Cp, cop)
                ws = hip.workspace(dev, nbytes)
                hip.check(L.sisr_wgrad3x3_c64_geo(hip.ptr(x), hip.view_plain(H, W, Cp), hip.ptr(dy), hip.view_plain(Hd, Wd, cop),
                                                  hip.ptr(dw), co, ci, hip.ptr(db), hip.ptr(ws), nbytes, B, Hv, Wv, Cp, cop,
                                                  wup, units, hip.stream()), "sisr_wgrad3x3_c64_geo")
            return dx, dw, db, None, None
        dyf = ops._empty_cl(B, cop, Hp, Wp, dev)
        hip.check(L.sisr_crop_stride(hip.ptr(dy), hip.ptr(dyf), B, Hp, Wp, cop, stride, 1, hip.stream()), "sisr_crop_stride(embed)")
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dxp = ops._empty_cl(B, Cp, Hp, Wp, dev)
            ops.conv_c64(dyf, hip.view_plain(Hp, Wp, cop), ctx.pd, None, (1, 64), dxp, hip.view_plain(Hp, Wp, Cp), B, Hp, Wp, cop, Cp)
            dx = ops._empty_cl(B, Cp, H, W, dev)
            hip.check(L.sisr_pad_reflect_up(hip.ptr(dxp), hip.ptr(dx), B, H, W, Cp, up, 1, hip.stream()), "sisr_pad_reflect_up(adjoint)")
        if ctx.needs_input_grad[1] or (ctx.bias is not None and ctx.needs_input_grad[2]):
            padded = (cop, Cp) != tuple(weight.shape[:2])
            dwp = torch.empty((cop, Cp, 3, 3), device=dev) if padded else ops._grad_buf(weight)
            has_b = ctx.bias is not None
            dbp = (torch.empty(cop, device=dev) if padded else ops._grad_buf(ctx.bias)) if has_b else None
            ops.wgrad_c64(xp, hip.view_plain(Hp, Wp, Cp), dyf, hip.view_plain(Hp, Wp, cop), dwp, dbp, B, Hp, Wp, Cp, cop)
            dw = ops._crop_oihw(dwp, tuple(weight.shape))
            if has_b:
                co = weight.shape[0]
                db = ops._crop_oihw(dbp.reshape(-1, 1), (co, 1)).reshape(co)
        return dx, dw, db, None, None


def refl_conv(x, weight, bias=None, up=1, stride=1):
    return _ReflConv.apply(x, weight, bias, int(up), int(stride))


class _BatchNormAct(Function):
    """LeakyReLU(slope)(BatchNorm2d(x)) on a channels-last map whose channels >= C_real are zero padding (ref: NormLayer +
    ReluLayer, SPARNet/blocks.py:10-66; slope 1 = no activation).  training: batch statistics, running statistics updated in
    place as torch does; else the running statistics (forward only)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, slope):
        B, C, H, W = x.shape
        Cr = gamma.shape[0]
        if C % 64 or Cr > C or C > 256:
            raise NotImplementedError("batch norm kernels: a 64-multiple map of at most 256 channels")
        dev, L = x.device, hip.lib()
        x = ops._cl(x)
        y = torch.empty_like(x)
        npix = B * H * W
        nbytes = L.sisr_bn_workspace_bytes(npix, C)
        ws = hip.workspace(dev, nbytes)
        mean, invstd = (torch.empty(C, device=dev), torch.empty(C, device=dev)) if training else (None, None)
        g, b = gamma.contiguous(), beta.contiguous()
        hip.check(L.sisr_bn_act_fwd(hip.ptr(x), hip.ptr(y), hip.ptr(g), hip.ptr(b), hip.ptr(running_mean),
                                    hip.ptr(running_var), hip.ptr(mean), hip.ptr(invstd), npix, C, Cr, int(training),
                                    float(momentum), float(eps), float(slope), hip.ptr(ws), nbytes, hip.stream()),
                  "sisr_bn_act_fwd")
        ctx.training, ctx.slope, ctx.geom = training, slope, (npix, C, Cr)
        if training:
            ctx.save_for_backward(x, g, b, mean, invstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.training:
            raise NotImplementedError("batch norm backward in eval mode (running statistics) is not built: the reference "
                                      "trains in train() mode and evaluates under no_grad")
        x, g, b, mean, invstd = ctx.saved_tensors
        npix, C, Cr = ctx.geom
        dev, L = dy.device, hip.lib()
        dy = ops._cl(dy)
        dx = torch.empty_like(x)
        dg, db = torch.empty(Cr, device=dev), torch.empty(Cr, device=dev)
        nbytes = L.sisr_bn_workspace_bytes(npix, C)
        ws = hip.workspace(dev, nbytes)
        hip.check(L.sisr_bn_act_bwd(hip.ptr(x), hip.ptr(dy), hip.ptr(g), hip.ptr(b), hip.ptr(mean), hip.ptr(invstd),
                                    hip.ptr(dx), hip.ptr(dg), hip.ptr(db), npix, C, Cr, float(ctx.slope), hip.ptr(ws), nbytes,
                                    hip.stream()), "sisr_bn_act_bwd")
        return dx, dg, db, None, None, None, None, None, None


def batch_norm_act(x, bn, slope=1.0):
    """bn: an nn.BatchNorm2d (parameter / buffer holder); slope: LeakyReLU slope folded in (1 = none)."""
    training = bn.training or bn.running_mean is None
    if bn.training and bn.num_batches_tracked is not None and not getattr(bn, "_sisr_counted_by_net", False):
        bn.num_batches_tracked += 1  # as nn.BatchNorm2d.forward does (momentum is a number here: the average is exponential)
    if bn.momentum is None:
        raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative average) is not built")
    return _BatchNormAct.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bool(training), float(bn.momentum),
                               float(bn.eps), float(slope))


class _NearestUp(Function):
    """nn.Upsample(scale_factor=up, mode='nearest') on a channels-last map (ref: advanced/SRMD_blocks.py:58-63)."""

    @staticmethod
    def forward(ctx, x, up):
        B, C, H, W = x.shape
        x = ops._cl(x)
        y = ops._empty_cl(B, C, H * up, W * up, x.device)
        hip.check(hip.lib().sisr_nearest_up(hip.ptr(x), hip.ptr(y), B, H, W, C, up, 0, hip.stream()), "sisr_nearest_up")
        ctx.geom = (B, C, H, W, up)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W, up = ctx.geom
        dy = ops._cl(dy)
        dx = ops._empty_cl(B, C, H, W, dy.device)
        hip.check(hip.lib().sisr_nearest_up(hip.ptr(dy), hip.ptr(dx), B, H, W, C, up, 1, hip.stream()), "sisr_nearest_up(adjoint)")
        return dx, None


def nearest_up(x, up):
    return _NearestUp.apply(x, int(up))


def instance_norm_act(x, norm, slope=1.0):
    """LeakyReLU(slope)(InstanceNorm2d(x)) (ref: advanced/SRMD_blocks.py:44-45 'I': nn.InstanceNorm2d(affine=True), statistics per
    sample and channel over H x W, in train() and eval() alike -- it tracks no running statistics).  Instance norm of a batch =
    batch norm of each sample on its own: the batch-norm kernels run once per sample (the affine parameters' gradients add up
    over the samples in autograd), and the normalised samples are concatenated."""
    if getattr(norm, "track_running_stats", False):
        raise NotImplementedError("InstanceNorm2d(track_running_stats=True) is not built")
    eps = float(norm.eps)
    outs = [_BatchNormAct.apply(x[b:b + 1], norm.weight, norm.bias, None, None, True, 0.0, eps, float(slope))
            for b in range(x.shape[0])]
    return outs[0] if len(outs) == 1 else torch.cat(outs, 0)


class _SparCombine(Function):
    """out = identity + x * sigmoid(logits[:, 0])  (ref: HourGlassBlock.forward, SPARNet/blocks.py:236-243, and the residual sum
    of ResidualBlock.forward :166).  logits: the 64 -> 1 attention conv's zero-padded 64-channel result."""

    @staticmethod
    def forward(ctx, x, logits, identity):
        B, C, H, W = x.shape
        dev, L = x.device, hip.lib()
        x, logits = ops._cl(x), ops._cl(logits)
        idn = ops._cl(identity) if identity is not None else None
        y = torch.empty_like(x)
        att = torch.empty(B * H * W, device=dev)
        hip.check(L.sisr_spar_combine_fwd(hip.ptr(x), hip.ptr(logits), hip.ptr(idn), hip.ptr(y), hip.ptr(att), B * H * W, C,
                                          logits.shape[1], hip.stream()), "sisr_spar_combine_fwd")
        ctx.save_for_backward(x, att)
        ctx.cl, ctx.has_idn = logits.shape[1], identity is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, att = ctx.saved_tensors
        B, C, H, W = x.shape
        dev, L = dy.device, hip.lib()
        dy = ops._cl(dy)
        dx = torch.empty_like(x)
        dl = ops._empty_cl(B, ctx.cl, H, W, dev)
        hip.check(L.sisr_spar_combine_bwd(hip.ptr(dy), hip.ptr(x), hip.ptr(att), hip.ptr(dx), hip.ptr(dl), B * H * W, C, ctx.cl,
                                          hip.stream()), "sisr_spar_combine_bwd")
        return dx, dl, (dy if ctx.has_idn else None)


def spar_combine(x, logits, identity=None):
    return _SparCombine.apply(x, logits, identity)


# ---- SPARNet's non-default ConvLayer options (csrc/sparnet.hip, "non-default ConvLayer options")
class _GroupNorm(Function):
    """InstanceNorm2d(affine) (cg = 1) / GroupNorm(32, C) (cg = C / 32) on a channels-last map whose channels >= C_real are zero
    padding (ref: SPARNet/blocks.py:21-24)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, cg, eps):
        B, C, H, W = x.shape
        Cr = gamma.shape[0]
        if Cr > C or Cr % cg:
            raise NotImplementedError(f"group statistics over groups of {cg} channels of {Cr}")
        dev, L = x.device, hip.lib()
        x = ops._cl(x)
        y = torch.empty_like(x)
        mean, inv = torch.empty(B * (Cr // cg), device=dev), torch.empty(B * (Cr // cg), device=dev)
        g, b = gamma.contiguous(), beta.contiguous()
        hip.check(L.sisr_group_norm_fwd(hip.ptr(x), hip.ptr(y), hip.ptr(g), hip.ptr(b), hip.ptr(mean), hip.ptr(inv), B, H * W, C, Cr,
                                        cg, float(eps), hip.stream()), "sisr_group_norm_fwd")
        ctx.save_for_backward(x, g, mean, inv)
        ctx.geom = (B, C, H, W, Cr, cg)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, g, mean, inv = ctx.saved_tensors
        B, C, H, W, Cr, cg = ctx.geom
        dev, L = dy.device, hip.lib()
        dy = ops._cl(dy)
        dx = torch.empty_like(x)
        dgb, dbb = torch.empty((B, Cr), device=dev), torch.empty((B, Cr), device=dev)
        hip.check(L.sisr_group_norm_bwd(hip.ptr(x), hip.ptr(dy), hip.ptr(g), hip.ptr(mean), hip.ptr(inv), hip.ptr(dx), hip.ptr(dgb),
                                        hip.ptr(dbb), B, H * W, C, Cr, cg, hip.stream()), "sisr_group_norm_bwd")
        dg, db = torch.empty(Cr, device=dev), torch.empty(Cr, device=dev)
        for part, out in ((dgb, dg), (dbb, db)):  # the samples' sums added in batch order
            hip.check(L.sisr_sum_partials(hip.ptr(part), B, 1, Cr, 1.0, hip.ptr(out), hip.stream()), "sisr_sum_partials")
        return dx, dg, db, None, None


def group_norm(x, gamma, beta, cg, eps=1e-5):
    return _GroupNorm.apply(x, gamma, beta, int(cg), float(eps))


class _PixelNorm(Function):
    """F.normalize(x, p = 2, dim = 1) on a channels-last map (ref: SPARNet/blocks.py:25-26)."""

    @staticmethod
    def forward(ctx, x):
        B, C, H, W = x.shape
        x = ops._cl(x)
        y = torch.empty_like(x)
        hip.check(hip.lib().sisr_pixel_norm(hip.ptr(x), None, hip.ptr(y), B * H * W, C, 0, hip.stream()), "sisr_pixel_norm")
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        B, C, H, W = x.shape
        dy = ops._cl(dy)
        dx = torch.empty_like(x)
        hip.check(hip.lib().sisr_pixel_norm(hip.ptr(x), hip.ptr(dy), hip.ptr(dx), B * H * W, C, 1, hip.stream()), "sisr_pixel_norm(bwd)")
        return dx


def pixel_norm(x):
    return _PixelNorm.apply(x)


class _Act(Function):
    """PReLU(C) (mode 0, slope: the module's weight) / SELU (mode 1) on a channels-last map (ref: SPARNet/blocks.py:55-58)."""

    @staticmethod
    def forward(ctx, x, slope, mode):
        B, C, H, W = x.shape
        x = ops._cl(x)
        y = torch.empty_like(x)
        a = slope.contiguous() if slope is not None else None
        if a is not None and a.shape[0] > C:
            raise NotImplementedError("PReLU slope count above the map's channels")
        if a is not None and a.shape[0] == 1 and C != 1:
            a = a.expand(C).contiguous()  # nn.PReLU(1): one slope for every channel
        hip.check(hip.lib().sisr_act(hip.ptr(x), None, hip.ptr(a), hip.ptr(y), None, B * H * W, C, a.shape[0] if a is not None else C,
                                     mode, 0, hip.stream()), "sisr_act")
        ctx.save_for_backward(x, a)
        ctx.mode, ctx.n_slope = mode, (slope.shape[0] if slope is not None else 0)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, a = ctx.saved_tensors
        B, C, H, W = x.shape
        dev, L = dy.device, hip.lib()
        dy = ops._cl(dy)
        dx = torch.empty_like(x)
        dyx = torch.empty_like(x) if ctx.mode == 0 else None
        hip.check(L.sisr_act(hip.ptr(x), hip.ptr(dy), hip.ptr(a), hip.ptr(dx), hip.ptr(dyx), B * H * W, C,
                             a.shape[0] if a is not None else C, ctx.mode, 1, hip.stream()), "sisr_act(bwd)")
        da = None
        if ctx.mode == 0 and ctx.needs_input_grad[1]:
            part, parts = ops._pixel_sums(dyx, None, B, H, W, C)  # [B][parts][C] ordered sums of dy * min(x, 0)
            per = torch.empty(C, device=dev)
            hip.check(L.sisr_sum_partials(hip.ptr(part), B * parts, 1, C, 1.0, hip.ptr(per), hip.stream()), "sisr_sum_partials")
            da = per[:a.shape[0]] if ctx.n_slope != 1 else per[:a.shape[0]].sum().reshape(1)
        return dx, da, None


def prelu(x, slope):
    return _Act.apply(x, slope, 0)


def selu(x):
    return _Act.apply(x, None, 1)


_const_slopes = {}


def leaky_relu(x, slope):
    """LeakyReLU(slope) (0: ReLU) as the PReLU kernel with a constant slope vector -- the activation behind a norm other than
    batch norm (behind batch norm it is part of the batch-norm kernel)."""
    key = (x.device.index, x.shape[1], float(slope))
    a = _const_slopes.get(key)
    if a is None:
        a = _const_slopes[key] = torch.full((x.shape[1],), float(slope), device=x.device)
    return _Act.apply(x, a, 0)


class _Spar3d(Function):
    """identity + x * sigmoid(logits), one logit per element (ref: SPARNet/blocks.py:147-151 att_name 'spar3d', :241-243)."""

    @staticmethod
    def forward(ctx, x, logits, identity):
        x, logits = ops._cl(x), ops._cl(logits)
        idn = ops._cl(identity) if identity is not None else None
        y = torch.empty_like(x)
        hip.check(hip.lib().sisr_spar3d(hip.ptr(x), hip.ptr(logits), hip.ptr(idn), hip.ptr(y), None, x.numel(), 0, hip.stream()),
                  "sisr_spar3d")
        ctx.save_for_backward(x, logits)
        ctx.has_idn = identity is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, logits = ctx.saved_tensors
        dy = ops._cl(dy)
        dx, dl = torch.empty_like(x), torch.empty_like(x)
        hip.check(hip.lib().sisr_spar3d(hip.ptr(x), hip.ptr(logits), hip.ptr(dy), hip.ptr(dx), hip.ptr(dl), x.numel(), 1, hip.stream()),
                  "sisr_spar3d(bwd)")
        return dx, dl, (dy if ctx.has_idn else None)


def spar_combine3d(x, logits, identity=None):
    return _Spar3d.apply(x, logits, identity)


class _ShuffleRGB(Function):
    """PixelShuffle(r) of the first C r^2 channels of a channels-last map into an NCHW (B, C, rH, rW) image."""

    @staticmethod
    def forward(ctx, y, C, r):
        B, Cp, H, W = y.shape
        y = ops._cl(y)
        out = torch.empty((B, C, H * r, W * r), device=y.device, dtype=torch.float32)
        hip.check(hip.lib().sisr_shuffle_rgb(hip.ptr(y), hip.ptr(out), B, C, r, H, W, Cp, 0, hip.stream()), "sisr_shuffle_rgb")
        ctx.geo = (B, C, r, H, W, Cp)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, C, r, H, W, Cp = ctx.geo
        dy = ops._empty_cl(B, Cp, H, W, dout.device)
        hip.check(hip.lib().sisr_shuffle_rgb(hip.ptr(dout.contiguous()), hip.ptr(dy), B, C, r, H, W, Cp, 1, hip.stream()),
                  "sisr_shuffle_rgb(adjoint)")
        return dy, None, None


def shuffle_rgb(y, channels, r):
    return _ShuffleRGB.apply(y, int(channels), int(r))
