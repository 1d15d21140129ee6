"""Attention operators over ops.py's core: the stand-alone gates (CALayer, gate multiply, pooling, PALayer, residual add),
HAN's layer / channel-spatial attention and map stacks, SAN's second-order channel attention and non-local blocks.
Reaches the core as ops.NAME at call time (the access rule at the top of ops.py); ops re-exports the operators."""
import torch
from torch.autograd import Function

from . import hip, ops


# ----------------------------------------------------------------------------- stand-alone gates
class _CALayer(Function):
    """y = x * sigmoid(W2 relu(W1 mean_hw(x) + b1) + b2)   (ref: advanced/architectures.py:29-32)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        B, C, H, W = x.shape
        if C != 64:
            raise NotImplementedError("channel attention kernels are specialised for 64 channels")
        x = ops._cl(x)
        dev = x.device
        R = w1.shape[0]
        w1c, w2c = w1.reshape(R, 64).contiguous(), w2.reshape(64, R).contiguous()
        part, parts = ops._pixel_sums(x, None, B, H, W)
        s, hid, ca, g = ops._vec(B, 64, dev), ops._vec(B, R, dev), ops._vec(B, 64, dev), ops._vec(B, 64, dev)
        hip.check(hip.lib().sisr_ca_gate_fwd(hip.ptr(part), parts, B, 1.0 / (H * W), hip.ptr(w1c),
                                             hip.ptr_c(b1), hip.ptr(w2c), hip.ptr_c(b2), 64, R,
                                             None, hip.ptr(s), hip.ptr(hid), hip.ptr(ca), hip.ptr(g), hip.stream()),
                  "sisr_ca_gate_fwd")
        ctx.save_for_backward(x, w1c, w2c, s, hid, ca)
        ctx.shapes = (w1.shape, w2.shape)
        return ops._affine(x, g, None, None, B, H, W, 64)

    @staticmethod
    def backward(ctx, dy):
        x, w1c, w2c, s, hid, ca = ctx.saved_tensors
        B, C, H, W = x.shape
        dev = x.device
        R = w1c.shape[0]
        dy = ops._cl(dy)
        dgp, parts = ops._pixel_sums(dy, x, B, H, W)
        shift = ops._vec(B, 64, dev)
        dw1, db1 = torch.empty_like(w1c), torch.empty(R, device=dev)
        dw2, db2 = torch.empty_like(w2c), torch.empty(64, device=dev)
        hip.check(hip.lib().sisr_ca_gate_bwd(hip.ptr(dgp), parts, B, 1.0 / (H * W), hip.ptr(w1c), hip.ptr(w2c), 64, R,
                                             hip.ptr(s), hip.ptr(hid), hip.ptr(ca), None, hip.ptr(shift), None,
                                             hip.ptr(dw1), hip.ptr(db1), hip.ptr(dw2), hip.ptr(db2),
                                             hip.ptr(ops._gate_ws(B, dev)), hip.gate_counter(dev), hip.stream()),
                  "sisr_ca_gate_bwd")
        dx = ops._affine(dy, ca, shift, None, B, H, W, 64)
        return dx, dw1.reshape(ctx.shapes[0]), db1, dw2.reshape(ctx.shapes[1]), db2


def ca_layer(x, w1, b1, w2, b2):
    if x.shape[1] != 64:  # wider maps: pooled sums + the generic gate MLP + gate multiply (see _wide_gated_block)
        B, C = x.shape[0], x.shape[1]
        g = ops._GateMlp.apply(global_avg_pool(x), x.new_zeros((B, 1, 1, 1)), None, ([(0, 0, 1), (0, 0, 2)], 0), w1, b1, w2, b2)
        return gate_mul(x, g.reshape(B, C, 1, 1))
    return _CALayer.apply(x, w1, b1, w2, b2)


class _GateMul(Function):
    """y = t * g[b,c] (+ x)."""

    @staticmethod
    def forward(ctx, t, g, x):
        B, C, H, W = t.shape
        t = ops._cl(t)
        g2 = g.reshape(B, C).contiguous()
        y = ops._affine(t, g2, None, ops._cl(x) if x is not None else None, B, H, W, C)
        ctx.save_for_backward(t, g2)
        ctx.gshape, ctx.has_x = g.shape, x is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        t, g2 = ctx.saved_tensors
        B, C, H, W = t.shape
        if C % 64:
            raise NotImplementedError("gate backward needs a multiple of 64 channels")
        dy = ops._cl(dy)
        dt = ops._affine(dy, g2, None, None, B, H, W, C)
        dgp, parts = ops._pixel_sums(dy, t, B, H, W, C)
        dg = ops._vec(B, C, t.device)
        hip.check(hip.lib().sisr_sum_partials(hip.ptr(dgp), parts, B, C, 1.0, hip.ptr(dg), hip.stream()),
                  "sisr_sum_partials")
        return dt, dg.reshape(ctx.gshape), (dy if ctx.has_x else None)


def gate_mul(t, g, x=None):
    return _GateMul.apply(t, g, x)


class _GlobalAvgPool(Function):
    """(B,64,H,W) -> (B,64,1,1) mean over pixels (ordered two-stage sum)."""

    @staticmethod
    def forward(ctx, t):
        B, C, H, W = t.shape
        if C % 64:
            raise NotImplementedError("GAP kernel needs a multiple of 64 channels")
        t = ops._cl(t)
        part, parts = ops._pixel_sums(t, None, B, H, W, C)
        s = ops._vec(B, C, t.device)
        hip.check(hip.lib().sisr_sum_partials(hip.ptr(part), parts, B, C, 1.0 / (H * W), hip.ptr(s), hip.stream()),
                  "sisr_sum_partials")
        ctx.geom = (B, C, H, W)
        return s.reshape(B, C, 1, 1)

    @staticmethod
    def backward(ctx, ds):
        B, C, H, W = ctx.geom
        dt = (ds.reshape(B, C, 1, 1) / (H * W)).expand(B, C, H, W).contiguous(memory_format=ops.CL)
        return dt


def global_avg_pool(t):
    return _GlobalAvgPool.apply(t)


class _PALayer(Function):
    """Per-pixel attention gate (ref: attention_manipulators/architectures.py:13-26)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        B, C, H, W = x.shape
        if C != 64 or w1.shape[0] != 8:
            raise NotImplementedError("pixel attention kernel is specialised for 64 channels / 8 hidden units")
        x = ops._cl(x)
        w1c, w2c = w1.reshape(8, 64).contiguous(), w2.reshape(8).contiguous()
        b1c, b2c = b1.contiguous(), b2.reshape(1).contiguous()
        y = ops._empty_cl(B, C, H, W, x.device)
        hip.check(hip.lib().sisr_pa_fwd(hip.ptr(x), hip.ptr(w1c), hip.ptr(b1c), hip.ptr(w2c), hip.ptr(b2c), hip.ptr(y),
                                        B * H * W, 64, 8, hip.stream()), "sisr_pa_fwd")
        ctx.save_for_backward(x, w1c, b1c, w2c, b2c)
        ctx.shapes = (w1.shape, w2.shape, b2.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w1c, b1c, w2c, b2c = ctx.saved_tensors
        B, C, H, W = x.shape
        L = hip.lib()
        dy = ops._cl(dy)
        npix = B * H * W
        ws = hip.workspace(x.device, L.sisr_pa_bwd_workspace_bytes(npix))
        dx = ops._empty_cl(B, C, H, W, x.device)
        dw1, db1 = torch.empty_like(w1c), torch.empty_like(b1c)
        dw2, db2 = torch.empty_like(w2c), torch.empty_like(b2c)
        hip.check(L.sisr_pa_bwd(hip.ptr(x), hip.ptr(w1c), hip.ptr(b1c), hip.ptr(w2c), hip.ptr(b2c), hip.ptr(dy),
                                hip.ptr(dx), hip.ptr(dw1), hip.ptr(db1), hip.ptr(dw2), hip.ptr(db2), hip.ptr(ws), npix,
                                64, 8, hip.stream()), "sisr_pa_bwd")
        s1, s2, sb2 = ctx.shapes
        return dx, dw1.reshape(s1), db1, dw2.reshape(s2), db2.reshape(sb2)


def pa_layer(x, w1, b1, w2, b2):
    return _PALayer.apply(x, w1, b1, w2, b2)


class _AddResidual(Function):
    """y = t + x on channels-last maps."""

    @staticmethod
    def forward(ctx, t, x):
        B, C, H, W = t.shape
        return ops._affine(ops._cl(t), None, None, ops._cl(x), B, H, W, C)

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


def add_residual(t, x):
    return _AddResidual.apply(t, x)


# ----------------------------------------------------------------------------- HAN attention modules
class _LAM(Function):
    """Layer attention over a [B][N][H][W][64] stack (ref: advanced/HAN_blocks.py:16-37)."""

    @staticmethod
    def forward(ctx, stack, gamma):
        B, N = stack.shape[0], stack.shape[1]
        chw = stack[0, 0].numel()
        stack = stack.contiguous()
        L = hip.lib()
        nbytes = L.sisr_lam_workspace_bytes(B, N, chw)
        if nbytes == 0:
            raise NotImplementedError(f"LAM kernel: unsupported shape B={B} N={N} chw={chw}")
        ws = hip.workspace(stack.device, nbytes)
        y = torch.empty_like(stack)
        attn = torch.empty((B, N, N), device=stack.device, dtype=torch.float32)
        g = gamma.reshape(1).contiguous()
        hip.check(L.sisr_lam_fwd(hip.ptr(stack), hip.ptr(g), hip.ptr(y), hip.ptr(attn), hip.ptr(ws), B, N, chw,
                                 hip.stream()), "sisr_lam_fwd")
        ctx.save_for_backward(stack, attn, g)
        ctx.gshape = gamma.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        stack, attn, g = ctx.saved_tensors
        B, N = stack.shape[0], stack.shape[1]
        chw = stack[0, 0].numel()
        L = hip.lib()
        nbytes = L.sisr_lam_workspace_bytes(B, N, chw)
        ws = hip.workspace(stack.device, nbytes)
        dy = dy.contiguous()
        dx = torch.empty_like(stack)
        dg = torch.empty(1, device=stack.device, dtype=torch.float32)
        hip.check(L.sisr_lam_bwd(hip.ptr(stack), hip.ptr(attn), hip.ptr(g), hip.ptr(dy), hip.ptr(dx), hip.ptr(dg),
                                 hip.ptr(ws), B, N, chw, hip.stream()), "sisr_lam_bwd")
        return dx, dg.reshape(ctx.gshape)


def lam(stack, gamma):
    return _LAM.apply(stack, gamma)


class _CSAM(Function):
    """x * (1 + gamma * sigmoid(conv3d(x))) on a channels-last 64-channel map (ref: advanced/HAN_blocks.py:58-76)."""

    @staticmethod
    def forward(ctx, x, w, b, gamma):
        B, C, H, W = x.shape
        if C != 64:
            raise NotImplementedError("CSAM kernel is specialised for 64 channels")
        x = ops._cl(x)
        w27 = w.reshape(27).contiguous()
        bb, g = b.reshape(1).contiguous(), gamma.reshape(1).contiguous()
        y = ops._empty_cl(B, C, H, W, x.device)
        hip.check(hip.lib().sisr_csam_fwd(hip.ptr(x), hip.ptr(w27), hip.ptr(bb), hip.ptr(g), hip.ptr(y), B, H, W, C,
                                          hip.stream()), "sisr_csam_fwd")
        ctx.save_for_backward(x, w27, bb, g)
        ctx.shapes = (w.shape, b.shape, gamma.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w27, bb, g = ctx.saved_tensors
        B, C, H, W = x.shape
        L = hip.lib()
        dy = ops._cl(dy)
        nbytes = L.sisr_csam_bwd_workspace_bytes(B, H, W, C)
        ws = hip.workspace(x.device, nbytes)
        dx = ops._empty_cl(B, C, H, W, x.device)
        dw, db, dg = (torch.empty(n, device=x.device, dtype=torch.float32) for n in (27, 1, 1))
        hip.check(L.sisr_csam_bwd(hip.ptr(x), hip.ptr(w27), hip.ptr(bb), hip.ptr(g), hip.ptr(dy), hip.ptr(dx),
                                  hip.ptr(dw), hip.ptr(db), hip.ptr(dg), hip.ptr(ws), B, H, W, C, hip.stream()),
                  "sisr_csam_bwd")
        sw, sb, sg = ctx.shapes
        return dx, dw.reshape(sw), db.reshape(sb), dg.reshape(sg)


def csam(x, w, b, gamma):
    return _CSAM.apply(x, w, b, gamma)


class _PixelShuffleCL(Function):
    """nn.PixelShuffle(r) of a channels-last map as one gather (upsamplers wider than 64 channels; ref: advanced/common.py:20-45)."""

    @staticmethod
    def forward(ctx, x, r):
        B, Crr, H, W = x.shape
        C = Crr // (r * r)
        if C * r * r != Crr:
            raise RuntimeError(f"PixelShuffle({r}) needs a channel count divisible by {r * r}; got {Crr}")
        y = ops._empty_cl(B, C, H * r, W * r, x.device)
        hip.check(hip.lib().sisr_pixel_shuffle_cl(hip.ptr(ops._cl(x)), hip.ptr(y), B, H, W, C, r, 0, hip.stream()),
                  "sisr_pixel_shuffle_cl")
        ctx.geo = (B, C, H, W, r)
        return y

    @staticmethod
    def backward(ctx, dy):
        B, C, H, W, r = ctx.geo
        dx = ops._empty_cl(B, C * r * r, H, W, dy.device)
        hip.check(hip.lib().sisr_pixel_shuffle_cl(hip.ptr(ops._cl(dy)), hip.ptr(dx), B, H, W, C, r, 1, hip.stream()),
                  "sisr_pixel_shuffle_cl(adjoint)")
        return dx, None


def pixel_shuffle(x, r):
    return _PixelShuffleCL.apply(x, int(r))


class _StackMaps(Function):
    """N channels-last (B, 64, H, W) maps -> the [B][N][H][W][64] stack LAM and the stack convs read as chunks (ref:
    advanced/architectures.py:357-362, the torch.cat of HAN's intermediate maps); backward hands every map its slot."""

    @staticmethod
    def forward(ctx, *maps):
        B, C, H, W = maps[0].shape
        if C != 64:
            raise NotImplementedError("map stacks hold 64-channel maps")
        N = len(maps)
        stack = torch.empty((B, N, H, W, 64), device=maps[0].device, dtype=torch.float32)
        for k, m in enumerate(maps):
            hip.check(hip.lib().sisr_stack_maps(hip.ptr(ops._cl(m)), hip.ptr(stack), B, H * W, N, k, 0, hip.stream()),
                      "sisr_stack_maps")
        return stack

    @staticmethod
    def backward(ctx, dstack):
        B, N, H, W, _ = dstack.shape
        dstack = dstack.contiguous()
        out = []
        for k in range(N):
            if not ctx.needs_input_grad[k]:
                out.append(None)
                continue
            g = ops._empty_cl(B, 64, H, W, dstack.device)
            hip.check(hip.lib().sisr_stack_maps(hip.ptr(dstack), hip.ptr(g), B, H * W, N, k, 1, hip.stream()),
                      "sisr_stack_maps(unstack)")
            out.append(g)
        return tuple(out)


def stack_maps(maps):
    return _StackMaps.apply(*maps)


class _ConvStack(Function):
    """3x3 conv 64*N -> 64 reading a [B][N][H][W][64] map stack as N channel chunks (HAN last_conv /
    last, ref: advanced/architectures.py:349-350,366-371) -- torch.cat is never materialised."""

    @staticmethod
    def forward(ctx, stack, weight, bias, residual=None):
        B, N, H, W, C = stack.shape
        if C != 64 or weight.shape[0] != 64 or weight.shape[1] != 64 * N:
            raise NotImplementedError("stack conv expects N maps of 64 channels -> 64 channels")
        stack = stack.contiguous()
        w = weight.contiguous()
        if ctx.needs_input_grad[0]:
            packed, ctx.pd = ops.pack_pair(w)
        else:
            packed, ctx.pd = ops.pack_weight(w, "fwd"), None
        y = ops._empty_cl(B, 64, H, W, stack.device)
        ops.conv_c64(stack, hip.view_maps(H, W, N), packed, bias, (1, 64), y, hip.view_plain(H, W, 64), B, H, W, 64 * N, 64,
                     res=ops._cl(residual) if residual is not None else None)
        ctx.save_for_backward(stack, w)
        ctx.has_bias, ctx.has_res = bias is not None, residual is not None
        return y

    @staticmethod
    @ops._in_backward
    def backward(ctx, dy):
        stack, w = ctx.saved_tensors
        B, N, H, W, C = stack.shape
        dev = stack.device
        dy = ops._cl(dy)
        dstack = None
        if ctx.needs_input_grad[0]:
            dstack = torch.empty_like(stack)
            ops.conv_c64(dy, hip.view_plain(H, W, 64), ctx.pd, None, (1, 64), dstack, hip.view_maps(H, W, N), B, H, W, 64,
                         64 * N)
        dw = torch.empty_like(w)
        db = torch.empty(64, device=dev, dtype=torch.float32) if ctx.has_bias else None
        ops.wgrad_c64(stack, hip.view_maps(H, W, N), dy, hip.view_plain(H, W, 64), dw, db, B, H, W, 64 * N, 64)
        return dstack, dw, db, (dy if ctx.has_res else None)


def conv3x3_stack(stack, weight, bias, residual=None):
    """conv over the stack's N maps as channel chunks (+ residual, added by the conv's epilogue)."""
    return _ConvStack.apply(stack, weight, bias, residual)


# ----------------------------------------------------------------------------- SAN attention modules
SOCA_LIMIT = 1000  # ref: advanced/SAN_blocks.py:265-266 (h1 = w1 = 1000)
SOCA_ITERS = 5     # ref: advanced/SAN_blocks.py:291 SqrtmLayer(cov_mat, 5)


def soca_window(H, W):
    """Slices of the centre crop SOCA pools over when a side exceeds 1000 (ref: advanced/SAN_blocks.py:267-280,
    strict comparisons and Python slice semantics kept); None when the whole map is used."""
    lim = SOCA_LIMIT
    if H < lim and W < lim:
        return None
    if H < lim and W > lim:
        w0 = (W - lim) // 2
        return slice(None), slice(w0, w0 + lim)
    if W < lim and H > lim:
        h0 = (H - lim) // 2
        return slice(h0, h0 + lim), slice(None)
    h0, w0 = (H - lim) // 2, (W - lim) // 2
    return slice(h0, h0 + lim), slice(w0, w0 + lim)


class _SOCA(Function):
    """Second-order channel attention  y = x * sigmoid(W2 relu(W1 v + b1) + b2),  v = column means of
    sqrtm(cov(x))  (ref: advanced/SAN_blocks.py:261-302; advanced/mpncov.py for cov / sqrtm and their
    hand-written backward, which is what the kernels implement)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        B, C, H, W = x.shape
        if C != 64:
            raise NotImplementedError("SOCA kernels are specialised for 64 channels")
        x = ops._cl(x)
        dev = x.device
        L = hip.lib()
        win = soca_window(H, W)
        xs = x if win is None else x[:, :, win[0], win[1]].contiguous(memory_format=ops.CL)
        hs, ws = xs.shape[2:]
        M = hs * ws
        part, parts = ops._pixel_sums(xs, None, B, hs, ws)
        mean = ops._vec(B, 64, dev)
        hip.check(L.sisr_sum_partials(hip.ptr(part), parts, B, 64, 1.0 / M, hip.ptr(mean), hip.stream()),
                  "sisr_sum_partials")
        cov = torch.empty((B, 64, 64), device=dev, dtype=torch.float32)
        wsp = hip.workspace(dev, L.sisr_covpool_workspace_bytes(B, M))
        hip.check(L.sisr_covpool_fwd(hip.ptr(xs), hip.ptr(mean), hip.ptr(cov), hip.ptr(wsp), B, M, 64, hip.stream()),
                  "sisr_covpool_fwd")
        saved = torch.empty(L.sisr_sqrtm_saved_bytes(B, 64, SOCA_ITERS) // 4, device=dev, dtype=torch.float32)
        pooled = ops._vec(B, 64, dev)
        hip.check(L.sisr_sqrtm_fwd(hip.ptr(cov), hip.ptr(saved), hip.ptr(pooled), B, 64, SOCA_ITERS, hip.stream()),
                  "sisr_sqrtm_fwd")
        R = w1.shape[0]
        w1c, w2c = w1.reshape(R, 64).contiguous(), w2.reshape(64, R).contiguous()
        s, hid, ca, g = ops._vec(B, 64, dev), ops._vec(B, R, dev), ops._vec(B, 64, dev), ops._vec(B, 64, dev)
        hip.check(L.sisr_ca_gate_fwd(hip.ptr(pooled), 1, B, 1.0, hip.ptr(w1c), hip.ptr_c(b1), hip.ptr(w2c),
                                     hip.ptr_c(b2), 64, R, None, hip.ptr(s), hip.ptr(hid), hip.ptr(ca),
                                     hip.ptr(g), hip.stream()), "sisr_ca_gate_fwd")
        ctx.save_for_backward(x, w1c, w2c, s, hid, ca, mean, cov, saved)
        ctx.shapes, ctx.win = (w1.shape, w2.shape), win
        return ops._affine(x, g, None, None, B, H, W, 64)

    @staticmethod
    def backward(ctx, dy):
        x, w1c, w2c, s, hid, ca, mean, cov, saved = ctx.saved_tensors
        B, C, H, W = x.shape
        dev = x.device
        L = hip.lib()
        R = w1c.shape[0]
        dy = ops._cl(dy)
        dgp, parts = ops._pixel_sums(dy, x, B, H, W)
        dpooled = ops._vec(B, 64, dev)
        dw1, db1 = torch.empty_like(w1c), torch.empty(R, device=dev)
        dw2, db2 = torch.empty_like(w2c), torch.empty(64, device=dev)
        hip.check(L.sisr_ca_gate_bwd(hip.ptr(dgp), parts, B, 1.0, hip.ptr(w1c), hip.ptr(w2c), 64, R, hip.ptr(s),
                                     hip.ptr(hid), hip.ptr(ca), None, hip.ptr(dpooled), None, hip.ptr(dw1),
                                     hip.ptr(db1), hip.ptr(dw2), hip.ptr(db2), hip.ptr(ops._gate_ws(B, dev)),
                                     hip.gate_counter(dev), hip.stream()),
                  "sisr_ca_gate_bwd")
        dsym = torch.empty_like(cov)
        hip.check(L.sisr_sqrtm_bwd(hip.ptr(cov), hip.ptr(saved), hip.ptr(dpooled), hip.ptr(dsym), B, 64, SOCA_ITERS,
                                   hip.stream()), "sisr_sqrtm_bwd")
        win = ctx.win
        if win is None:
            dx = ops._empty_cl(B, 64, H, W, dev)
            hip.check(L.sisr_soca_bwd_apply(hip.ptr(dy), hip.ptr(ca), hip.ptr(x), hip.ptr(mean), hip.ptr(dsym),
                                            hip.ptr(dx), B, H * W, 64, hip.stream()), "sisr_soca_bwd_apply")
        else:  # covariance term only inside the pooled window (maps with a side > 1000: evaluation-size inputs)
            dx = ops._affine(dy, ca, None, None, B, H, W, 64)
            xs = x[:, :, win[0], win[1]].contiguous(memory_format=ops.CL)
            hs, ws = xs.shape[2:]
            zero = torch.zeros_like(xs)
            dwin = torch.empty_like(xs)
            hip.check(L.sisr_soca_bwd_apply(hip.ptr(zero), hip.ptr(ca), hip.ptr(xs), hip.ptr(mean), hip.ptr(dsym),
                                            hip.ptr(dwin), B, hs * ws, 64, hip.stream()), "sisr_soca_bwd_apply")
            dx[:, :, win[0], win[1]] += dwin
        return dx, dw1.reshape(ctx.shapes[0]), db1, dw2.reshape(ctx.shapes[1]), db2


def soca(x, w1, b1, w2, b2):
    return _SOCA.apply(x, w1, b1, w2, b2)


class _NonLocalAttention(Function):
    """y_i = sum_j softmax_j(theta_i . phi_j) g_j on [nb][n][8] rows (ref: advanced/SAN_blocks.py:126-141)."""

    @staticmethod
    def forward(ctx, theta, phi, g):
        nb, nq, d = theta.shape
        nk = phi.shape[1]
        theta, phi, g = theta.contiguous(), phi.contiguous(), g.contiguous()
        y = torch.empty_like(theta)
        lse = torch.empty((nb, nq), device=theta.device, dtype=torch.float32)
        hip.check(hip.lib().sisr_nl_attn_fwd(hip.ptr(theta), hip.ptr(phi), hip.ptr(g), hip.ptr(y), hip.ptr(lse), nb, nq,
                                             nk, d, hip.stream()), "sisr_nl_attn_fwd")
        ctx.save_for_backward(theta, phi, g, y, lse)
        return y

    @staticmethod
    def backward(ctx, dy):
        theta, phi, g, y, lse = ctx.saved_tensors
        nb, nq, d = theta.shape
        nk = phi.shape[1]
        dy = dy.contiguous()
        dtheta, dphi, dg = torch.empty_like(theta), torch.empty_like(phi), torch.empty_like(g)
        dsum = torch.empty_like(lse)
        hip.check(hip.lib().sisr_nl_attn_bwd(hip.ptr(theta), hip.ptr(phi), hip.ptr(g), hip.ptr(y), hip.ptr(lse),
                                             hip.ptr(dy), hip.ptr(dtheta), hip.ptr(dphi), hip.ptr(dg), hip.ptr(dsum), nb,
                                             nq, nk, d, hip.stream()), "sisr_nl_attn_bwd")
        return dtheta, dphi, dg


def nonlocal_attention(theta, phi, g):
    return _NonLocalAttention.apply(theta, phi, g)


def _nl_domain_groups(B, H, W, quadrants):
    """Attention domains of a map as groups of equal rectangles (sisr_nl_* `domains` arrays): the whole map, or the four
    quadrants (ref: advanced/SAN_blocks.py:316-334: H // 2, W // 2 split) -- one group when they are equal."""
    import ctypes
    mk = lambda *v: (ctypes.c_int * 9)(*v)  # noqa: E731
    if not quadrants:
        return [(mk(B, H, W, 0, 0, H, W, 1, 1), B, H, W)]
    h1, w1 = H // 2, W // 2
    if H % 2 == 0 and W % 2 == 0:
        return [(mk(B, H, W, 0, 0, h1, w1, 2, 2), 4 * B, h1, w1)]
    return [(mk(B, H, W, y0, x0, hq, wq, 1, 1), B, hq, wq)
            for y0, hq in ((0, h1), (h1, H - h1)) for x0, wq in ((0, w1), (w1, W - w1))]


class _NonLocalBlock(Function):
    """z = W(softmax(theta(x)^T phi(x)) g(x)) + x with phi / g max-pooled 2x2, per attention domain (ref:
    advanced/SAN_blocks.py:104-148, :305-336).  Projections 64 -> 24 and their two gradients on the fp32 matrix cores,
    split / pool / scatter and the 8 -> 64 output projection as streaming kernels (csrc/nonlocal.hip), the attention itself
    csrc/san.hip; nothing here is a library call."""

    @staticmethod
    def forward(ctx, x, quadrants, wt, bt, wp, bp, wg, bg, ww, bw):
        B, C, H, W = x.shape
        if C != 64 or wt.shape[0] != 8 or ww.shape[0] != 64:
            raise NotImplementedError("non-local block kernels: 64 channels, 8 embedding channels (SAN's configuration)")
        L, dev, npix = hip.lib(), x.device, B * H * W
        x = ops._cl(x)
        wt, wp, wg, ww = (t.reshape(t.shape[0], -1).contiguous() for t in (wt, wp, wg, ww))
        proj = torch.empty((npix, 24), device=dev)
        hip.check(L.sisr_nl_project_fwd(hip.ptr(x), hip.ptr(wt), hip.ptr_c(bt), hip.ptr(wp), hip.ptr_c(bp), hip.ptr(wg),
                                        hip.ptr_c(bg), hip.ptr(proj), npix, hip.stream()), "sisr_nl_project_fwd")
        z = ops._empty_cl(B, 64, H, W, dev)
        saved = []
        for dom, nd, hq, wq in _nl_domain_groups(B, H, W, quadrants):
            if hq < 2 or wq < 2:
                raise RuntimeError("non-local block needs at least 2x2 positions per attention domain (MaxPool2d(2))")
            nq, nk = hq * wq, (hq // 2) * (wq // 2)
            theta = torch.empty((nd, nq, 8), device=dev)
            phi, g = torch.empty((nd, nk, 8), device=dev), torch.empty((nd, nk, 8), device=dev)
            hip.check(L.sisr_nl_split_pool_fwd(hip.ptr(proj), hip.ptr(theta), hip.ptr(phi), hip.ptr(g), dom, hip.stream()),
                      "sisr_nl_split_pool_fwd")
            y = torch.empty_like(theta)
            lse = torch.empty((nd, nq), device=dev)
            hip.check(L.sisr_nl_attn_fwd(hip.ptr(theta), hip.ptr(phi), hip.ptr(g), hip.ptr(y), hip.ptr(lse), nd, nq, nk, 8,
                                         hip.stream()), "sisr_nl_attn_fwd")
            hip.check(L.sisr_nl_output_fwd(hip.ptr(y), hip.ptr(x), hip.ptr(ww), hip.ptr_c(bw), hip.ptr(z), dom, hip.stream()),
                      "sisr_nl_output_fwd")
            saved += [theta, phi, g, y, lse]
        ctx.save_for_backward(x, proj, wt, wp, wg, ww, *saved)
        ctx.cfg = (B, H, W, bool(quadrants))
        return z

    @staticmethod
    def backward(ctx, dz):
        B, H, W, quadrants = ctx.cfg
        x, proj, wt, wp, wg, ww, *saved = ctx.saved_tensors
        L, dev, npix = hip.lib(), x.device, B * H * W
        dz = ops._cl(dz)
        groups = _nl_domain_groups(B, H, W, quadrants)
        oparts = [L.sisr_nl_output_bwd_parts(dom) for dom, _, _, _ in groups]
        opart = torch.empty((sum(oparts), 64 * 8 + 64), device=dev)
        dproj = torch.empty((npix, 24), device=dev)
        row = 0
        for k, (dom, nd, hq, wq) in enumerate(groups):
            theta, phi, g, y, lse = saved[5 * k:5 * k + 5]
            nq, nk = hq * wq, (hq // 2) * (wq // 2)
            dy = torch.empty_like(y)
            hip.check(L.sisr_nl_output_bwd(hip.ptr(dz), hip.ptr(y), hip.ptr(ww), hip.ptr(dy), hip.ptr(opart[row:]), dom,
                                           hip.stream()), "sisr_nl_output_bwd")
            row += oparts[k]
            dtheta, dphi, dg = torch.empty_like(theta), torch.empty_like(phi), torch.empty_like(g)
            dsum = torch.empty_like(lse)
            hip.check(L.sisr_nl_attn_bwd(hip.ptr(theta), hip.ptr(phi), hip.ptr(g), hip.ptr(y), hip.ptr(lse), hip.ptr(dy),
                                         hip.ptr(dtheta), hip.ptr(dphi), hip.ptr(dg), hip.ptr(dsum), nd, nq, nk, 8,
                                         hip.stream()), "sisr_nl_attn_bwd")
            hip.check(L.sisr_nl_split_pool_bwd(hip.ptr(proj), hip.ptr(dtheta), hip.ptr(dphi), hip.ptr(dg), hip.ptr(dproj), dom,
                                               hip.stream()), "sisr_nl_split_pool_bwd")
        out_g = torch.empty(64 * 8 + 64, device=dev)
        hip.check(L.sisr_sum_partials(hip.ptr(opart), opart.shape[0], 1, 64 * 8 + 64, 1.0, hip.ptr(out_g), hip.stream()),
                  "sisr_sum_partials")
        pparts = L.sisr_nl_project_bwd_parts(npix)
        ppart = torch.empty((pparts, 33 * 64), device=dev)
        dx = ops._empty_cl(B, 64, H, W, dev)
        hip.check(L.sisr_nl_project_bwd(hip.ptr(x), hip.ptr(dproj), hip.ptr(dz), hip.ptr(wt), hip.ptr(wp), hip.ptr(wg),
                                        hip.ptr(dx), hip.ptr(ppart), npix, hip.stream()), "sisr_nl_project_bwd")
        pg = torch.empty(33 * 64, device=dev)
        hip.check(L.sisr_sum_partials(hip.ptr(ppart), pparts, 1, 33 * 64, 1.0, hip.ptr(pg), hip.stream()), "sisr_sum_partials")
        pg = pg.view(33, 64)
        dw = [pg[8 * i:8 * i + 8].reshape(8, 64, 1, 1) for i in range(3)]
        db = [pg[32, 8 * i:8 * i + 8] for i in range(3)]
        return (dx, None, dw[0], db[0], dw[1], db[1], dw[2], db[2], out_g[:512].view(64, 8, 1, 1), out_g[512:])


def nonlocal_block(x, block, quadrants):
    """block: san.NONLocalBlock2D (parameter holder)."""
    return _NonLocalBlock.apply(x, bool(quadrants), block.theta.weight, block.theta.bias, block.phi[0].weight,
                                block.phi[0].bias, block.g[0].weight, block.g[0].bias, block.W.weight, block.W.bias)


class _ScaleAdd(Function):
    """y = a + gamma * r with a learnable scalar gamma (SAN's share-source skip, ref: advanced/architectures.py:301-302)."""

    @staticmethod
    def forward(ctx, a, r, gamma):
        B, C, H, W = a.shape
        a, r = ops._cl(a), ops._cl(r)
        gv = gamma.reshape(1, 1).expand(B, C).contiguous()
        ctx.save_for_backward(r, gv)
        ctx.gshape = gamma.shape
        return ops._affine(r, gv, None, a, B, H, W, C)

    @staticmethod
    def backward(ctx, dy):
        r, gv = ctx.saved_tensors
        B, C, H, W = r.shape
        dy = ops._cl(dy)
        dr = ops._affine(dy, gv, None, None, B, H, W, C)
        if C != 64:
            raise NotImplementedError("scale_add backward is specialised for 64 channels")
        dgp, parts = ops._pixel_sums(dy, r, B, H, W)  # [B][parts][64] ordered partial sums of dy * r
        L = hip.lib()
        per = ops._vec(B, C, dy.device)
        hip.check(L.sisr_sum_partials(hip.ptr(dgp), parts, B, C, 1.0, hip.ptr(per), hip.stream()), "sisr_sum_partials")
        dgam = torch.empty(1, device=dy.device, dtype=torch.float32)
        hip.check(L.sisr_sum_partials(hip.ptr(per), B * C, 1, 1, 1.0, hip.ptr(dgam), hip.stream()), "sisr_sum_partials")
        return dy, dr, dgam.reshape(ctx.gshape)


def scale_add(a, r, gamma):
    return _ScaleAdd.apply(a, r, gamma)
