"""Residual Dense Blocks on the dense-block kernels (csrc/dense.hip): ops.dense_conv, ops.dense_block, ops.dense_skip.
Reaches the core as ops.NAME at call time (the access rule at the top of ops.py); ops re-exports the operators.

A block works on ONE channels-last stack S (B, 192, H, W): channels 0..63 the block input x, slot j = channels
64 + 32 (j - 1) .. 64 + 32 j - 1 the output x_j of growth layer j.  Layer j reads channels [0, 64 + 32 (j - 1)) and writes its
slot of the same buffer; conv5 (192 -> 64) runs on conv_c64 with the stack as its input view and channels 0..63 as `res`, and
writes x5 * alpha + x into channels 0..63 of a NEW stack, which it returns as a (B, 64, H, W) view of pitch 192.  The next
dense_block (or dense_skip's successor) recognises such a view and fills the rest of that stack: torch.cat never runs, and the
stack is the one activation a block keeps for its backward pass.
"""
import functools
import math
import weakref

import torch
from torch.autograd import Function

from . import hip, ops

STACK = 192   # channels of a block's stack
GROW = 32     # output channels of a growth conv
LAYERS = 4    # growth convs per block
CINS = tuple(64 + GROW * j for j in range(LAYERS))  # (64, 96, 128, 160)

# Stacks whose channels 64.. nobody has written yet: address of the storage -> (weak reference to the storage object, address
# of channel 0).  A block CLAIMS the stack behind its input (one claim per stack: a map fed to two blocks is copied for the
# second), so an entry lives from the launch that wrote the stack's first 64 channels to the first block that reads them -- or,
# for a stack nobody claims (the trunk's last dense_skip), to the death of its storage: the weak reference's callback removes
# it then, so an entry never outlives the storage it names.  torch keeps ONE Python object per live storage, so a claim also
# checks that the view's storage IS the recorded object: an unrelated tensor that the allocator gives the same addresses
# afterwards can never pass for an open stack.
_OPEN_STACKS = {}


def _forget_stack(key, ref):
    """callback of an entry's weak reference: the storage is gone, and so is the entry (unless the key is another stack's by now)"""
    entry = _OPEN_STACKS.get(key)
    if entry is not None and entry[0] is ref:
        del _OPEN_STACKS[key]


def _stack_strides(t, H, W):
    """is t (B, C, H, W) laid out as channels of pitch-192 pixel records (strides of size-1 dimensions do not matter)?"""
    want = (H * W * STACK, 1, W * STACK, STACK)
    return all(n == 1 or s == w for n, s, w in zip(t.shape, t.stride(), want))


def _new_stack(B, H, W, device, open_=True):
    S = ops._empty_cl(B, STACK, H, W, device)
    if open_:
        st = S.untyped_storage()
        key = st._cdata
        _OPEN_STACKS[key] = (weakref.ref(st, functools.partial(_forget_stack, key)), S.data_ptr())
    return S


def _claim_stack(x):
    """the (B, 192, H, W) stack x is the first 64 channels of, if x is an unclaimed output of dense_block / dense_skip"""
    B, _, H, W = x.shape
    st = x.untyped_storage()
    entry = _OPEN_STACKS.get(st._cdata)
    if entry is None or entry[0]() is not st or entry[1] != x.data_ptr() or not _stack_strides(x, H, W) or x.storage_offset() != 0:
        return None
    if st.nbytes() < B * H * W * STACK * 4:
        return None
    del _OPEN_STACKS[st._cdata]
    return torch.as_strided(x, (B, STACK, H, W), (H * W * STACK, 1, W * STACK, STACK))


def _pitched(t):
    """(map, pitch) of a 64-channel map the kernels can read in place: contiguous channels-last, or a view into a stack"""
    B, C, H, W = t.shape
    if C == 64 and _stack_strides(t, H, W) and t.data_ptr() % 16 == 0:
        return t, STACK
    t = ops._cl(t)
    return t, C


def _check_slope(slope, what):
    slope = float(slope)
    if not (math.isfinite(slope) and slope >= 0):  # (the backward reads the sign of the pre-activation off the saved output)
        raise ValueError(f"{what}: the LeakyReLU slope must be finite and >= 0, got {slope}")
    return slope


def dense_pack(weight, need_dgrad=True):
    """OIHW (32, cin, 3, 3) -> (forward packing, input-gradient packing | None) of the dense-block kernels, one launch"""
    co, ci = weight.shape[0], weight.shape[1]
    if co != GROW or ci not in CINS or tuple(weight.shape[2:]) != (3, 3):
        raise NotImplementedError(f"the dense-block kernels take (32, cin, 3, 3) weights with cin in {CINS}, "
                                  f"got {tuple(weight.shape)}")
    buf = torch.empty((2 if need_dgrad else 1, weight.numel()), device=weight.device, dtype=torch.float32)
    hip.check(hip.lib().sisr_pack_dense3x3(hip.ptr(weight.contiguous()), hip.ptr(buf[0]), hip.ptr(buf[1]) if need_dgrad else None,
                                           ci, hip.stream()), "sisr_pack_dense3x3")
    return buf[0], (buf[1] if need_dgrad else None)


def dense_conv(stack, cin, weight, bias, slope=0.2, act=True):
    """One growth layer, in place and without autograd: channels [cin, cin + 32) of the channels-last `stack` become
    act ? lrelu_slope(conv(stack[:, :cin]) + bias) : conv + bias; every other channel stays as it is.  Returns that slot (a view)."""
    ops._fp32_only("dense_conv")
    B, C, H, W = stack.shape
    if C % 32 or C < cin + GROW or not stack.is_contiguous(memory_format=ops.CL):
        raise RuntimeError(f"dense_conv: the stack must be channels-last with a multiple of 32 channels and room for the slot "
                           f"[{cin}, {cin + GROW}); got {tuple(stack.shape)}")
    if weight.shape[1] != cin:
        raise RuntimeError(f"dense_conv: the weight takes {weight.shape[1]} channels, cin is {cin}")
    slope = _check_slope(slope, "dense_conv")
    with torch.no_grad():
        pf, _ = dense_pack(weight, need_dgrad=False)
        hip.check(hip.lib().sisr_dense3x3_fwd(hip.ptr(stack), C, cin, hip.ptr(pf), hip.ptr_c(bias), int(bool(act)), slope,
                                              hip.ptr(stack) + 4 * cin, C, B, H, W, hip.stream()), "sisr_dense3x3_fwd")
    return stack[:, cin:cin + GROW]


class _DenseBlock(Function):
    """RDB(x) = conv5(cat(x, x_1 .. x_4)) * alpha + x with x_j = lrelu(conv_j(cat(x, x_1 .. x_{j-1}))) as ONE node.
    Forward: four sisr_dense3x3_fwd launches into the stack, conv5 on conv_c64.  Keeps the stack and nothing else pixel-sized.
    Backward, over a gradient stack dS: conv5's input gradient fills dS (+ dOut on channels 0..63); for j = 4 .. 1 slot j of dS,
    read through the LeakyReLU mask of slot j of S, goes through sisr_dense3x3_wgrad and sisr_dense3x3_dgrad(accumulate) into
    dS[:, :cin_j]; dx is channels 0..63 of dS."""

    @staticmethod
    def forward(ctx, x, slope, alpha, *params):
        ops._fp32_only("dense_block")
        B, C, H, W = x.shape
        ws, bs = params[0::2], params[1::2]
        dev, L = x.device, hip.lib()
        any_grad = any(ctx.needs_input_grad)
        S = _claim_stack(x)
        if S is None:
            xc = ops._cl(x)
            S = _new_stack(B, H, W, dev, open_=False)
            ops._map64(xc, 64, None, 0, S, STACK, B * H * W, 0)
        n = [w.numel() for w in ws[:LAYERS]]
        packs = torch.empty((2 if any_grad else 1, sum(n)), device=dev, dtype=torch.float32)
        off, pd = 0, []
        for j in range(LAYERS):
            cin, w = CINS[j], ws[j].contiguous()
            pf = packs[0, off:off + n[j]]
            pd.append(packs[1, off:off + n[j]] if any_grad else None)
            off += n[j]
            hip.check(L.sisr_pack_dense3x3(hip.ptr(w), hip.ptr(pf), hip.ptr(pd[j]), cin, hip.stream()), "sisr_pack_dense3x3")
            hip.check(L.sisr_dense3x3_fwd(hip.ptr(S), STACK, cin, hip.ptr(pf), hip.ptr_c(bs[j]), 1, slope,
                                          hip.ptr(S) + 4 * cin, STACK, B, H, W, hip.stream()), "sisr_dense3x3_fwd")
        w5 = ws[LAYERS].contiguous()
        if any_grad:
            pf5, pd5 = ops.pack_pair(w5)
        else:
            pf5, pd5 = ops.pack_weight(w5, "fwd"), None
        out = _new_stack(B, H, W, dev)
        v = hip.view_plain(H, W, STACK)
        ops.conv_c64(S, v, pf5, bs[LAYERS], (1, 64), out, v, B, H, W, STACK, 64, res=S, alpha=alpha)
        ctx.save_for_backward(S, packs[1] if any_grad else None, pd5, *ws)
        ctx.biases, ctx.cfg = bs, (B, H, W, slope, alpha, n)
        return out[:, :64]

    @staticmethod
    @ops._in_backward
    def backward(ctx, dout):
        S, pdall, pd5, *ws = ctx.saved_tensors
        bs = ctx.biases
        B, H, W, slope, alpha, n = ctx.cfg
        dev, L = S.device, hip.lib()
        need = ctx.needs_input_grad
        need_w = [need[3 + 2 * j] for j in range(LAYERS + 1)]
        need_b = [bs[j] is not None and need[4 + 2 * j] for j in range(LAYERS + 1)]
        dout, p = _pitched(dout)
        v, vo = hip.view_plain(H, W, STACK), hip.view_plain(H, W, p)
        grads = [None] * (2 * (LAYERS + 1))
        if need_w[LAYERS] or need_b[LAYERS]:
            w5 = ws[LAYERS]
            dwb, db, dw = ops._wb_grad_bufs(w5, bs[LAYERS], need_w[LAYERS], need_b[LAYERS])
            ops.wgrad_c64(S, v, dout, vo, dwb, db, B, H, W, STACK, 64, alpha=alpha, owner=w5 if need_w[LAYERS] else None)
            grads[2 * LAYERS], grads[2 * LAYERS + 1] = dw, db
        inner = [need[0] or any(need_w[:j]) or any(need_b[:j]) for j in range(LAYERS + 1)]  # is dS[:, :cin_j] wanted at all?
        dx = None
        if inner[LAYERS]:
            dS = ops._empty_cl(B, STACK, H, W, dev)
            ops.conv_c64(dout, vo, pd5, None, (1, 64), dS, v, B, H, W, 64, STACK, alpha=alpha)
            ops._map64(dS, STACK, dout, p, dS, STACK, B * H * W, 1)
            off = sum(n)
            for j in reversed(range(LAYERS)):
                cin = CINS[j]
                off -= n[j]
                dy, mask = hip.ptr(dS) + 4 * cin, hip.ptr(S) + 4 * cin
                if need_w[j] or need_b[j]:
                    dwb, db, dw = ops._wb_grad_bufs(ws[j], bs[j], need_w[j], need_b[j])
                    nb = L.sisr_dense3x3_wgrad_workspace_bytes(B, H, W, cin)
                    wsp = hip.workspace(dev, nb)
                    hip.check(L.sisr_dense3x3_wgrad(hip.ptr(S), STACK, cin, dy, STACK, mask, STACK, slope, hip.ptr(dwb),
                                                    hip.ptr(db), hip.ptr(wsp), nb, B, H, W, hip.stream()), "sisr_dense3x3_wgrad")
                    grads[2 * j], grads[2 * j + 1] = dw, db
                if inner[j]:
                    hip.check(L.sisr_dense3x3_dgrad(dy, STACK, mask, STACK, slope, hip.ptr(pdall[off:off + n[j]]), hip.ptr(dS),
                                                    STACK, cin, 1, B, H, W, hip.stream()), "sisr_dense3x3_dgrad")
            if need[0]:
                dx = dS[:, :64]
        return (dx, None, None, *grads)


def dense_block(x, convs, slope=0.2, alpha=0.2, out=None):
    """One Residual Dense Block.  convs: five (weight, bias) pairs, (32, 64 + 32 (j - 1), 3, 3) for j = 1 .. 4 and (64, 192, 3, 3).
    Returns conv5(...) * alpha + x as a (B, 64, H, W) view (pitch 192) of a fresh stack that the next block fills in place.
    out: not taken -- the block always allocates the stack its result opens."""
    if out is not None:
        raise NotImplementedError("dense_block allocates the stack that its result opens; `out` is not taken")
    if x.dim() != 4 or x.shape[1] != 64:
        raise NotImplementedError(f"dense_block takes a 64-channel map, got {tuple(x.shape)}")
    convs = list(convs)
    shapes = [(GROW, c, 3, 3) for c in CINS] + [(64, STACK, 3, 3)]
    if len(convs) != LAYERS + 1 or any(tuple(w.shape) != s for (w, _), s in zip(convs, shapes)):
        raise NotImplementedError(f"dense_block takes five convs of shapes {shapes} (num_features 64, num_grow_ch 32), got "
                                  f"{[tuple(w.shape) for w, _ in convs]}")
    slope = _check_slope(slope, "dense_block")
    flat = [t for wb in convs for t in wb]
    return _DenseBlock.apply(x, slope, float(alpha), *flat)


class _DenseSkip(Function):
    """y = t * g[b, c] + x between stacks: t and x are read at their own pitch, y opens a new stack."""

    @staticmethod
    def forward(ctx, t, g, x):
        ops._fp32_only("dense_skip")
        B, C, H, W = t.shape
        t, tp = _pitched(t)
        x, xp = _pitched(x)
        g2 = g.reshape(B, 64).contiguous()
        out = _new_stack(B, H, W, t.device)
        hip.check(hip.lib().sisr_dense_skip(hip.ptr(t), tp, hip.ptr(g2), hip.ptr(x), xp, hip.ptr(out), STACK, B, H * W,
                                            hip.stream()), "sisr_dense_skip")
        tc = None
        if ctx.needs_input_grad[1]:  # the gate's gradient sums dy * t: keep t alone, not the stack it closes
            tc = ops._empty_cl(B, 64, H, W, t.device)
            ops._map64(t, tp, None, 0, tc, 64, B * H * W, 0)
        ctx.save_for_backward(g2, tc)
        ctx.gshape = g.shape
        return out[:, :64]

    @staticmethod
    def backward(ctx, dy):
        g2, tc = ctx.saved_tensors
        B, C, H, W = dy.shape
        dt = dg = None
        if ctx.needs_input_grad[0]:
            dyp, p = _pitched(dy)
            dt = ops._empty_cl(B, 64, H, W, dy.device)
            hip.check(hip.lib().sisr_dense_skip(hip.ptr(dyp), p, hip.ptr(g2), None, 0, hip.ptr(dt), 64, B, H * W, hip.stream()),
                      "sisr_dense_skip(backward)")
        if ctx.needs_input_grad[1]:
            part, parts = ops._pixel_sums(ops._cl(dy), tc, B, H, W, 64)
            dg = ops._vec(B, 64, dy.device)
            hip.check(hip.lib().sisr_sum_partials(hip.ptr(part), parts, B, 64, 1.0, hip.ptr(dg), hip.stream()),
                      "sisr_sum_partials")
            dg = dg.reshape(ctx.gshape)
        return dt, dg, (dy if ctx.needs_input_grad[2] else None)


def dense_skip(t, g, x):
    """t * g + x on 64-channel maps, g (B, 64): an RRDB's skip.  Reads outputs of dense_block in place and returns a view
    that the next dense_block fills in place."""
    if t.dim() != 4 or t.shape[1] != 64 or x.shape != t.shape:
        raise NotImplementedError(f"dense_skip takes two 64-channel maps of one shape, got {tuple(t.shape)} and {tuple(x.shape)}")
    return _DenseSkip.apply(t, g, x)
