"""Dense-block entry points, host side (no GPU): every bad argument is refused with an error code before any device call, the
workspace query answers on the host, and the operators exist where callers look for them."""
import ctypes as C

import pytest

import sisr_amd

hip, ops = sisr_amd.hip, sisr_amd.ops
ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -4


def _standins():
    buf = (C.c_float * 4096)()
    a = (C.addressof(buf) + 15) & ~15  # non-null, 16-byte aligned: every call below must fail before it is dereferenced
    return buf, a


def test_dense_workspace_query_counts_slices_of_tiles():
    """one slice per 8 x 32 pixel tile until cin / 32 chunks of them fill 768 workgroups; each holds (32, cin, 3, 3) + 32 floats"""
    q = hip.lib().sisr_dense3x3_wgrad_workspace_bytes
    assert q(1, 8, 32, 64) == 1 * (32 * 64 * 9 + 32) * 4
    assert q(2, 9, 33, 96) == 2 * 2 * 2 * (32 * 96 * 9 + 32) * 4
    assert q(8, 128, 128, 64) == (768 // 2) * (32 * 64 * 9 + 32) * 4
    assert q(8, 128, 128, 160) == (768 // 5) * (32 * 160 * 9 + 32) * 4
    for bad in ((0, 8, 8, 64), (1, 0, 8, 64), (1, 8, 8, 48), (1, 8, 8, 0), (1, 8, 8, 224), (1, 8, 8, 192), (1, 8, 8, 32)):
        assert q(*bad) == 0, bad


def test_dense_entry_points_refuse_bad_arguments_before_any_device_call():
    L = hip.lib()
    buf, a = _standins()
    y = a + 4 * 64  # the slot behind 64 input channels
    ws = L.sisr_dense3x3_wgrad_workspace_bytes(1, 8, 8, 64)
    fwd = lambda **k: L.sisr_dense3x3_fwd(*[k.get(n, d) for n, d in (  # noqa: E731
        ("x", a), ("xp", 192), ("cin", 64), ("packed", a), ("bias", None), ("act", 1), ("slope", 0.2), ("y", y), ("yp", 192),
        ("B", 1), ("H", 8), ("W", 8), ("stream", None))])
    dgrad = lambda **k: L.sisr_dense3x3_dgrad(*[k.get(n, d) for n, d in (  # noqa: E731
        ("dy", y), ("dyp", 192), ("mask", None), ("mp", 192), ("slope", 0.2), ("packed", a), ("dx", a), ("dxp", 192), ("cin", 64),
        ("accumulate", 1), ("B", 1), ("H", 8), ("W", 8), ("stream", None))])
    wgrad = lambda **k: L.sisr_dense3x3_wgrad(*[k.get(n, d) for n, d in (  # noqa: E731
        ("x", a), ("xp", 192), ("cin", 64), ("dy", y), ("dyp", 192), ("mask", None), ("mp", 192), ("slope", 0.2), ("dw", a),
        ("db", None), ("ws", a), ("bytes", ws), ("B", 1), ("H", 8), ("W", 8), ("stream", None))])
    # null pointers
    for name in ("x", "packed", "y"):
        assert fwd(**{name: None}) == ERR_ARG, name
    for name in ("dy", "packed", "dx"):
        assert dgrad(**{name: None}) == ERR_ARG, name
    for name in ("x", "dy", "dw", "ws"):
        assert wgrad(**{name: None}) == ERR_ARG, name
    assert L.sisr_pack_dense3x3(None, a, a, 64, None) == ERR_ARG and L.sisr_pack_dense3x3(a, None, None, 64, None) == ERR_ARG
    # channel counts: no multiple of 32, zero, beyond the stack; multiples of 32 that are not built
    for call in (fwd, dgrad, wgrad):
        for cin in (48, 0, 224, -64):
            assert call(cin=cin) != 0, cin
        assert call(cin=48) == ERR_ARG and call(cin=0) == ERR_ARG
        assert call(cin=224) == ERR_UNSUPPORTED and call(cin=32) == ERR_UNSUPPORTED and call(cin=192) == ERR_UNSUPPORTED
    assert L.sisr_pack_dense3x3(a, a, a, 48, None) == ERR_ARG and L.sisr_pack_dense3x3(a, a, a, 224, None) == ERR_UNSUPPORTED
    # pitches: no multiple of 32, too small for the range
    assert fwd(xp=100) == ERR_ARG and fwd(yp=100) == ERR_ARG and fwd(xp=32) == ERR_ARG and fwd(yp=0) == ERR_ARG
    assert dgrad(dyp=100) == ERR_ARG and dgrad(dxp=100) == ERR_ARG and dgrad(dxp=32) == ERR_ARG and dgrad(mask=y, mp=100) == ERR_ARG
    assert wgrad(xp=100) == ERR_ARG and wgrad(dyp=100) == ERR_ARG and wgrad(mask=y, mp=16) == ERR_ARG
    # overlapping in-place ranges: the slot inside the channels read / the gradient written, or wrapping into the next pixel
    assert fwd(y=a + 4 * 32) == ERR_ARG and fwd(y=a) == ERR_ARG and fwd(y=a + 4 * 176) == ERR_ARG
    assert fwd(y=a + 4 * 64, yp=96) == ERR_ARG  # one allocation, two pitches
    assert dgrad(dy=a + 4 * 32) == ERR_ARG and dgrad(dy=a + 4 * 176) == ERR_ARG and dgrad(mask=a + 4 * 32) == ERR_ARG
    # misaligned pointers
    assert fwd(x=a + 4) == ERR_ALIGN and fwd(y=y + 8) == ERR_ALIGN and dgrad(dx=a + 4) == ERR_ALIGN and wgrad(dy=y + 4) == ERR_ALIGN
    # a workspace one byte short, an empty batch, an empty image, a slope that is no number
    assert wgrad(bytes=ws - 1) == ERR_ARG
    for call in (fwd, dgrad, wgrad):
        assert call(B=0) == ERR_ARG and call(H=0) == ERR_ARG and call(W=-1) == ERR_ARG and call(B=65536) == ERR_ARG
        assert call(slope=float("nan")) == ERR_ARG and call(slope=float("inf")) == ERR_ARG
    # the skip between stacks
    skip = lambda **k: L.sisr_dense_skip(*[k.get(n, d) for n, d in (  # noqa: E731
        ("t", a), ("tp", 192), ("g", a), ("x", None), ("xp", 0), ("y", a + 4 * 64), ("yp", 192), ("B", 1), ("hw", 4),
        ("stream", None))])
    assert skip(t=None) == ERR_ARG and skip(g=None) == ERR_ARG and skip(y=None) == ERR_ARG and skip(B=0) == ERR_ARG
    assert skip(tp=100) == ERR_ARG and skip(yp=32) == ERR_ARG and skip(y=a + 4 * 32) == ERR_ARG and skip(x=a, xp=48) == ERR_ARG
    assert skip(y=a + 4) == ERR_ALIGN
    del buf


def test_ops_offers_the_dense_operators_and_they_are_fp32_only():
    import torch
    for name in ("dense_conv", "dense_block", "dense_skip", "dense_pack"):
        assert callable(getattr(ops, name)), name
    x = torch.zeros(1, 64, 4, 4)
    convs = [(torch.zeros(32, 64 + 32 * j, 3, 3), torch.zeros(32)) for j in range(4)] + [(torch.zeros(64, 192, 3, 3), torch.zeros(64))]
    ops.set_precision("bf16")
    try:
        with pytest.raises(NotImplementedError, match="fp32"):
            ops.dense_block(x, convs)
        with pytest.raises(NotImplementedError, match="fp32"):
            ops.dense_conv(torch.zeros(1, 192, 4, 4).contiguous(memory_format=torch.channels_last), 64, convs[0][0], None)
        with pytest.raises(NotImplementedError, match="fp32"):
            ops.dense_skip(x, torch.zeros(1, 64), x)
    finally:
        ops.set_precision("fp32")
    with pytest.raises(NotImplementedError, match="five convs"):
        ops.dense_block(x, convs[:4])
    with pytest.raises(NotImplementedError, match="64-channel"):
        ops.dense_block(torch.zeros(1, 32, 4, 4), convs)
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP device"):
        ops.dense_block(x, convs)


# ----------------------------------------------------------------------------- the registry of open stacks (plain host logic)
# ops_dense._new_stack / _claim_stack only allocate and compare: host tensors take the same path as device ones.
OD = sisr_amd.ops_dense
SHAPE = (2, 9, 21)  # (B, H, W)


def _open(shape=SHAPE):
    B, H, W = shape
    return OD._new_stack(B, H, W, "cpu")


def test_an_unclaimed_stack_leaves_the_registry_with_its_storage():
    """an entry never outlives the storage it names: dropped unclaimed, a stack takes its entry with it -- once, and ten
    thousand times over without the registry growing or a live open stack losing its claim to the pile of dead ones"""
    import gc
    gc.collect()
    start = len(OD._OPEN_STACKS)
    S = _open()
    y = S[:, :64]
    assert len(OD._OPEN_STACKS) == start + 1
    del S
    assert len(OD._OPEN_STACKS) == start + 1, "the 64-channel view keeps the storage, and with it the entry, alive"
    del y
    gc.collect()
    assert len(OD._OPEN_STACKS) == start
    live = _open()
    keep = live[:, :64]
    del live
    start = len(OD._OPEN_STACKS)
    worst = start
    for _ in range(10000):
        S = _open()
        y = S[:, :64]
        worst = max(worst, len(OD._OPEN_STACKS))
        del S, y
        worst = max(worst, len(OD._OPEN_STACKS))
    assert worst <= start + 1, (start, worst)
    gc.collect()
    assert len(OD._OPEN_STACKS) == start
    full = OD._claim_stack(keep)
    assert full is not None and tuple(full.shape) == (2, 192, 9, 21) and full.data_ptr() == keep.data_ptr()
    assert len(OD._OPEN_STACKS) == start - 1


def test_a_foreign_tensor_at_a_dead_stacks_address_is_not_claimed():
    """the allocator may hand an unrelated (B, 192, H, W) tensor the storage-object address AND the block of a stack that died
    unclaimed; its first 64 channels must not pass for an open stack, or dense_block would fill the caller's channels 64.."""
    B, H, W = SHAPE
    reused = []
    for _ in range(8):
        S = _open()
        y = S[:, :64]
        was = (S.untyped_storage()._cdata, S.data_ptr())
        del S, y
        Z = ops._empty_cl(B, 192, H, W, "cpu")
        reused.append((Z.untyped_storage()._cdata, Z.data_ptr()) == was)
        assert OD._claim_stack(Z[:, :64]) is None, "claimed a tensor that _new_stack never made (addresses reused: %s)" % reused[-1]
    print("storage address and block reused in %d of 8 rounds" % sum(reused))


def test_claims_are_single_and_only_for_the_view_new_stack_made(monkeypatch):
    import torch
    B, H, W = SHAPE
    S = _open()
    y = S[:, :64]
    full = OD._claim_stack(y)
    assert full is not None and full.data_ptr() == S.data_ptr() and full.stride() == S.stride() and full.shape == S.shape
    assert OD._claim_stack(y) is None, "a stack is claimed once"
    # a nonzero storage offset: channels 32..95 of an open stack, and the second image of one
    S = _open()
    assert OD._claim_stack(S[:, 32:96]) is None
    assert OD._claim_stack(S[1:, :64]) is None
    assert OD._claim_stack(S[:, :64]) is not None, "the refusals above must not have consumed the entry"
    # a storage too small for the stack: a registered 64-channel map of pitch 192 whose storage ends with its own last pixel,
    # 128 floats short of the stack (everything else about it matches: the size check alone refuses it)
    strides = (H * W * 192, 1, W * 192, 192)
    short = torch.as_strided(torch.empty(B * H * W * 192 - 128), (B, 64, H, W), strides)
    monkeypatch.setattr(ops, "_empty_cl", lambda *a: short)
    y = _open()
    monkeypatch.undo()
    assert y is short and y.untyped_storage()._cdata in OD._OPEN_STACKS and y.storage_offset() == 0
    assert OD._claim_stack(y) is None
    # pitch 192, offset 0, room enough -- but not from _new_stack
    Z = ops._empty_cl(B, 192, H, W, "cpu")
    assert OD._claim_stack(Z[:, :64]) is None
    closed = OD._new_stack(B, H, W, "cpu", open_=False)
    assert OD._claim_stack(closed[:, :64]) is None
    # ... nor a contiguous 64-channel map
    assert OD._claim_stack(ops._empty_cl(B, 64, H, W, "cpu")) is None
