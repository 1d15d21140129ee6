"""The two epilogues of conv3x3_c64_w4_kernel against each other, bit for bit (pytest -m gpu).

A tile that lies inside the image takes the straight-line epilogue (select 12: Winograd forced); select 14 runs the
predicated epilogue on every tile.  Every form the kernel is instantiated for -- the eight 64 -> 64 forms and the chunked
plain one -- is launched under both, with the options the host accepts for it crossed (bias, ReLU, alpha = 0.5, out_scale,
partial sums on / off), and y, gate_out and the GAP / DOT partials must hold the same bit patterns (compared as int32: -0 is
not +0, a NaN equals itself).  Shapes:

  (3, 8, 64)      full tiles only, one tile per workgroup
  (3, 100, 250)   600 tiles, several per workgroup; full rows, ragged last column tile: both epilogues in one launch
  (2, 7, 45)      ragged both ways
  (1, 6, 64)      ragged rows only
  (2, 8, 20)      narrower than a tile

The maps are random with the cases an epilogue can get wrong planted in them: the first six pixel columns of x (and of the
gate's skip) are exact zeros of both signs, so that without a bias the conv's outputs there are zeros, the next six are
denormals (products and sums stay denormal: the kernels keep them), and the mask / residual / dot maps carry zeros of both
signs, denormals and negative values; about half of the outputs are cut by the ReLU and by the mask.
y and gate_out lie between guard bands of NaN canaries, which must stay untouched; a launch without partial sums must leave
a canary-filled partials buffer alone.  On dyadic data (tests/_exact.py) y, the partials and gate_out equal float64 at
(3, 100, 250) under both selects, which depends on neither epilogue agreeing with the other.
"""
import pytest
import torch

import sisr_amd
import test_exact_gpu as E
from test_winograd_chunks_gpu import packed_with_transform as packed_chunked

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
hip = sisr_amd.hip
DEV = "cuda:0"
FULL, PRED = ops.SELECT_WINOGRAD_FORCE, ops.SELECT_WINOGRAD_PREDICATED
GUARD = 4096  # floats of NaN before and after a guarded map (16-byte aligned)
NAN = float("nan")

SHAPES = [(3, 8, 64), (3, 100, 250), (2, 7, 45), (1, 6, 64), (2, 8, 20)]
# <AFFINE, MASK, RES, GATE, DOT> of the eight 64 -> 64 instantiations
FORMS = ["plain", "mask", "mask_affine", "res", "gate", "gate_res", "dot", "dot_res"]
CHAIN = {"gate", "gate_res", "dot", "dot_res"}  # the host refuses out_scale beside a gate or a dot


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def planted(shape, seed, zero_cols=True):
    """random normal map (B, C, H, W) on the CPU with zeros of both signs and denormals planted (module docstring)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=g)
    if zero_cols:  # whole pixel columns, all channels: the conv's outputs inherit them
        t[..., 0:3] = 0.0
        t[..., 3:6] = -0.0
        t[..., 6:12] *= 1e-41
    else:  # element-wise, for the epilogue's own operand maps
        u = torch.rand(*shape, generator=g)
        t[u < 0.10] = 0.0
        t[(u >= 0.10) & (u < 0.20)] = -0.0
        sel = (u >= 0.20) & (u < 0.30)
        t[sel] = t[sel] * 1e-41
    return t


class Maps:
    """the operands of one shape, shared by every form and option"""

    def __init__(self, B, H, W):
        s = (B, 64, H, W)
        seed = 1000 + 7 * B + 3 * H + W
        g = torch.Generator().manual_seed(seed)
        self.B, self.H, self.W = B, H, W
        self.x, self.skip = E.dev4(planted(s, seed + 1)), E.dev4(planted(s, seed + 2))
        self.res, self.mask, self.dot = (E.dev4(planted(s, seed + k, zero_cols=False)) for k in (3, 4, 5))
        self.w = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).to(DEV)
        self.bias = torch.randn(64, generator=g).to(DEV)
        self.sc, self.sh, self.os = (torch.randn(B, 64, generator=g).to(DEV) for _ in range(3))
        self.pf, self.pd = E.packed_with_transform(self.w)


_MAPS = {}


def maps(B, H, W):
    if (B, H, W) not in _MAPS:
        _MAPS.clear()  # one shape resident at a time
        _MAPS[(B, H, W)] = Maps(B, H, W)
    return _MAPS[(B, H, W)]


def guarded(B, C, H, W):
    """-> (flat buffer, its (B, C, H, W) channels-last window between two guard bands), all NaN"""
    n = B * C * H * W
    buf = torch.full((n + 2 * GUARD,), NAN, device=DEV)
    return buf, buf[GUARD:GUARD + n].view(B, H, W, C).permute(0, 3, 1, 2)


def guards_intact(buf):
    return bool(buf[:GUARD].isnan().all()) and bool(buf[-GUARD:].isnan().all())


def form_kwargs(form, M):
    kw = {}
    if form in ("mask", "mask_affine"):
        kw["mask"] = M.mask
    if form == "mask_affine":
        kw.update(in_scale=M.sc, in_shift=M.sh)
    if form in ("res", "gate_res", "dot_res"):
        kw["res"] = M.res
    if form in ("gate", "gate_res"):
        kw.update(in_scale=M.sc, gate_add=M.skip)
    if form in ("dot", "dot_res"):
        kw["dot"] = M.dot
    return kw


def options(form):
    """bias x ReLU x (neither | alpha | out_scale | alpha and out_scale) x partial sums, where the host accepts them"""
    out = []
    for bias in (False, True):
        for relu in (False, True):
            for scale in ("none", "alpha", "out_scale", "both"):
                if form in CHAIN and scale in ("out_scale", "both"):
                    continue
                for gap in (False, True):
                    if form in ("dot", "dot_res") and not gap:
                        continue  # a dot without partial sums is refused
                    out.append((bias, relu, scale, gap))
    return out


def launch(form, opt, M, select, canary=None):
    bias, relu, scale, gap = opt
    B, H, W = M.B, M.H, M.W
    kw = form_kwargs(form, M)
    if scale in ("alpha", "both"):
        kw["alpha"] = 0.5
    if scale in ("out_scale", "both"):
        kw["out_scale"] = M.os
    ybuf, y = guarded(B, 64, H, W)
    gbuf = gout = None
    if "gate_add" in kw:
        gbuf, gout = guarded(B, 64, H, W)
    parts = torch.full((B, ops.gap_parts(H, W), 64), NAN, device=DEV) if gap else None
    pk = M.pd if form in ("mask", "mask_affine") else M.pf
    v = hip.view_plain(H, W, 64)
    ops.conv_c64(M.x, v, pk, M.bias if bias else None, (1, 64), y, v, B, H, W, 64, 64, relu=relu, gap=parts, gate_out=gout,
                 select=select, **kw)
    assert guards_intact(ybuf), "y's guard bands were written"
    assert gbuf is None or guards_intact(gbuf), "gate_out's guard bands were written"
    if canary is not None:
        assert bool(canary.isnan().all()), "a launch without partial sums wrote the partials buffer"
    return y, gout, parts


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_full_tile_epilogue_equals_the_predicated_one(B, H, W, form):
    M = maps(B, H, W)
    canary = torch.full((B, ops.gap_parts(H, W), 64), NAN, device=DEV)
    seen_zero = seen_denormal = False
    for opt in options(form):
        got = launch(form, opt, M, FULL, canary=None if opt[3] else canary)
        want = launch(form, opt, M, PRED, canary=None if opt[3] else canary)
        for name, a, b in zip(("y", "gate_out", "partials"), got, want):
            assert (a is None) == (b is None)
            if a is None:
                continue
            assert not bool(a.isnan().any()), f"{form} {opt}: {name} has unwritten elements"
            assert same_bits(a, b), f"{form} {opt}: {name} differs between the two epilogues"
        y = got[0]
        seen_zero |= bool((y == 0).any())
        tiny = torch.finfo(torch.float32).tiny
        seen_denormal |= bool(((y != 0) & (y.abs() < tiny)).any())
    assert seen_zero, "no option produced an exact zero in y"
    if form in ("plain", "res", "dot", "dot_res"):  # x reaches the conv unscaled: the denormal columns give denormal outputs
        assert seen_denormal, "no option produced a denormal in y"


@pytest.mark.parametrize("dgrad", [False, True])
@pytest.mark.parametrize("B,H,W", [(2, 8, 32), (3, 100, 250), (2, 7, 45), (2, 8, 20)])
def test_chunked_form(B, H, W, dgrad):
    """64 -> 256 stored through the PixelShuffle(2) view and 256 -> 64 read through it: bias / ReLU / alpha crossed"""
    r = 2
    g = torch.Generator().manual_seed(50 + H + W)
    w = (torch.randn(256, 64, 3, 3, generator=g) * 0.05).to(DEV)
    bias = torch.randn(64 if dgrad else 256, generator=g).to(DEV)
    pf, pd = packed_chunked(w, r)
    x = E.dev4(planted((B, 64, r * H, r * W) if dgrad else (B, 64, H, W), 60 + H + W))
    vp, vs = hip.view_plain(H, W, 64), hip.view_shuffle(H, W, r)
    for use_bias in (False, True):
        for relu in (False, True):
            for alpha in (1.0, 0.5):
                ys = []
                for sel in (FULL, PRED):
                    ybuf, y = guarded(B, 64, H, W) if dgrad else guarded(B, 64, r * H, r * W)
                    if dgrad:
                        ops.conv_c64(x, vs, pd, bias if use_bias else None, (1, 64), y, vp, B, H, W, 256, 64, alpha=alpha,
                                     relu=relu, select=sel)
                    else:
                        ops.conv_c64(x, vp, pf, bias if use_bias else None, (r * r, 1), y, vs, B, H, W, 64, 256, alpha=alpha,
                                     relu=relu, select=sel)
                    assert guards_intact(ybuf), "y's guard bands were written"
                    assert not bool(y.isnan().any())
                    ys.append(y)
                assert same_bits(*ys), (use_bias, relu, alpha)


_EXACT = {}


@pytest.mark.parametrize("select", [FULL, PRED])
@pytest.mark.parametrize("form", ["bias_relu_gap", "mask_affine", "gate_relu", "dot_res"])
def test_exact_against_float64(form, select):
    """plain, mask + affine, GATE and DOT + residual on dyadic data at (3, 100, 250): y, partials and gate_out equal float64"""
    B, H, W = 3, 100, 250
    if not _EXACT:
        D = E.ConvData(B, H, W, seed=1100)
        _EXACT["d"] = (D, E.packed_with_transform(D.dev["w"]))
    D, packs = _EXACT["d"]
    fail = E.check_conv_case(form, D, packs, select, winograd=True)
    assert fail is None, fail


def test_the_predicated_select_is_the_forced_winograd_form():
    """select 14 picks the same kernel as 12 below the size threshold too, and a packing without the transform is refused
    neither more nor less than under 12 (other channel counts: an argument error)"""
    M = maps(2, 8, 20)
    y12, _, _ = launch("plain", (True, True, "none", False), M, FULL)
    y14, _, _ = launch("plain", (True, True, "none", False), M, PRED)
    y7, _, _ = launch("plain", (True, True, "none", False), M, 7)
    assert same_bits(y12, y14) and not same_bits(y14, y7)
    x = E.dev4(torch.zeros(1, 128, 8, 32))
    y = E.nan4(1, 128, 8, 32)
    pk = torch.zeros(128 * 128 * 9 + 4 * ops.WINOGRAD_FLOATS, device=DEV)
    with pytest.raises(RuntimeError):
        ops.conv_c64(x, hip.view_plain(8, 32, 128), pk, None, (1, 64), y, hip.view_plain(8, 32, 128), 1, 8, 32, 128, 128, select=PRED)
    torch.cuda.synchronize()
