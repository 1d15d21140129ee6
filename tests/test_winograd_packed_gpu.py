"""The Winograd kernels with their transforms on packed adds (v_pk_add_f32 on register pairs: conv3x3_c64_w4_kernel pairs
the four ci of a register quad, wgrad3x3_c64_w4_kernel the columns (j, j + 1) of a patch row).  One-hot detectors on dyadic
data, exact against float64: a swapped half or a lost negation of a packed add changes an integer of the output, and the
failure names the form, the element and the patch position that feed it."""
import itertools

import pytest
import torch

import _exact as X
import sisr_amd
import test_exact_gpu as E
import test_winograd_wgrad_gpu as T

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
hip = sisr_amd.hip
DEV = "cuda:0"
WINO = ops.SELECT_WINOGRAD_FORCE

# ---------------------------------------------------------------------------------------------------------------- conv
CONV_SHAPES = [(1, 4, 32), (1, 6, 70), (2, 9, 33), (3, 20, 64)]
CIS = [0, 1, 2, 3, 21, 42, 63]  # ci = 16 G + 4 q + e: every e at (G, q) = (0, 0), then (1, 1, e 1), (2, 2, e 2), (3, 3, e 3)
FORMS = ["plain", "mask_affine", "gate", "dot_res"]
# the plain tap-and-sign weights, and the same with the factor 1 + e: a value that lands on another element of its register quad
# (a swapped pair) then meets another weight
WEIGHTS = ["tap_sign", "tap_sign_e"]


def detector_weight(kind):
    ky, kx = torch.meshgrid(torch.arange(3), torch.arange(3), indexing="ij")
    w = (2.0 ** (3 * ky + kx)).view(1, 1, 3, 3) * ((-1.0) ** torch.arange(64)).view(64, 1, 1, 1) * torch.ones(1, 64, 1, 1)
    if kind == "tap_sign_e":
        w = w * (1 + torch.arange(64) % 4).view(1, 64, 1, 1)
    return w.contiguous()


def conv_places(B, H, W):
    """(b, h, w, what): a 4 x 4 window of pixels that is the patch of one Winograd tile (rows 2 tr - 1 .. 2 tr + 2, columns
    2 tc - 1 .. 2 tc + 2; at H = 4 no patch lies inside the image: rows 0 .. 3 are positions 1 .. 3 of tile row 0 and 0 .. 2
    of tile row 1), then both sides of the 32-column and 4-row tile boundaries and the last pixel"""
    h0, w0 = (1 if H >= 5 else 0), 7
    tr, tc = (h0 + 1) // 2, (w0 + 1) // 2
    places = []
    for h, w in itertools.product(range(h0, h0 + 4), range(w0, w0 + 4)):
        assert 0 <= h < H and 0 <= w < W, "TEST BUG: the window leaves the image"
        places.append((B - 1, h, w, f"patch position ({h - (2 * tr - 1)}, {w - (2 * tc - 1)}) of Winograd tile ({tr}, {tc})"))
    for w in (31, 32):
        if w < W:
            places.append((0, min(2, H - 1), w, f"column {w} at the 32-column tile boundary"))
    for h in (3, 4):
        if h < H:
            places.append((0, h, min(5, W - 1), f"row {h} at the 4-row tile boundary"))
    places.append((0, H - 1, W - 1, "last pixel of the image"))
    return places


_PACKS = {}


def packs(kind):
    if kind not in _PACKS:
        w = detector_weight(kind)
        _PACKS[kind] = (w, E.packed_with_transform(w.to(DEV))[0])
    return _PACKS[kind]


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,H,W", CONV_SHAPES)
def test_conv_one_hot_detector(B, H, W, form, weights):
    """x zero but for one pixel (value 1) of one input channel; weights 2^(3 ky + kx) (-1)^co [(1 + e)]: every output is a
    signed power of two (times 1 + e) that names the tap.  Forms: plain (bias, ReLU, pooled sums); mask + affine (in_scale a
    power of two per channel, in_shift zero so that the map stays one-hot, mask with zeros); GATE (the gated map x * g + 0,
    also checked as gate_out); DOT + residual (integer residual and dot maps, the partial sums compared as their sum)."""
    w, pf = packs(weights)
    w64 = E.dd(w)
    s = (B, 64, H, W)
    sc = 2.0 ** X.ints((B, 64), 31, -1, 1)
    res, dot, m = X.ints(s, 32), X.ints(s, 33), X.ints(s, 34, zeros=0.3)
    bias = X.ints((64,), 35, -4, 4)
    dev = dict(sc=sc.to(DEV), sh=torch.zeros(B, 64, device=DEV), res=E.dev4(res), dot=E.dev4(dot), m=E.dev4(m), b=bias.to(DEV),
               skip=E.dev4(torch.zeros(s)))
    res64, dot64, mask64 = E.dd(res), E.dd(dot), X.relu_mask(E.dd(m))
    bad = []
    cases = [(ci, p) for ci in CIS for p in conv_places(B, H, W)]
    for ci, (b, h, wc, what) in cases:
        x = torch.zeros(s)
        x[b, ci, h, wc] = 1.0
        u = E.dd(x)
        kw, gap_ref, gout_ref = {}, None, None
        if form in ("mask_affine", "gate"):
            u = u * E.dd(sc).view(B, 64, 1, 1)
        y_ref = X.conv_ref(u, w64)
        if form == "plain":
            kw = dict(bias=dev["b"], relu=True)
            y_ref = torch.relu(y_ref + E.dd(bias).view(1, 64, 1, 1))
            gap_ref = y_ref.sum(dim=(2, 3))
        elif form == "mask_affine":
            kw = dict(mask=dev["m"], in_scale=dev["sc"], in_shift=dev["sh"])
            y_ref = y_ref * mask64
        elif form == "gate":
            kw = dict(bias=dev["b"], in_scale=dev["sc"], gate_add=dev["skip"])
            y_ref = y_ref + E.dd(bias).view(1, 64, 1, 1)
            gout_ref = u
        else:
            kw = dict(res=dev["res"], dot=dev["dot"])
            y_ref = y_ref + res64
            gap_ref = (y_ref * dot64).sum(dim=(2, 3))
        y, gap, gout = E.run_conv(E.dev4(x), pf, B, H, W, WINO, want_gap=gap_ref is not None, want_gout=gout_ref is not None, **kw)
        wrong = X.mismatch(y, y_ref)
        if wrong.any():
            i = wrong.nonzero()[0].tolist()
            bad.append(f"{form}, ci = {ci} (G {ci >> 4}, q {(ci >> 2) & 3}, e {ci & 3}), pixel (b {b}, h {h}, w {wc}) = {what}: "
                       f"{int(wrong.sum())} wrong outputs, first y{i} = {float(y[tuple(i)])} want {float(y_ref[tuple(i)])}")
        if gap_ref is not None and not torch.equal(gap.double().sum(dim=1), gap_ref):
            bad.append(f"{form}, ci = {ci}, e {ci & 3}, {what}: partial sums differ")
        if gout_ref is not None and not torch.equal(gout.double(), gout_ref):
            bad.append(f"{form}, ci = {ci}, e {ci & 3}, {what}: gate_out differs")
    assert not bad, f"{len(bad)} of {len(cases)} cases wrong:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("B,H,W", CONV_SHAPES)
def test_gate_out_is_the_gate_formula_bit_for_bit(B, H, W):
    """random normal x, g and skip: gate_out = fl(fl(x * g) + skip), the product rounded before the sum, as float32
    tensor arithmetic computes it; written for every pixel of the image and nothing else (NaN prefill)"""
    g = torch.Generator().manual_seed(41 + H)
    x, skip = torch.randn(B, 64, H, W, generator=g), torch.randn(B, 64, H, W, generator=g)
    sc = torch.randn(B, 64, generator=g)
    _, pf = packs("tap_sign")
    _, _, gout = E.run_conv(E.dev4(x), pf, B, H, W, WINO, want_gout=True, in_scale=sc.to(DEV), gate_add=E.dev4(skip), relu=True)
    want = E.dev4(x) * sc.to(DEV).view(B, 64, 1, 1) + E.dev4(skip)
    assert torch.equal(gout, want)


# ---------------------------------------------------------------------------------------------------- weight gradient
WGRAD_SHAPES = [(129, 32, 32), (2049, 8, 8), (9, 128, 128)]


def wgrad_places(B, H, W):
    """per channel o: (b, dY' pixel, x pixel, position of the x pixel in its block's 4 x 4 patch).  Channels 16 g .. 16 g + 15
    use block g of four blocks (given by their first output pixel: both block rows of a tile, both block-column parities kk,
    and on the larger maps a later tile row and column); the x pixel of channel o sits at patch row (o >> 2) & 3, column
    j = o & 3, and the dY' pixel of o is the pixel of the same block next to it (row pr >> 1, column pj >> 1 of the block)"""
    blocks = [(2, 2), (2, 4), (4, 2), (4, 4)]
    if H >= 12 and W >= 40:
        blocks = [(2, 2), (4, 36), (6, 34), (10, 4)]
    places = []
    for o in range(64):
        bh, bw = blocks[o >> 4]
        pr, pj = (o >> 2) & 3, o & 3
        hx, wx = bh - 1 + pr, bw - 1 + pj
        hy, wy = bh + (pr >> 1), bw + (pj >> 1)
        assert 0 <= hx < H and 0 <= wx < W and abs(hx - hy) <= 1 and abs(wx - wy) <= 1, "TEST BUG: placement"
        places.append((o % B, hy, wy, hx, wx, pr, pj))
    return places


@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("B,H,W", WGRAD_SHAPES)
def test_wgrad_one_hot_detector(B, H, W, affine):
    """one dY' pixel (value o + 1) and one x pixel (value 64 - o) per channel pair o = c: dw has one non-zero tap per matching
    pair and the products of the other pairs that meet, all small integers, exact against float64; outputs prefilled with
    NaN; plain and with dy_scale (powers of two) + dy_shift (multiples of 1/2, which makes dY' dense); two runs bit-identical"""
    assert B * H * W > T.THRESHOLD
    places = wgrad_places(B, H, W)
    assert {(p[5], p[6]) for p in places} == set(itertools.product(range(4), range(4))), "TEST BUG: patch positions not covered"
    assert {p[2] & 1 for p in places} == {0, 1} and {p[1] & 1 for p in places} == {0, 1}, "TEST BUG: dY' block positions"
    x, dy = torch.zeros(B, 64, H, W), torch.zeros(B, 64, H, W)
    for o, (b, hy, wy, hx, wx, _, _) in enumerate(places):
        dy[b, o, hy, wy] = o + 1
        x[b, o, hx, wx] = 64 - o
    kw, sc, sh = {}, None, None
    if affine:
        sc, sh = 2.0 ** X.ints((B, 64), 51, -1, 1), X.ints((B, 64), 52, -1, 1) / 2
        kw = dict(dy_scale=sc.to(DEV), dy_shift=sh.to(DEV))
    dw_ref, db_ref = T.exact_ref(x, dy, sc, sh)
    xd, dyd = T.dev4(x), T.dev4(dy)
    dw, db = T.run(xd, dyd, B, H, W, **kw)
    dw2, db2 = T.run(xd, dyd, B, H, W, **kw)
    assert not torch.isnan(dw).any() and not torch.isnan(db).any(), "an output was left unwritten"
    bad = X.mismatch(dw, dw_ref).nonzero().tolist()
    lines = []
    for o, c, ky, kx in bad[:12]:
        b, hy, wy, hx, wx, pr, pj = places[c]
        lines.append(f"dw[o={o}, c={c}, ky={ky}, kx={kx}] = {float(dw[o, c, ky, kx])} want {float(dw_ref[o, c, ky, kx])}: x pixel of c at "
                     f"patch row {pr}, column j = {pj} (pair {pj >> 1}, half {pj & 1}); dY' pixel of o at block row {places[o][1] & 1}, "
                     f"column {places[o][2] & 1}")
    assert not bad, f"{'affine' if affine else 'plain'}: {len(bad)} wrong taps:\n" + "\n".join(lines)
    X.assert_exact(db, db_ref, "db")
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two runs differ"


def test_bias_gradient_lane_to_channel_map():
    """the staging threads of wgrad3x3_c64_w4_kernel own channels [4 c8, 4 c8 + 4) and [32 + 4 c8, 32 + 4 c8 + 4) of a pixel
    column (conflict-free LDS writes) and sum dY' for the bias gradient in that map: one dY' pixel per channel, value
    o + 1, in a column of its own (a different tile column and staging thread per channel) -- db[o] = o + 1 exactly, and
    with dy_scale + dy_shift the per-sample affine values in the same channel order"""
    B, H, W = 33, 4, 1000
    x = X.ints((B, 64, H, W), 61, lo=-1, hi=1, zeros=0.75)
    dy = torch.zeros(B, 64, H, W)
    for o in range(64):
        dy[o % B, o, o % H, (37 * o + 5) % W] = o + 1
    xd, dyd = T.dev4(x), T.dev4(dy)
    dw_ref, db_ref = T.exact_ref(x, dy)
    assert db_ref.tolist() == [float(o + 1) for o in range(64)]
    dw, db = T.run(xd, dyd, B, H, W)
    X.assert_exact(db, db_ref, "plain db")
    X.assert_exact(dw, dw_ref, "plain dw")
    sc, sh = 2.0 ** X.ints((B, 64), 62, -1, 1), X.ints((B, 64), 63, 0, 1) * (torch.arange(64) % 4 + torch.arange(64) // 32 + 1).view(1, 64) / 2
    dw_ref, db_ref = T.exact_ref(x, dy, sc, sh)
    dw, db = T.run(xd, dyd, B, H, W, dy_scale=sc.to(DEV), dy_shift=sh.to(DEV))
    X.assert_exact(db, db_ref, "affine db")
    X.assert_exact(dw, dw_ref, "affine dw")
