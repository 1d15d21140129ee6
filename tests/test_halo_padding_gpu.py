"""Zero padding of the staged halos, decided per tile (csrc/conv_tiles.h halo_commit; pytest -m gpu).

The persistent fp32 64 -> 64 conv kernels (select 7: conv3x3_c64_p4_kernel; 12 / 14: conv3x3_c64_w4_kernel with the
straight-line / the predicated epilogue) zero what lies outside the image by scalar decisions of the tile: a halo row is
inside or outside for the whole workgroup, and in a full-width tile only halo column 0 (left image edge) and column 33
(right image edge) can be outside; width-ragged tiles keep the per-element predicate.  Every operand here is a dyadic
rational (tests/_exact.py) and x, the gate's skip map, in_shift and the weights have NO zero: a pixel of the neighbouring
row, sample or column read where a zero belongs changes the result, and the comparison with float64 has zero tolerance.

Shapes (B, H, W), one per branch:
  (2, 4, 32)      one tile per image, all four edges in it; two samples: a missed row mask reads the other sample's pixels
  (2, 5, 33)      ragged both ways: a second tile row with one valid row, a second tile column with one valid column
  (2, 12, 96)     3 x 3 tiles: each edge alone, each corner, one interior tile
  (3, 8, 64), (2, 7, 45), (1, 6, 64)   the walk / staging shapes of tests/test_exact_gpu.py
  (3, 100, 250)   a long ragged walk, several tiles per workgroup
Forms: plain, ReLU + GAP, residual, mask + affine (in_shift without a zero: padding is +0 AFTER the affine), GATE,
GATE + residual, DOT + residual; y and the summed partials equal float64, gate_out equals float64 and, bit for bit, the map
of the stand-alone gate kernel (ops.gate_mul); two launches give the same bits.  The chunked form (64 -> 256 through the
PixelShuffle view and its 256 -> 64 input gradient) runs at (2, 5, 33) and (2, 12, 96).

The weight gradient (whose kernels stage the same kind of halo) is exact at the same shapes, plain and with dy_scale /
dy_shift (no zero in the shift), under the default selection and with the Winograd form switched off; below
8 x 128^2 pixels per launch the rule selects the quadrant or the dense kernel either way, so (9, 128, 128) -- the step's
geometry, just above the threshold -- and (45, 30, 98), ragged both ways, run the Winograd kernel as well.
"""
import pytest
import torch

import _exact as X
import sisr_amd
import test_exact_gpu as E
import test_winograd_wgrad_gpu as WG
from test_winograd_chunks_gpu import packed_with_transform as packed_chunked

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
hip = sisr_amd.hip
DEV = "cuda:0"
NAN = float("nan")

SHAPES = [(2, 4, 32), (2, 5, 33), (2, 12, 96), (3, 8, 64), (2, 7, 45), (1, 6, 64), (3, 100, 250)]
SELECTS = [12, 14, 7]  # w4, w4 with the predicated epilogue, p4
FORMS = ["plain", "bias_relu_gap", "res_alpha", "mask_affine", "gate_relu", "gate_res", "dot_res"]


def bits(t):
    return t.contiguous().view(torch.int32)


class Data(E.ConvData):
    """E.ConvData with no zero in x, the skip map, in_shift and the weights"""

    def __init__(self, B, H, W, seed):
        s = (B, 64, H, W)
        super().__init__(B, H, W, seed, x=X.nonzero_ints(s, seed))
        self.w = X.weights((64, 64, 3, 3), seed + 1, nonzero=True)
        self.skip = X.nonzero_ints(s, seed + 4)
        self.sh = X.nonzero_ints((B, 64), seed + 8, m=4) / 4
        self.dev["skip"] = E.dev4(self.skip)
        self.dev["w"], self.dev["sh"] = self.w.to(DEV), self.sh.to(DEV)
        assert all(bool((t != 0).all()) for t in (self.x, self.w, self.skip, self.sh))


_SHAPE = {}


def shape_data(B, H, W):
    """operands, packings and the exact references of one shape (computed once, one shape resident at a time)"""
    if (B, H, W) not in _SHAPE:
        _SHAPE.clear()
        D = Data(B, H, W, seed=1300 + 11 * B + 5 * H + W)
        refs = {}
        for form in FORMS:
            pk, kw, y_ref, gap_ref, gout_ref, u, wk, extras = E.conv_case(form, D)
            E.conv_budget(u, wk, extras=extras, what=form)
            X.winograd_budget(u, wk, what=form)
            if gap_ref is not None:
                X.assert_budget((y_ref.abs() * (E.dd(D.dot).abs() if "dot" in kw else 1)).sum(dim=(2, 3)), X.granule(y_ref),
                                form + " partials")
            refs[form] = (pk, kw, y_ref, gap_ref, gout_ref)
        gate = ops.gate_mul(D.dev["x"], D.dev["sc"].view(B, 64, 1, 1), D.dev["skip"])  # the stand-alone gate kernel's map
        _SHAPE[(B, H, W)] = (D, {"plain": ops.pack_pair(D.dev["w"]), "wino": E.packed_with_transform(D.dev["w"])}, refs, gate)
    return _SHAPE[(B, H, W)]


@pytest.mark.parametrize("select", SELECTS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_conv_forms_exact(B, H, W, select):
    D, packs, refs, gate = shape_data(B, H, W)
    pf, pd = packs["plain" if select == 7 else "wino"]
    fails = []
    for form in FORMS:
        pk, kw, y_ref, gap_ref, gout_ref = refs[form]
        outs = [E.run_conv(D.dev["x"], pf if pk == "f" else pd, B, H, W, select, want_gap=gap_ref is not None,
                           want_gout=gout_ref is not None, **dict(kw)) for _ in range(2)]
        y, gap, gout = outs[0]
        try:
            X.assert_exact(y, y_ref, f"{form} output")
            if gap_ref is not None:
                X.assert_exact(gap.double().sum(dim=1), gap_ref, f"{form} partial sums (summed over slots)")
            if gout_ref is not None:
                X.assert_exact(gout, gout_ref, f"{form} gate_out")
                assert torch.equal(bits(gout), bits(gate)), f"{form}: gate_out differs from the stand-alone gate kernel's map"
            for name, a, b in zip(("y", "partials", "gate_out"), outs[0], outs[1]):
                assert a is None or torch.equal(bits(a), bits(b)), f"{form}: two launches differ in {name}"
        except AssertionError as e:
            fails.append(f"select {select}: {e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("select", [12, 14])
@pytest.mark.parametrize("B,H,W", [(2, 5, 33), (2, 12, 96)])
def test_chunked_form_exact(B, H, W, select):
    """64 -> 256 stored through the PixelShuffle(2) view and the 256 -> 64 input gradient read through it.  Weights are
    multiples of 1/2 (the transform G g G^T divides by 4 at most), maps non-zero integers: exact."""
    r, rr = 2, 4
    x = X.nonzero_ints((B, 64, H, W), 1400 + H)
    dy = X.nonzero_ints((B, 64, r * H, r * W), 1401 + H)
    w = X.nonzero_ints((64 * rr, 64, 3, 3), 1402, m=2) / 2
    b = X.biases(64 * rr, 1403)
    E.conv_budget(x, w, extras=(b,), what="chunked forward")
    X.winograd_budget(E.dd(x), E.dd(w), what="chunked forward")
    dyc = torch.nn.functional.pixel_unshuffle(E.dd(dy), r)
    wt = E.dd(w).flip(2, 3).transpose(0, 1)
    X.conv_budget(dyc, wt, what="chunked input gradient")
    X.winograd_budget(dyc, wt, what="chunked input gradient")
    pf, pd = packed_chunked(w.to(DEV), r)
    vp, vs = hip.view_plain(H, W, 64), hip.view_shuffle(H, W, r)
    ys, dxs = [], []
    for _ in range(2):
        y = E.nan4(B, 64, r * H, r * W)
        ops.conv_c64(E.dev4(x), vp, pf, b.to(DEV), (rr, 1), y, vs, B, H, W, 64, 64 * rr, select=select)
        dx = E.nan4(B, 64, H, W)
        ops.conv_c64(E.dev4(dy), vs, pd, None, (1, 64), dx, vp, B, H, W, 64 * rr, 64, alpha=X.ALPHA, select=select)
        ys.append(y)
        dxs.append(dx)
    X.assert_exact(ys[0], torch.nn.functional.pixel_shuffle(X.conv_ref(E.dd(x), E.dd(w), E.dd(b)), r), "chunked forward")
    X.assert_exact(dxs[0], X.ALPHA * X.dgrad_ref(dyc, E.dd(w)), "chunked input gradient")
    assert torch.equal(bits(ys[0]), bits(ys[1])) and torch.equal(bits(dxs[0]), bits(dxs[1])), "two launches differ"


# ------------------------------------------------------------------------------------------------- weight gradient
# (45, 30, 98), ragged both ways, and (9, 128, 128) hold more than 8 x 128^2 pixels: the Winograd kernel under the default
# switches.  A sum over that many pixels fits the exact-data budget only with a sparse x (as in
# tests/test_winograd_wgrad_gpu.py), so there x is +-1 on the two outermost rows and columns of every image -- the kernels
# clamp their addresses into the image, so what a missed mask reads instead of a zero is one of those pixels -- and
# three quarters zero inside; dY is +-1 everywhere.  The smaller shapes have no zero at all.
LARGE = [(45, 30, 98), (9, 128, 128)]
WGRAD_SHAPES = SHAPES + LARGE


def border_dense(shape, seed):
    t = X.nonzero_ints(shape, seed, m=1)
    kill = torch.rand(shape, generator=torch.Generator().manual_seed(seed + 1)) < 0.75
    kill[:, :, :2] = False
    kill[:, :, -2:] = False
    kill[..., :2] = False
    kill[..., -2:] = False
    t[kill] = 0.0
    return t


@pytest.mark.parametrize("B,H,W", WGRAD_SHAPES)
def test_weight_gradient_exact(B, H, W):
    """dw and db against float64, plain and with dy_scale in {1, 2} / dy_shift = +-1 (no zero in the shift), under the
    default selection and with the Winograd form switched off (the dense or the quadrant kernel); two launches each."""
    wino = B * H * W > WG.THRESHOLD
    assert wino == ((B, H, W) in LARGE)
    x = border_dense((B, 64, H, W), 1500 + H) if wino else X.nonzero_ints((B, 64, H, W), 1500 + H, m=1)
    dy = X.nonzero_ints((B, 64, H, W), 1501 + W, m=1)
    sc, sh = X.ints((B, 64), 1502, 1, 2), X.nonzero_ints((B, 64), 1503, m=1)
    xd, dyd = E.dev4(x), E.dev4(dy)
    for opts, kw in ((dict(), dict()), (dict(sc=sc, sh=sh), dict(dy_scale=sc.to(DEV), dy_shift=sh.to(DEV)))):
        dw_ref, db_ref = WG.exact_ref(x, dy, **opts) if wino else E.wgrad_exact(x, dy, **opts)[:2]
        for switches in (WG.WINO, WG.DIRECT):
            what = f"{'default' if switches is WG.WINO else 'Winograd off'} {list(kw)}"
            outs = [WG.run(xd, dyd, B, H, W, switches=switches, **kw) for _ in range(2)]
            X.assert_exact(outs[0][0], dw_ref, what + " dw")
            X.assert_exact(outs[0][1], db_ref, what + " db")
            assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1])), \
                what + ": two launches differ"
