"""Winograd F(2x2,3x3) conv with the A fragments built in registers (conv3x3_c64_w4_kernel): every form it is instantiated
for, forced with select 12 on a packing that carries the transform, bit for bit against float64 on exact data
(tests/_exact.py, the budget asserted before each comparison), on the shapes at which its wave / lane mapping, tile walk and
halo hand-over change path:

  (1, 4, 32)      exactly one tile
  (1, 3, 5)       tile row mb = 1 partly outside the image, 3 valid Winograd tile columns
  (1, 6, 34)      4 tiles: grid no multiple of 8, second tile row half empty, last tile column 2 pixels wide
  (2, 9, 65)      odd sizes
  (3, 100, 250)   600 tiles, ragged, more than one tile per workgroup through the per-XCD walk
  (5, 128, 128)   640 tiles, the interior path with a next tile to prefetch

The partial-sum slots are compared with the direct persistent form's (exact data: equal bit for bit), and a hand-over race
detector runs six copies of one random map as one batch: every copy, and a second launch, must give the same bits.
"""
import pytest
import torch

import _exact as X
import sisr_amd
import test_exact_gpu as E

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
hip = sisr_amd.hip
DEV = "cuda:0"
WINO, DIRECT = ops.SELECT_WINOGRAD_FORCE, 7

SHAPES = [(1, 4, 32), (1, 3, 5), (1, 6, 34), (2, 9, 65), (3, 100, 250), (5, 128, 128)]
# <AFFINE, MASK, RES, GATE, DOT>: plain (bias, ReLU, GAP), <1,1,0,0,0>, <0,0,1,0,0>, <0,0,0,1,0>, <0,0,1,1,0>, <0,0,1,0,1>
# and the two remaining instantiations <0,1,0,0,0>, <0,0,0,0,1>
FORMS = ["bias_relu_gap", "mask_affine", "res_alpha", "gate_relu", "gate_res", "dot_res", "mask", "dot"]

_DATA = {}


def data(B, H, W):
    """one set of exact operands and packings per shape, shared by the forms"""
    key = (B, H, W)
    if key not in _DATA:
        _DATA.clear()  # one shape resident at a time
        D = E.ConvData(B, H, W, seed=600 + B + H + W)
        _DATA[key] = (D, E.packed_with_transform(D.dev["w"]))
    return _DATA[key]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_every_form_exact_against_float64(B, H, W, form):
    D, packs = data(B, H, W)
    fail = E.check_conv_case(form, D, packs, WINO, winograd=True)
    assert fail is None, fail


@pytest.mark.parametrize("form", ["bias_relu_gap", "dot_res"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_partial_slots_equal_the_direct_forms(B, H, W, form):
    """slot (tile, tile row mb) is written by wave (mb, coh) for its 32 channels: on exact data every slot holds the exact
    sum of its 2 x 32 pixel strip, so it equals the direct persistent form's slot bit for bit (NaN prefill: none unwritten)"""
    D, packs = data(B, H, W)
    pk, kw, y_ref, gap_ref, _, u, wk, extras = E.conv_case(form, D)
    E.conv_budget(u, wk, extras=extras, what=form)
    X.winograd_budget(u, wk, what=form)
    X.assert_budget((y_ref.abs() * (E.dd(D.dot).abs() if "dot" in kw else 1)).sum(dim=(2, 3)), X.granule(y_ref), form + " partials")
    got = {}
    for sel in (WINO, DIRECT):
        _, gap, _ = E.run_conv(D.dev["x"], packs[0] if pk == "f" else packs[1], B, H, W, sel, want_gap=True, **dict(kw))
        got[sel] = gap
    assert not got[WINO].isnan().any(), "a partial-sum slot was left unwritten"
    assert torch.equal(got[WINO], got[DIRECT])


@pytest.mark.parametrize("gate", [False, True])
def test_halo_handover_race_detector(gate):
    """Six copies of one random 128 x 128 map as a batch (768 tiles, 1.5 tiles per workgroup: the next tile's halo is
    written while other waves may still be in this tile's K loop or epilogue).  Each copy sees the same values whatever
    workgroup, tile order and prefetch state it meets, so all six outputs and partial sums, and those of a second launch,
    must be the same bits."""
    H = W = 128
    g = torch.Generator().manual_seed(77)
    one = lambda: torch.randn(1, 64, H, W, generator=g).expand(6, 64, H, W)  # noqa: E731
    x, skip = E.dev4(one()), E.dev4(one())
    w = (torch.randn(64, 64, 3, 3, generator=g) * 0.05).to(DEV)
    b = torch.randn(64, generator=g).to(DEV)
    sc = torch.rand(1, 64, generator=g).expand(6, 64).contiguous().to(DEV)
    pf, _ = E.packed_with_transform(w)
    kw = dict(bias=b, relu=True)
    if gate:
        kw.update(in_scale=sc, gate_add=skip)
    runs = [E.run_conv(x, pf, 6, H, W, WINO, want_gap=True, want_gout=gate, **dict(kw)) for _ in range(2)]
    for y, gap, gout in runs:
        for t in (y, gap) + ((gout,) if gate else ()):
            assert not t.isnan().any()
            for i in range(1, 6):
                assert torch.equal(t[i], t[0]), f"copy {i} differs from copy 0"
    for a, c in zip(runs[0], runs[1]):
        if a is not None:
            assert torch.equal(a, c), "two launches differ"
