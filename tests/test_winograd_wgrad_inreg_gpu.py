"""wgrad3x3_c64_w4_kernel with the Winograd operands built in registers (no V / M chunks in LDS): each lane reads the raw
4 x 4 input patch and 2 x 2 dY' block of its (block, channel) slot and transforms them itself.  Shapes that put that
mapping on its edges (the form is selected only above 8 x 128^2 pixels per launch), a detector that names a wrong
lane -> (block, channel) slot, and the hand-over of the raw image between tiles."""
import pytest
import torch

import _exact as X
import test_winograd_wgrad_gpu as T

pytestmark = pytest.mark.gpu
DEV = T.DEV


@pytest.mark.parametrize("B,H,W", [
    (2049, 8, 8),      # every tile is an edge tile: 8 of 32 columns valid, block columns >= 4 all padding
    (65, 46, 44),      # last tile row: block row 1 fully outside; second tile column 12 pixels wide
    (33, 4, 1000),     # one tile row, 32 tile columns, the last 8 pixels wide; many tiles per workgroup
    (9, 128, 128),     # the interior path with prefetch
])
def test_exact_on_the_edges_of_the_lane_mapping(B, H, W):
    """x in {-1, 0, 1} (3/4 zeros), dY in {-1, 0, 1}: dw and db bit-equal to float64, plain and with dy_scale + dy_shift
    (halves) + alpha; outputs prefilled with NaN (T.run), none may remain; the budget is asserted before each comparison"""
    assert B * H * W > T.THRESHOLD
    x = X.ints((B, 64, H, W), 700 + H, lo=-1, hi=1, zeros=0.75)
    dy = X.ints((B, 64, H, W), 701 + W, lo=-1, hi=1)
    xd, dyd = T.dev4(x), T.dev4(dy)
    dw_ref, db_ref = T.exact_ref(x, dy)
    dw, db = T.run(xd, dyd, B, H, W)
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    X.assert_exact(dw, dw_ref, "plain dw")
    X.assert_exact(db, db_ref, "plain db")
    sc, sh = X.scales((B, 64), 702), X.ints((B, 64), 703) / 2
    dw_ref, db_ref = T.exact_ref(x, dy, sc, sh, X.ALPHA)
    dw, db = T.run(xd, dyd, B, H, W, alpha=X.ALPHA, dy_scale=sc.to(DEV), dy_shift=sh.to(DEV))
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    X.assert_exact(dw, dw_ref, "affine dw")
    X.assert_exact(db, db_ref, "affine db")


# columns of the dY' pixels: blocks 0 / 1 and 15 of the first tile, the first blocks of the second, the halo on both sides
# of a tile boundary (dY' at 31 with x at 32, dY' at 32 with x at 31), the last tile's last block
DET_W = [0, 1, 2, 3, 30, 31, 32, 33, 63, 64, 65, 95, 96, 126, 127]


def _detector_places(H, W, B):
    """channel c: dY' pixel (b, h, w) of output channel c, x pixel of input channel c one tap (ky, kx) away"""
    places = []
    for c in range(64):
        b, h, w = c % B, (5 * c) % H, DET_W[c % len(DET_W)]
        tap = (2 * c + c // 15) % 9
        ky, kx = tap // 3, tap % 3
        hx, wx = h + ky - 1, w + kx - 1
        if not 0 <= hx < H:
            ky, hx = 2 - ky, h - (ky - 1)
        if not 0 <= wx < W:
            kx, wx = 2 - kx, w - (kx - 1)
        places.append((b, h, w, ky, kx, hx, wx))
    return places


def test_tap_placement_detector():
    """one pixel per input channel and one per output channel: dw has one non-zero tap per matching pair (o = c) and zeros
    elsewhere, bit-equal to float64; a wrong tap is reported with the K-step, block parity and lanes of the slot that feeds it"""
    B, H, W = 9, 128, 128
    places = _detector_places(H, W, B)
    # what the placement covers (a TEST BUG otherwise): block rows 0 and 1, block columns 0, 15 and the next tile's first,
    # both block parities, and x pixels in the halo's edge columns (left of a tile's first column, right of its last)
    assert {(h % 4) // 2 for _, h, *_ in places} == {0, 1}
    assert {0, 15} <= {(w % 32) // 2 for _, _, w, *_ in places} and any(w // 32 == 1 and (w % 32) // 2 == 0 for _, _, w, *_ in places)
    assert {((w % 32) // 2) & 1 for _, _, w, *_ in places} == {0, 1}
    assert any(w % 32 == 0 and wx == w - 1 for _, _, w, _, _, _, wx in places if w)
    assert any(w % 32 == 31 and wx == w + 1 for _, _, w, _, _, _, wx in places if w < W - 1)
    x, dy = torch.zeros(B, 64, H, W), torch.zeros(B, 64, H, W)
    for c, (b, h, w, ky, kx, hx, wx) in enumerate(places):
        dy[b, c, h, w] = c + 1
        x[b, c, hx, wx] = 64 - c
    dw_ref, db_ref = T.exact_ref(x, dy)
    nz = dw_ref.nonzero().tolist()
    assert sorted(nz) == sorted([c, c, p[3], p[4]] for c, p in enumerate(places)), "TEST BUG: pairs other than o = c meet"
    dw, db = T.run(T.dev4(x), T.dev4(dy), B, H, W)
    bad = X.mismatch(dw, dw_ref).nonzero().tolist()
    lines = []
    for o, c, ky, kx in bad[:12]:
        b, h, w = places[o][:3]
        blk = ((h % 4) // 2) * 16 + (w % 32) // 2
        lines.append(f"dw[o={o}, c={c}, ky={ky}, kx={kx}] = {float(dw[o, c, ky, kx])} want {float(dw_ref[o, c, ky, kx])}: dY' pixel "
                     f"of o at (b={b}, h={h}, w={w}) = tile column {w // 32}, block {blk} (K-step {blk >> 1}, kk {blk & 1}), "
                     f"B lane {o % 32} of co half {o // 32}; A lane {c % 32} of ci half {c // 32}")
    assert not bad, f"{len(bad)} wrong taps:\n" + "\n".join(lines)
    X.assert_exact(db, db_ref, "db")


@pytest.mark.parametrize("B,H,W", [(9, 128, 128), (33, 4, 1000)])
def test_hand_over_and_determinism(B, H, W):
    """random normal data with dy_scale + dy_shift + alpha: two launches give the same bits (a K-loop read racing the next
    tile's commit would not), within 1e-5 of float64 and at most 3x the direct form's max error"""
    assert B * H * W > T.THRESHOLD
    x, dy = T.rnd(B, 64, H, W, seed=710), T.rnd(B, 64, H, W, seed=711)
    sc, sh = T.rnd(B, 64, seed=712).abs() + 0.5, T.rnd(B, 64, seed=713)
    xd, dyd = T.dev4(x), T.dev4(dy)
    kw = dict(dy_scale=sc.to(DEV), dy_shift=sh.to(DEV), alpha=0.7)
    dyp = T.dd(dy) * T.dd(sc).view(B, 64, 1, 1) + T.dd(sh).view(B, 64, 1, 1)
    want, want_b = 0.7 * X.wgrad_ref(T.dd(x), dyp), 0.7 * dyp.sum(dim=(0, 2, 3))
    dw_w, db_w = T.run(xd, dyd, B, H, W, **kw)
    dw_w2, db_w2 = T.run(xd, dyd, B, H, W, **kw)
    dw_d, db_d = T.run(xd, dyd, B, H, W, switches=T.DIRECT, **kw)
    assert torch.equal(dw_w, dw_w2) and torch.equal(db_w, db_w2), "two runs differ"
    assert not torch.equal(dw_w, dw_d), "the Winograd form did not engage"
    scale = float(want.abs().max())
    err_w = float((dw_w.double() - want).abs().max()) / scale
    err_d = float((dw_d.double() - want).abs().max()) / scale
    print(f"max |err| / max |dw|: winograd {err_w:.3e}, direct {err_d:.3e}")
    assert err_d < 1e-5 and err_w < 1e-5
    assert err_w <= 3 * err_d
    err_b = float((db_w.double() - want_b).abs().max()) / float(want_b.abs().max())
    assert err_b < 1e-5
