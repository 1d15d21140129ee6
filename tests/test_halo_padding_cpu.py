"""The per-tile padding rules of the staged halos, restated in numpy and compared with the per-element predicate.

csrc/conv_tiles.h halo_commit (conv3x3_c64_p4_kernel / conv3x3_c64_w4_kernel): a tile of TH x TW = 4 x 32 output pixels at
(h0, w0) stages halo rows r = 0..5 (image row gh = h0 - 1 + r) and halo columns col = pcol + 16 k (image column
gw = w0 - 1 + col), k = 0..2, staging lane pcol = 0..15, the k = 2 piece for pcol < 2 only.  A piece is padding (written as
+0) exactly where the per-element predicate `0 <= gh < H && 0 <= gw < W && col < HALO_W` fails.  The kernel decides it

  width-ragged tile (w0 + TW > W)   by that predicate, per element
  full-width tile                   row r outside the image (scalar): every piece of the row;
                                    w0 == 0 (scalar): the k = 0 piece of the lanes with pcol == 0;
                                    w0 + TW == W (scalar): the k = 2 piece of the lanes with pcol == 1; nothing else

and the GATE prologue stores a piece to gate_out where `rown && cok && 1 <= col <= TW` (rown: r in 1..TH and gh < H), in a
full-width tile decided as rown (scalar) and k == 1, or k == 0 and pcol != 0, or k == 2 and pcol == 0.

csrc/wgrad3x3_mfma.hip wgrad3x3_c64_w4_kernel: tiles of 4 x 32 pixels, halo rows r = 0..5, main columns w0 + pcol
(pcol = 0..31), dY rows h0 + r (r = 0..3); the two edge columns keep their per-lane mask.  Interior tiles mask nothing; a
tile whose pixels are all inside the image zeroes halo row 0 where h0 == 0 and halo row 5 where h0 + 4 == H, nothing else;
ragged tiles use the per-element predicates `0 <= gh < H && w0 + pcol < W` (x) and `h0 + r < H && w0 + pcol < W` (dY).

Both sets -- the pieces the scalar rules zero / store and the pieces the predicate does -- must be equal for every tile of
every shape, the GPU test's (tests/test_halo_padding_gpu.py) and a few more.
"""
import itertools

import pytest

TH, TW = 4, 32
HALO_H, HALO_W = TH + 2, TW + 2
SIZES = [(4, 32), (5, 33), (12, 96), (8, 64), (7, 45), (6, 64), (100, 250), (128, 128), (8, 20), (3, 5), (1, 1), (4, 33),
         (9, 64), (30, 98)]


def tiles(H, W):
    return list(itertools.product(range(0, H, TH), range(0, W, TW)))


def pieces():
    """(r, k, pcol) of every staged 16-byte piece (per channel group)"""
    return [(r, k, pcol) for r in range(HALO_H) for k in range(3) for pcol in range(16) if k < 2 or pcol < 2]


def test_the_staged_pieces_cover_the_halo_once():
    cols = sorted(pcol + 16 * k for r, k, pcol in pieces() if r == 0)
    assert cols == list(range(HALO_W))


def padding_by_predicate(H, W, h0, w0):
    out = set()
    for r, k, pcol in pieces():
        col = pcol + 16 * k
        gh, gw = h0 - 1 + r, w0 - 1 + col
        if not (0 <= gh < H and 0 <= gw < W and col < HALO_W):
            out.add((r, k, pcol))
    return out


def padding_by_tile_rules(H, W, h0, w0):
    if w0 + TW > W:  # the ragged fallback is the predicate itself
        return padding_by_predicate(H, W, h0, w0)
    left, right = w0 == 0, w0 + TW == W
    out = set()
    for r, k, pcol in pieces():
        gh = h0 - 1 + r
        row_outside = gh < 0 or gh >= H
        if row_outside or (k == 0 and left and pcol == 0) or (k == 2 and right and pcol == 1):
            out.add((r, k, pcol))
    return out


def stores_by_predicate(H, W, h0, w0):
    out = set()
    for r, k, pcol in pieces():
        col = pcol + 16 * k
        gh, gw = h0 - 1 + r, w0 - 1 + col
        rown = 1 <= r <= TH and gh < H
        cok = 0 <= gw < W and col < HALO_W
        if rown and cok and 1 <= col <= TW:
            out.add((r, k, pcol))
    return out


def stores_by_tile_rules(H, W, h0, w0):
    if w0 + TW > W:
        return stores_by_predicate(H, W, h0, w0)
    out = set()
    for r, k, pcol in pieces():
        rown = 1 <= r <= TH and h0 - 1 + r < H
        if rown and (k == 1 or (k == 0 and pcol != 0) or (k == 2 and pcol == 0)):
            out.add((r, k, pcol))
    return out


@pytest.mark.parametrize("H,W", SIZES)
def test_conv_padding_rules_equal_the_predicate(H, W):
    interior = one_edge = 0
    for h0, w0 in tiles(H, W):
        want, got = padding_by_predicate(H, W, h0, w0), padding_by_tile_rules(H, W, h0, w0)
        assert got == want, (h0, w0, sorted(got ^ want)[:6])
        if h0 >= 1 and h0 + TH + 1 <= H and w0 >= 1 and w0 + TW + 1 <= W:
            assert not want, "an interior tile has no padding"
            interior += 1
        # the pieces a side edge costs: six rows of one piece, one lane group
        if w0 + TW <= W and h0 >= 1 and h0 + TH + 1 <= H and (w0 == 0) != (w0 + TW == W):
            assert len(want) == HALO_H
            one_edge += 1
    if (H, W) == (128, 128):  # the step's map: the tile mix the counters are weighted with
        assert (interior, one_edge, len(tiles(H, W))) == (60, 60, 128)


@pytest.mark.parametrize("H,W", SIZES)
def test_gate_out_store_rules_equal_the_predicate(H, W):
    owned = set()
    for h0, w0 in tiles(H, W):
        want, got = stores_by_predicate(H, W, h0, w0), stores_by_tile_rules(H, W, h0, w0)
        assert got == want, (h0, w0, sorted(got ^ want)[:6])
        for r, k, pcol in got:
            px = (h0 - 1 + r, w0 - 1 + pcol + 16 * k)
            assert px not in owned, "a pixel of gate_out is written by one tile only"
            owned.add(px)
    assert owned == set(itertools.product(range(H), range(W)))


# ------------------------------------------------------------------------------------------------- weight gradient
W4_TH, WT_W = 4, 32
W4_HH = W4_TH + 2


def wgrad_by_predicate(H, W, h0, w0):
    """-> (zeroed x pieces (r, pcol), zeroed dY pieces (r, pcol)) of the per-element masks, which interior tiles skip"""
    interior = h0 >= 1 and h0 + W4_TH + 1 <= H and w0 >= 1 and w0 + WT_W + 1 <= W
    xs = {(r, pc) for r in range(W4_HH) for pc in range(WT_W) if not (0 <= h0 - 1 + r < H and w0 + pc < W)}
    ys = {(r, pc) for r in range(W4_TH) for pc in range(WT_W) if not (h0 + r < H and w0 + pc < W)}
    if interior:
        assert not xs and not ys
    return xs, ys


def wgrad_by_tile_rules(H, W, h0, w0):
    interior = h0 >= 1 and h0 + W4_TH + 1 <= H and w0 >= 1 and w0 + WT_W + 1 <= W
    full = h0 + W4_TH <= H and w0 + WT_W <= W
    if interior:
        return set(), set()
    if not full:
        return wgrad_by_predicate(H, W, h0, w0)
    rows = ([0] if h0 == 0 else []) + ([W4_HH - 1] if h0 + W4_TH == H else [])
    return {(r, pc) for r in rows for pc in range(WT_W)}, set()


@pytest.mark.parametrize("H,W", SIZES)
def test_weight_gradient_rules_equal_the_predicates(H, W):
    for h0, w0 in itertools.product(range(0, H, W4_TH), range(0, W, WT_W)):
        assert wgrad_by_tile_rules(H, W, h0, w0) == wgrad_by_predicate(H, W, h0, w0), (h0, w0)
        # the edge columns (w0 - 1 and w0 + 32, six rows) keep their per-lane mask on every tile that is not interior:
        # an interior tile must have none of them outside the image
        if h0 >= 1 and h0 + W4_TH + 1 <= H and w0 >= 1 and w0 + WT_W + 1 <= W:
            assert all(0 <= h0 - 1 + r < H and 0 <= gw < W for r in range(W4_HH) for gw in (w0 - 1, w0 + WT_W))
