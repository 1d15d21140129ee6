"""The output addresses of conv3x3_c64_w4_kernel's two epilogues, restated in numpy (uint32 arithmetic, as the kernel's).

Wave (mb, coh), lane (n = l & 15, q = l >> 4), N block nb and register (i, j, r) hold output pixel
(h0 + 2 mb + i, w0 + 8 q + 2 r + j), channel co + 16 nb with co = 32 coh + n.  Every access is
resource base (y + b sB + chunk) + lane byte offset + scalar byte offset + immediate:

  predicated form   lane ((col sW + co + 16 nb) 4), scalar (row sH 4), no immediate, under row < H and col < W
  full-tile form    lane ((8 q sW + co) 4), scalar (((h0 + 2 mb) sH + w0 sW) 4 + i sH 4 + (2 r + j) sW 4), immediate 64 nb,
                    no predicate: taken where h0 + 4 <= H and w0 + 32 <= W

The full-tile sum must be the predicated one for every wave, lane, N block and register of every full tile, lie inside the
batch image, and the tile test must fail exactly for the tiles that have a pixel outside the image.  Shapes: the plain
view at (3, 8, 64) and (3, 100, 250), and the 64 -> 256 conv stored through the PixelShuffle(2) view at (2, 8, 32).
"""
import itertools

import numpy as np
import pytest

TH, TW = 4, 32
HUGE = 1 << 30
U32 = np.uint32


def view_plain(H, W, C=64):
    return dict(sB=H * W * C, sH=W * C, sW=C, chi=0, clo=64, cdiv=HUGE)


def view_shuffle(H, W, r):
    rH, rW = r * H, r * W
    return dict(sB=rH * rW * 64, sH=r * rW * 64, sW=r * 64, chi=rW * 64, clo=64, cdiv=r)


def chunk(v, q):
    return (q // v["cdiv"]) * v["chi"] + (q % v["cdiv"]) * v["clo"]


def u32(x):
    return np.asarray(x, dtype=np.int64).astype(U32)


LANE = np.arange(64)
N, Q = LANE & 15, LANE >> 4
# registers in the kernel's order: (nb, i, j, r)
REGS = list(itertools.product(range(2), range(2), range(2), range(4)))


def predicated(v, H, W, h0, w0, mb, coh, nb, i, j, r):
    """-> (byte offsets of the 64 lanes, the lanes' store predicate), as the predicated epilogue forms them"""
    co = 32 * coh + N
    row, col = h0 + 2 * mb + i, w0 + 8 * Q + 2 * r + j
    with np.errstate(over="ignore"):
        vo = u32(col * v["sW"] + co + 16 * nb) * U32(4)
        so = U32(row * v["sH"]) * U32(4)
        return vo + so, (row < H) & (col < W)


def full_tile(v, h0, w0, mb, coh, nb, i, j, r):
    """-> byte offsets of the 64 lanes as the full-tile epilogue forms them: lane offset + scalar offset + immediate"""
    co = 32 * coh + N
    with np.errstate(over="ignore"):
        sHb, sWb = U32(v["sH"]) * U32(4), U32(v["sW"]) * U32(4)
        loff = u32(8 * Q * v["sW"] + co) * U32(4)
        s0 = U32(h0 + 2 * mb) * sHb + U32(w0) * sWb
        so = s0 + U32(i) * sHb + U32(2 * r + j) * sWb
        imm = U32(64 * nb)
        assert 0 <= int(imm) < 4096  # the buffer instruction's 12-bit immediate
        return loff + so + imm


def tile_is_full(H, W, h0, w0):
    return h0 + TH <= H and w0 + TW <= W


CASES = [("plain", 3, 8, 64, 1), ("plain", 3, 100, 250, 1), ("shuffle", 2, 8, 32, 2)]


def case_view(kind, H, W, r):
    return view_plain(H, W) if kind == "plain" else view_shuffle(H, W, r)


@pytest.mark.parametrize("kind,B,H,W,r", CASES)
def test_full_tile_offsets_equal_the_predicated_ones(kind, B, H, W, r):
    v = case_view(kind, H, W, r)
    chunks = r * r
    image_bytes = v["sB"] * 4
    assert image_bytes * B < 2 ** 32
    n_full = 0
    seen = np.zeros(v["sB"], dtype=np.int32)  # floats of one batch image: how many (tile, chunk, lane, register) write it
    for h0, w0 in itertools.product(range(0, H, TH), range(0, W, TW)):
        if not tile_is_full(H, W, h0, w0):
            continue
        n_full += 1
        for oq, mb, coh, (nb, i, j, rr) in itertools.product(range(chunks), range(2), range(2), REGS):
            base = chunk(v, oq) * 4  # of the resource, from the batch image's first byte
            want, ok = predicated(v, H, W, h0, w0, mb, coh, nb, i, j, rr)
            got = full_tile(v, h0, w0, mb, coh, nb, i, j, rr)
            assert ok.all(), "a full tile has no masked element"
            assert np.array_equal(got, want), (h0, w0, oq, mb, coh, nb, i, j, rr)
            at = got.astype(np.int64) + base
            assert (at >= 0).all() and (at + 4 <= image_bytes).all() and (at % 4 == 0).all()
            np.add.at(seen, at // 4, 1)
    assert n_full == (H // TH) * (W // TW) and n_full > 0
    # every float of the full tiles' pixels is written exactly once (the layouts are dense: 64 r^2 channels per pixel)
    assert seen.max() == 1 and int(seen.sum()) == n_full * TH * TW * 64 * chunks


@pytest.mark.parametrize("H,W", [(8, 64), (100, 250), (7, 45), (6, 64), (8, 20), (4, 32), (3, 5), (5, 33)])
def test_tile_condition_is_false_exactly_for_ragged_tiles(H, W):
    tiles = list(itertools.product(range(0, H, TH), range(0, W, TW)))
    assert len(tiles) == ((H + TH - 1) // TH) * ((W + TW - 1) // TW)
    for h0, w0 in tiles:
        outside = any(h0 + dh >= H or w0 + dw >= W for dh in range(TH) for dw in range(TW))
        assert tile_is_full(H, W, h0, w0) == (not outside), (h0, w0)
    if H % TH == 0 and W % TW == 0:
        assert all(tile_is_full(H, W, h0, w0) for h0, w0 in tiles)


@pytest.mark.parametrize("kind,B,H,W,r", CASES)
def test_predicated_offsets_stay_inside_the_image_on_ragged_tiles(kind, B, H, W, r):
    """the other branch, for the tiles the condition refuses: its stored elements are inside the batch image"""
    v = case_view(kind, H, W, r)
    for h0, w0 in itertools.product(range(0, H, TH), range(0, W, TW)):
        if tile_is_full(H, W, h0, w0):
            continue
        for oq, mb, coh, (nb, i, j, rr) in itertools.product(range(r * r), range(2), range(2), REGS):
            off, ok = predicated(v, H, W, h0, w0, mb, coh, nb, i, j, rr)
            at = off.astype(np.int64)[ok] + chunk(v, oq) * 4
            assert (at + 4 <= v["sB"] * 4).all()
