"""wgrad3x3_c64_w4_kernel with one Winograd transform row per wave: wave xr builds row xr of B^T d B and of A dY' A^T for all
64 ci x 64 co (channels i and 32 + i per lane), and the four rows of an element meet in the end-of-kernel exchange, where
wave w folds the registers [4 w, 4 w + 4).  Only shapes just over the form's threshold (more than 8 x 128^2 pixels per launch):
a detector that names a swapped channel half, a wrong row pair or sign and a wrong folding wave, the edge-tile shapes with
dy_scale + dy_shift and the bias gradient (the exchange shares LDS with the bias reduction), a multi-pair grid, determinism."""
import pytest
import torch

import _exact as X
import test_winograd_wgrad_gpu as T

pytestmark = pytest.mark.gpu
DEV = T.DEV

# wave xr: raw patch rows (ra, rb) and sign of d_ra + s d_rb; the taps kh (and kw) that transform row (column) xr reaches
# through the fold G^T dU G
ROWS = [(0, 2, "-"), (1, 2, "+"), (2, 1, "-"), (1, 3, "-")]
FEEDS = {0: (0, 1, 2), 1: (1, 2), 2: (1, 2, 3)}
DET_W = [0, 1, 3, 30, 31, 32, 33, 63, 64, 65, 94, 95, 96, 124, 125, 127]


def _detector_places(H, W, B):
    """channel c: dY' pixel (b, h, w) of output channel c, x pixel of input channel c one tap (ky, kx) away; channel c + 32
    sits one block column further (the other block parity, the other lane half of a K-step) on another tap"""
    places = []
    for c in range(64):
        lo, hi = c % 32, c // 32
        b, h = c % B, (5 * c) % H
        w = DET_W[lo % len(DET_W)]
        w = w + 2 if hi and w + 2 < W else (w - 2 if hi else w)
        tap = (2 * lo + lo // 9 + 4 * hi) % 9
        ky, kx = tap // 3, tap % 3
        hx, wx = h + ky - 1, w + kx - 1
        if not 0 <= hx < H:
            ky, hx = 2 - ky, h - (ky - 1)
        if not 0 <= wx < W:
            kx, wx = 2 - kx, w - (kx - 1)
        places.append((b, h, w, ky, kx, hx, wx))
    return places


def test_quadrant_and_row_detector():
    """one pixel per input channel and one per output channel: dw has one non-zero tap per pair o = c and zeros elsewhere,
    bit-equal to float64.  A wrong tap is reported with the channel halves (accumulator quadrant), the waves whose transform
    rows feed that tap with their (ra, rb, sign), and the wave that folds the element"""
    B, H, W = 9, 128, 128
    assert B * H * W > T.THRESHOLD
    places = _detector_places(H, W, B)
    for c in range(32):  # what the placement covers (a TEST BUG otherwise)
        p, q = places[c], places[c + 32]
        assert (p[3], p[4]) != (q[3], q[4]), "TEST BUG: channels c and c + 32 on the same tap"
        assert ((p[2] % 32) // 2) & 1 != ((q[2] % 32) // 2) & 1, "TEST BUG: channels c and c + 32 in the same block parity"
    assert {(p[3], p[4]) for p in places} == {(a, b) for a in range(3) for b in range(3)}
    assert {(h % 4) // 2 for _, h, *_ in places} == {0, 1}
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
        rows = ", ".join(f"wave {r} (ra, rb, sign) = {ROWS[r]}" for r in FEEDS[ky])
        lines.append(f"dw[o={o}, c={c}, ky={ky}, kx={kx}] = {float(dw[o, c, ky, kx])} want {float(dw_ref[o, c, ky, kx])}: accumulators "
                     f"(ci half {c // 32}, co half {o // 32}), columns xc {FEEDS[kx]}; tap row {ky} is fed by {rows}; folded by wave "
                     f"{(c % 32) // 8}; dY' pixel of o at (b={b}, h={h}, w={w}) = block {blk} (K-step {blk >> 1}, kk {blk & 1}), "
                     f"A lane {c % 32}, B lane {o % 32}")
    assert not bad, f"{len(bad)} wrong taps:\n" + "\n".join(lines)
    X.assert_exact(db, db_ref, "db")


@pytest.mark.parametrize("B,H,W", [(2049, 8, 8), (33, 4, 1000)])
def test_exact_on_edge_tiles_with_affine_and_bias(B, H, W):
    """x in {-1, 0, 1} (3/4 zeros), dY in {-1, 0, 1}, dy_scale + dy_shift (halves) + alpha and the bias gradient: dw and db
    bit-equal to float64 (every tile an edge tile / many tiles per workgroup; the exchange and the bias reduction share LDS)"""
    assert B * H * W > T.THRESHOLD
    x = X.ints((B, 64, H, W), 900 + H, lo=-1, hi=1, zeros=0.75)
    dy = X.ints((B, 64, H, W), 901 + W, lo=-1, hi=1)
    sc, sh = X.scales((B, 64), 902), X.ints((B, 64), 903) / 2
    dw_ref, db_ref = T.exact_ref(x, dy, sc, sh, X.ALPHA)
    dw, db = T.run(T.dev4(x), T.dev4(dy), B, H, W, alpha=X.ALPHA, dy_scale=sc.to(DEV), dy_shift=sh.to(DEV))
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    X.assert_exact(dw, dw_ref, "affine dw")
    X.assert_exact(db, db_ref, "affine db")


def test_exact_on_a_multi_pair_grid():
    """64 -> 256 at 9 x 128^2: four chunk pairs per K-slice go through the exchange, one of them with the bias sums"""
    B, H, W, cout = 9, 128, 128, 256
    x = X.ints((B, 64, H, W), 910, lo=-1, hi=1, zeros=0.75)
    dy = X.ints((B, cout, H, W), 911, lo=-1, hi=1)
    dw_ref, db_ref = T.exact_ref(x, dy)
    dw, db = T.run(T.dev4(x), T.dev4(dy), B, H, W, cout=cout)
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    X.assert_exact(dw, dw_ref, "dw")
    X.assert_exact(db, db_ref, "db")


def test_two_launches_give_the_same_bits():
    B, H, W = 9, 128, 128
    x, dy = T.dev4(T.rnd(B, 64, H, W, seed=920)), T.dev4(T.rnd(B, 64, H, W, seed=921))
    kw = dict(dy_scale=(T.rnd(B, 64, seed=922).abs() + 0.5).to(DEV), dy_shift=T.rnd(B, 64, seed=923).to(DEV), alpha=0.7)
    dw, db = T.run(x, dy, B, H, W, **kw)
    dw2, db2 = T.run(x, dy, B, H, W, **kw)
    assert not torch.isnan(dw).any() and not torch.isnan(db).any()
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "two runs differ"
    dw_d, _ = T.run(x, dy, B, H, W, switches=T.DIRECT, **kw)
    assert not torch.equal(dw, dw_d), "the Winograd form did not engage"
