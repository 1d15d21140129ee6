"""The lane -> LDS map of the in-register K loop of wgrad3x3_c64_w4_kernel (csrc/wgrad3x3_mfma.hip), restated on the CPU:
K-step ks, lane (i = lane & 31, kk = lane >> 5) of wave (ci half cih, co half coh) reads the raw 4 x 4 patch / 2 x 2 dY'
block of block 2 ks + kk; it must address what the former chunk builder read for that block, produce every (block, channel,
transform point) once per wave pair, hit 32 distinct banks per 32-lane half, and add in the chunk builder's order."""
import itertools

import numpy as np

from test_winograd_wgrad_cpu import AS, BT

WH_W, WT_W, W4_HH, W4_TH = 34, 32, 6, 4   # halo / tile width, halo / tile rows of the staged raw image
W4G_X = W4_HH * WH_W * 64                 # floats of the x halo; dY' follows it


def x_index(ks, kk, i, cih, r, j):
    vbr, vbc = ks >> 3, 2 * (ks & 7) + kk
    return ((2 * vbr + r) * WH_W + 2 * vbc + j) * 64 + cih * 32 + i


def y_index(ks, kk, i, coh, r, j):
    vbr, vbc = ks >> 3, 2 * (ks & 7) + kk
    return W4G_X + ((2 * vbr + r) * WT_W + 2 * vbc + j) * 64 + coh * 32 + i


def builder_x_index(vb, ch, r, j):
    """the chunk builder of the LDS form: block vb = (row vb >> 4, column vb & 15), channel ch"""
    return ((2 * (vb >> 4) + r) * WH_W + 2 * (vb & 15) + j) * 64 + ch


def builder_y_index(vb, ch, r, j):
    return W4G_X + ((2 * (vb >> 4) + r) * WT_W + 2 * (vb & 15) + j) * 64 + ch


LANES = list(itertools.product(range(16), range(2), range(32), range(2)))  # ks, kk, i, channel half


def test_every_step_and_lane_reads_its_blocks_patch():
    for ks, kk, i, half in LANES:
        vb, ch = 2 * ks + kk, half * 32 + i
        for r, j in itertools.product(range(4), range(4)):
            a = x_index(ks, kk, i, half, r, j)
            assert a == builder_x_index(vb, ch, r, j) and 0 <= a < W4G_X
        for r, j in itertools.product(range(2), range(2)):
            a = y_index(ks, kk, i, half, r, j)
            assert a == builder_y_index(vb, ch, r, j) and W4G_X <= a < W4G_X + W4_TH * WT_W * 64


def test_every_block_channel_and_point_once_per_wave_pair():
    """a lane's 16 V (M) values are the 16 transform points of its (block, channel); over the 16 K-steps the two waves that
    share a ci (co) half each produce all 32 blocks x 32 channels of that half once"""
    for half in range(2):
        seen = {}
        for ks, kk, i in itertools.product(range(16), range(2), range(32)):
            key = (2 * ks + kk, half * 32 + i)
            seen[key] = seen.get(key, 0) + 1
        assert len(seen) == 32 * 32 and set(seen.values()) == {1}
    assert {(2 * ks + kk, half * 32 + i) for ks, kk, i, half in LANES} == set(itertools.product(range(32), range(64)))


def test_no_read_of_the_loop_has_a_bank_conflict():
    """ds_read_b32 / ds_read2st64_b32: bank (byte address / 4) % 32, conflicts only within a 32-lane half (one kk)"""
    for ks, kk, half in itertools.product(range(16), range(2), range(2)):
        for r, j in itertools.product(range(4), range(4)):
            assert len({x_index(ks, kk, i, half, r, j) % 32 for i in range(32)}) == 32
        for r, j in itertools.product(range(2), range(2)):
            assert len({y_index(ks, kk, i, half, r, j) % 32 for i in range(32)}) == 32


def lane_transform(d, y):
    """the K loop's adds on one lane's raw values, float32: rows first, then columns"""
    f = np.float32
    rr = np.empty((4, 4), f)
    for j in range(4):
        rr[0, j], rr[1, j], rr[2, j], rr[3, j] = d[0, j] - d[2, j], d[1, j] + d[2, j], d[2, j] - d[1, j], d[1, j] - d[3, j]
    V = np.empty((4, 4), f)
    for xr in range(4):
        V[xr] = rr[xr, 0] - rr[xr, 2], rr[xr, 1] + rr[xr, 2], rr[xr, 2] - rr[xr, 1], rr[xr, 1] - rr[xr, 3]
    ry = np.empty((4, 2), f)
    for j in range(2):
        ry[0, j], ry[1, j], ry[2, j], ry[3, j] = y[0, j], y[0, j] + y[1, j], y[0, j] - y[1, j], y[1, j]
    M = np.empty((4, 4), f)
    for xr in range(4):
        M[xr] = ry[xr, 0], ry[xr, 0] + ry[xr, 1], ry[xr, 0] - ry[xr, 1], ry[xr, 1]
    return V, M


def test_add_order_reproduces_the_transform_matrices_in_float32():
    """every row of B^T and of A (last row negated) has at most two non-zero entries, +-1: applied in float32, rows first and
    then columns, each entry of V = B^T d B and M = A dY' A^T is one rounding per stage -- the lane's adds must give the
    same float32 values (compared as numbers: +0 == -0)"""
    g = np.random.default_rng(77)
    bt, a_s = BT.astype(np.float32), AS.astype(np.float32)
    for _ in range(200):
        d, y = g.standard_normal((4, 4)).astype(np.float32), g.standard_normal((2, 2)).astype(np.float32)
        rows_v = np.array([[sum(np.float32(bt[r, k] * d[k, j]) for k in range(4) if bt[r, k]) for j in range(4)] for r in range(4)], np.float32)
        want_v = np.array([[sum(np.float32(rows_v[r, l] * bt[s, l]) for l in range(4) if bt[s, l]) for s in range(4)] for r in range(4)], np.float32)
        rows_m = np.array([[sum(np.float32(a_s[r, k] * y[k, j]) for k in range(2) if a_s[r, k]) for j in range(2)] for r in range(4)], np.float32)
        want_m = np.array([[sum(np.float32(rows_m[r, l] * a_s[s, l]) for l in range(2) if a_s[s, l]) for s in range(4)] for r in range(4)], np.float32)
        V, M = lane_transform(d, y)
        assert V.dtype == np.float32 and np.array_equal(V, want_v) and np.array_equal(M, want_m)
        # and the float64 matrices of test_winograd_wgrad_cpu.py, to float32 rounding of the two stages
        np.testing.assert_allclose(V, BT @ d.astype(np.float64) @ BT.T, rtol=0, atol=4 * 2.0 ** -23 * np.abs(d).sum())
        np.testing.assert_allclose(M, AS @ y.astype(np.float64) @ AS.T, rtol=0, atol=4 * 2.0 ** -23 * np.abs(y).sum())
