"""The one-transform-row-per-wave map of wgrad3x3_c64_w4_kernel (csrc/wgrad3x3_mfma.hip), restated in numpy on integer data.
Wave xr owns the four transform points xi = 4 xr + xc for all 64 ci x 64 co: per K-step ks lane (i = lane & 31, kk = lane >> 5)
reads the two raw patch rows (ra, rb) and the dY' rows (ya, yb) that row xr of B^T d and of A dY' needs, for the channels i
and 32 + i of block 2 ks + kk, forms d_ra + s d_rb and y_ya + s y_yb (s = +-1 in a register, v_pk_fma_f32; a wave whose row
of A has one entry reads yb from an area of +0), then the column steps, and issues 16 MFMAs on the accumulators
t = (xc, ci half, co half).  After the last tile the waves exchange a quadrant at a time through LDS and wave w folds the
registers [4 w, 4 w + 4) of every element."""
import itertools
import os
import re
from fractions import Fraction

import numpy as np

from test_winograd_wgrad_cpu import AS, BT
from test_winograd_wgrad_inreg_cpu import W4G_X, W4_HH, W4_TH, WH_W, WT_W

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "super-resolution-meta-attention-networks_amd", "csrc",
                   "wgrad3x3_mfma.hip")
W4G_Y = W4_TH * WT_W * 64
W4G_Z = int(re.search(r"#define W4G_Z (\d+)", open(SRC).read())[1])  # floats of +0 behind the staged image
ZERO = W4G_X + W4G_Y

# wave xr: raw patch rows (ra, rb) and sign of B^T's row xr; dY' rows (ya, yb) of A's row xr (yb None: the zero area)
ROWS = [(0, 2, -1), (1, 2, +1), (2, 1, -1), (1, 3, -1)]
YROWS = [(0, None), (0, 1), (0, 1), (1, None)]


def x_base(xr, which, ks, kk, i, ch, c):
    """first float of the ds_read2st64_b32 (the second is 64 floats on) of column pair c, row ra (which = 0) or rb (1)"""
    row = ROWS[xr][which]
    return ((2 * (ks >> 3) + row) * WH_W + 4 * (ks & 7) + 2 * kk + 2 * c) * 64 + 32 * ch + i


def y_base(xr, which, ks, kk, i, ch):
    row = YROWS[xr][which]
    off = ((2 * (ks >> 3)) * WT_W + 4 * (ks & 7) + 2 * kk) * 64 + 32 * ch + i
    return ZERO + off if row is None else W4G_X + row * WT_W * 64 + off


def lane_operands(lds, xr, ks, kk, i):
    """the 12 packed instructions of a K-step on integers: V[ch][xc], M[ch][xc] with column 2 of both negated"""
    s = ROWS[xr][2]
    V, M = np.empty((2, 4), np.int64), np.empty((2, 4), np.int64)
    for ch in range(2):
        rr = []
        for c in range(2):
            a, b = x_base(xr, 0, ks, kk, i, ch, c), x_base(xr, 1, ks, kk, i, ch, c)
            rr.append((lds[a] + s * lds[b], lds[a + 64] + s * lds[b + 64]))           # k 0 .. 3: fma(s, d_rb, d_ra)
        V[ch] = (rr[0][0] - rr[1][0], rr[0][1] + rr[1][0],                              # va = pk_add_nl
                 rr[0][1] - rr[1][0], rr[0][1] - rr[1][1])                              # vb = pk_hh_sub: (-V2, V3)
        a, b = y_base(xr, 0, ks, kk, i, ch), y_base(xr, 1, ks, kk, i, ch)
        ry = (lds[a] + s * lds[b], lds[a + 64] + s * lds[b + 64])                       # k 8 .. 9
        M[ch] = ry[0], ry[1] + ry[0], ry[1] - ry[0], ry[1]                              # mc = pk_h_pm_l: (M1, -M2)
    return V, M


def staged_image(seed):
    g = np.random.default_rng(seed)
    x = g.integers(-9, 10, (W4_HH, WH_W, 64))
    y = g.integers(-9, 10, (W4_TH, WT_W, 64))
    lds = np.concatenate([x.ravel(), y.ravel(), np.zeros(W4G_Z, np.int64)])
    return x, y, lds


def transforms(x, y):
    """V[xi][block][ci], M[xi][block][co] of the 32 blocks of a tile, today's sign conventions (column 2 negated in both)"""
    V, M = np.empty((16, 32, 64), np.int64), np.empty((16, 32, 64), np.int64)
    bt, a_s = BT.astype(np.int64), AS.astype(np.int64)
    neg = np.array([1, 1, -1, 1])
    for blk in range(32):
        br, bc = blk >> 4, blk & 15
        d = x[2 * br:2 * br + 4, 2 * bc:2 * bc + 4]    # [row][column][channel]
        yy = y[2 * br:2 * br + 2, 2 * bc:2 * bc + 2]
        V[:, blk] = (np.einsum("rk,klc,sl->rsc", bt, d, bt) * neg[None, :, None]).reshape(16, 64)
        M[:, blk] = (np.einsum("rk,klc,sl->rsc", a_s, yy, a_s) * neg[None, :, None]).reshape(16, 64)
    return V, M


def test_every_operand_is_its_entry_of_the_transforms():
    x, y, lds = staged_image(5)
    V, M = transforms(x, y)
    for xr, ks, kk, i in itertools.product(range(4), range(16), range(2), range(32)):
        v, m = lane_operands(lds, xr, ks, kk, i)
        blk = 2 * ks + kk
        for ch, xc in itertools.product(range(2), range(4)):
            assert v[ch, xc] == V[4 * xr + xc, blk, 32 * ch + i], ("V", xr, ks, kk, i, ch, xc, ROWS[xr])
            assert m[ch, xc] == M[4 * xr + xc, blk, 32 * ch + i], ("M", xr, ks, kk, i, ch, xc, YROWS[xr])


def test_every_point_and_channel_pair_is_accumulated_once_in_k_order():
    """v_mfma_f32_32x32x2_f32: D[m][n] += sum_k A[m][k] B[k][n], lane (i, kk) supplies A[i][kk] and B[kk][i].  Accumulator
    t = (xc, cih, coh) of wave xr takes A = V[cih][xc], B = M[coh][xc]: it holds (xi = 4 xr + xc, ci = 32 cih + m,
    co = 32 coh + n), and its K sequence is ks ascending with block 2 ks + kk in slot kk"""
    x, y, lds = staged_image(6)
    V, M = transforms(x, y)
    want = np.einsum("xbc,xbo->xco", V, M)
    owner = {}
    for xr in range(4):
        ops = {(ks, kk, i): lane_operands(lds, xr, ks, kk, i) for ks, kk, i in itertools.product(range(16), range(2), range(32))}
        for t in range(16):
            xc, cih, coh = t >> 2, (t >> 1) & 1, t & 1
            acc, order = np.zeros((32, 32), np.int64), []
            for ks in range(16):
                A = np.array([[ops[ks, kk, i][0][cih, xc] for kk in range(2)] for i in range(32)])
                Bm = np.array([[ops[ks, kk, i][1][coh, xc] for i in range(32)] for kk in range(2)])
                acc += A @ Bm
                order += [2 * ks, 2 * ks + 1]
            assert order == list(range(32))
            xi = 4 * xr + xc
            assert np.array_equal(acc, want[xi, 32 * cih:32 * cih + 32, 32 * coh:32 * coh + 32]), (xr, t)
            for m, n in itertools.product(range(32), range(32)):
                key = (xi, 32 * cih + m, 32 * coh + n)
                assert key not in owner
                owner[key] = (xr, t)
    assert len(owner) == 16 * 64 * 64


def test_every_read_of_the_loop_is_32_consecutive_floats_inside_its_area():
    """per 32-lane half (one kk) both floats of a ds_read2st64_b32 are 32 consecutive addresses: 32 distinct banks; x reads
    stay in the halo image, dY' reads in the dY' image, the reads of the waves with a one-entry row of A in the zero area"""
    zero_reads = 0
    for xr, ks, kk, ch in itertools.product(range(4), range(16), range(2), range(2)):
        reads = [([x_base(xr, w, ks, kk, i, ch, c) for i in range(32)], (0, W4G_X)) for w in range(2) for c in range(2)]
        for w in range(2):
            in_zero = YROWS[xr][w] is None
            zero_reads += in_zero
            reads.append(([y_base(xr, w, ks, kk, i, ch) for i in range(32)], (ZERO, ZERO + W4G_Z) if in_zero else (W4G_X, ZERO)))
        for a, (lo, hi) in reads:
            for second in (0, 64):
                b = [v + second for v in a]
                assert b == list(range(b[0], b[0] + 32)) and lo <= b[0] and b[-1] < hi, (xr, ks, kk, ch, b[0], lo, hi)
    assert zero_reads == 2 * 16 * 2 * 2  # waves 0 and 3 only, one read per channel and step
    assert W4G_X == W4_HH * WH_W * 64 and (W4G_X + W4G_Y + W4G_Z) * 4 <= 160 * 1024


def ex_index(row, xc, rq, lane):
    """first float of the 16 bytes lane `lane` moves for transform point (row, xc), registers [4 rq, 4 rq + 4)"""
    return (((row * 4 + xc) * 4 + rq) * 64 + lane) * 4


def test_exchange_writes_and_reads_every_value_once_without_a_conflict():
    """per quadrant: wave xr writes registers r of its four accumulators (xc) with 16 ds_write_b128, wave w reads the
    registers [4 w, 4 w + 4) of all 16 transform points with 16 ds_read_b128; 16-byte lane stride (every 8 lanes cover the
    32 banks once), 64 KB inside the dead raw image"""
    mem = {}
    for xr, xc, rq in itertools.product(range(4), range(4), range(4)):
        a = [ex_index(xr, xc, rq, lane) for lane in range(64)]
        assert a == list(range(a[0], a[0] + 256, 4))
        for lane, e in itertools.product(range(64), range(4)):
            assert a[lane] + e not in mem
            mem[a[lane] + e] = (xr, xc, 4 * rq + e, lane)  # (transform row, column, register, lane)
    assert sorted(mem) == list(range(16384)) and 16384 <= W4G_X + W4G_Y
    seen = set()
    for w, row, xc in itertools.product(range(4), range(4), range(4)):
        a = [ex_index(row, xc, w, lane) for lane in range(64)]
        assert a == list(range(a[0], a[0] + 256, 4))
        for lane, e in itertools.product(range(64), range(4)):
            assert mem[a[lane] + e] == (row, xc, 4 * w + e, lane)  # the reader's own lane, its registers, every point
            assert a[lane] + e not in seen
            seen.add(a[lane] + e)
    assert len(seen) == 16384


def f32_round(q, sign_if_zero):
    """Fraction -> float32 bits, round to nearest even (one rounding), subnormals included"""
    if q == 0:
        return np.uint32(0x80000000 if sign_if_zero else 0)
    sign, q = q < 0, abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    m = q / Fraction(2) ** (e - 23)  # 24-bit integer mantissa (less below the normal range), to be rounded
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    if n == 1 << 24:
        n, e = 1 << 23, e + 1
    assert e <= 127
    bits = n if n < 1 << 23 else ((e + 127) << 23) | (n - (1 << 23))
    return np.uint32(bits | (0x80000000 if sign else 0))


def fma_bits(s, b, a):
    """IEEE fma(s, b, a) in float32: the exact s b + a, rounded once; an exact zero is -0 only if product and addend both are"""
    prod_neg = bool(np.signbit(s)) != bool(np.signbit(b))
    return f32_round(Fraction(float(s)) * Fraction(float(b)) + Fraction(float(a)), prod_neg and bool(np.signbit(a)))


def test_fma_with_a_unit_multiplier_and_the_add_of_minus_zero_are_the_adds_bit_for_bit():
    f = np.float32
    g = np.random.default_rng(9)
    vals = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 2.0, 0.5, 3.0, 1e-45, -1e-45, 1.1754944e-38, 3.0e38, -3.0e38, 1e-40], f),
                           g.standard_normal(40).astype(f), (g.standard_normal(20) * 1e-3).astype(f)])
    one, mone, pz = f(1.0), f(-1.0), f(0.0)
    bits = lambda v: np.asarray(v, f).view(np.uint32)
    with np.errstate(over="ignore"):
        for a, b in itertools.product(vals, vals):
            if not np.isfinite(a + b) or not np.isfinite(a - b):
                continue
            assert fma_bits(one, b, a) == bits(a + b), (a, b)
            assert fma_bits(mone, b, a) == bits(a - b), (a, b)
    for x in vals:  # a one-entry row of A: x + (-1)(+0) = x + (-0) = x, zeros of either sign included
        assert fma_bits(mone, pz, x) == bits(x) == bits(x + f(-0.0)), x
    # ... and why the multiplier may not be 0 instead: -0 + 0 * y is +0
    assert fma_bits(pz, f(5.0), f(-0.0)) == bits(f(0.0)) != bits(f(-0.0))
