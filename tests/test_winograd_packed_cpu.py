"""The packed adds (v_pk_add_f32, two floats per instruction) of the Winograd transforms in wgrad3x3_c64_w4_kernel and
conv3x3_c64_w4_kernel, restated in numpy float32.  The modifiers (op_sel, op_sel_hi, neg_lo, neg_hi) are read from the
helpers' own assembly strings in csrc/, so a changed modifier changes what is checked here.  Every value must be the scalar
formula's, bit for bit; the weight gradient holds column 2 of V and of M negated, which may differ from the negated scalar
value in the sign of a zero only, and neither a product nor an accumulated sum can tell."""
import os
import re

import numpy as np

from test_winograd_wgrad_inreg_cpu import lane_transform

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "super-resolution-meta-attention-networks_amd", "csrc")
N = 100_000
F = np.float32


def helpers():
    """name -> (operand numbers of the two sources, modifier dict) of every f32x2 helper built on v_pk_add_f32"""
    found = {}
    for name in ("sisr_common.h", "wgrad3x3_mfma.hip"):
        text = open(os.path.join(CSRC, name)).read()
        for m in re.finditer(r"f32x2 (\w+)\(f32x2 a(?:, f32x2 b)?\) \{[^}]*?asm volatile\(\"v_pk_add_f32 %0, %(\d), %(\d)([^\"]*)\"", text):
            mods = {k: (int(a), int(b)) for k, a, b in re.findall(r"(\w+):\[(\d),(\d)\]", m[4])}
            found[m[1]] = ((int(m[2]), int(m[3])), mods)
    return found


HELPERS = helpers()


def pk(name, a, b=None):
    """the instruction on arrays (..., 2) = (lo, hi): per source, op_sel picks the half that feeds the low add and
    op_sel_hi the half that feeds the high add (default: lo, hi), neg_lo / neg_hi negate what feeds the low / high add"""
    (i0, i1), mods = HELPERS[name]
    src = {1: a, 2: b}
    s = (src[i0], src[i1])
    sel, selh = mods.get("op_sel", (0, 0)), mods.get("op_sel_hi", (1, 1))
    nlo, nhi = mods.get("neg_lo", (0, 0)), mods.get("neg_hi", (0, 0))
    lo = [(-s[k][..., sel[k]] if nlo[k] else s[k][..., sel[k]]) for k in range(2)]
    hi = [(-s[k][..., selh[k]] if nhi[k] else s[k][..., selh[k]]) for k in range(2)]
    out = np.stack([lo[0] + lo[1], hi[0] + hi[1]], axis=-1)
    assert out.dtype == F
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}"


def patches(seed, shape):
    """random normal float32 values, a quarter of the patches with entries from {-1, 0, -0, 1, 2} (equal neighbours: sums and
    differences that are exact zeros of either sign) and some with a few zeros among random values"""
    g = np.random.default_rng(seed)
    x = g.standard_normal((N,) + shape).astype(F)
    small = np.array([-1.0, 0.0, -0.0, 1.0, 2.0], F)
    x[: N // 4] = small[g.integers(0, 5, (N // 4,) + shape)]
    mixed = x[N // 4: N // 2]
    mixed[g.random(mixed.shape) < 0.3] = 0.0
    return x


def test_the_helpers_are_found_with_their_modifiers():
    assert set(HELPERS) == {"sisr_pk_add", "sisr_pk_sub", "pk_add_nl", "pk_hh_sub", "pk_h_pm_l"}
    assert HELPERS["sisr_pk_add"] == ((1, 2), {})
    assert HELPERS["pk_h_pm_l"][0] == (1, 1)


def scalar_reference(d, y):
    """lane_transform (the scalar adds, tests/test_winograd_wgrad_inreg_cpu.py) on all patches at once"""
    V, M = np.empty((N, 4, 4), F), np.empty((N, 4, 4), F)
    rr = np.stack([d[:, 0] - d[:, 2], d[:, 1] + d[:, 2], d[:, 2] - d[:, 1], d[:, 1] - d[:, 3]], axis=1)
    V[:, :, 0], V[:, :, 1] = rr[:, :, 0] - rr[:, :, 2], rr[:, :, 1] + rr[:, :, 2]
    V[:, :, 2], V[:, :, 3] = rr[:, :, 2] - rr[:, :, 1], rr[:, :, 1] - rr[:, :, 3]
    ry = np.stack([y[:, 0], y[:, 0] + y[:, 1], y[:, 0] - y[:, 1], y[:, 1]], axis=1)
    M[:, :, 0], M[:, :, 1], M[:, :, 2], M[:, :, 3] = ry[:, :, 0], ry[:, :, 0] + ry[:, :, 1], ry[:, :, 0] - ry[:, :, 1], ry[:, :, 1]
    for n in (0, N // 4 + 1, N - 1):  # and that restatement against the per-lane original
        v1, m1 = lane_transform(d[n], y[n])
        assert np.array_equal(bits(v1), bits(V[n])) and np.array_equal(bits(m1), bits(M[n]))
    return V, M


def packed_wgrad(d, y):
    """the kernel's transform_op steps 0 .. 21 -> (V, M) with column 2 of both negated, [patch][xr][xc]"""
    dp = d.reshape(N, 4, 2, 2)  # [row][pair c][half]: pair c = columns (2c, 2c + 1)
    rr = np.empty((N, 4, 2, 2), F)
    for c in range(2):
        rr[:, 0, c] = pk("sisr_pk_sub", dp[:, 0, c], dp[:, 2, c])
        rr[:, 1, c] = pk("sisr_pk_add", dp[:, 1, c], dp[:, 2, c])
        rr[:, 2, c] = pk("sisr_pk_sub", dp[:, 2, c], dp[:, 1, c])
        rr[:, 3, c] = pk("sisr_pk_sub", dp[:, 1, c], dp[:, 3, c])
    V, M = np.empty((N, 4, 4), F), np.empty((N, 4, 4), F)
    for xr in range(4):
        V[:, xr, 0:2] = pk("pk_add_nl", rr[:, xr, 0], rr[:, xr, 1])  # va = (V0, V1)
        V[:, xr, 2:4] = pk("pk_hh_sub", rr[:, xr, 0], rr[:, xr, 1])  # vb = (-V2, V3)
    ry = np.stack([y[:, 0], pk("sisr_pk_add", y[:, 0], y[:, 1]), pk("sisr_pk_sub", y[:, 0], y[:, 1]), y[:, 1]], axis=1)
    for xr in range(4):
        mc = pk("pk_h_pm_l", ry[:, xr])  # (M1, -M2)
        M[:, xr, 0], M[:, xr, 1], M[:, xr, 2], M[:, xr, 3] = ry[:, xr, 0], mc[:, 0], mc[:, 1], ry[:, xr, 1]
    return V, M


def test_weight_gradient_transform_packed_equals_scalar():
    d, y = patches(81, (4, 4)), patches(82, (2, 2))
    V, M = scalar_reference(d, y)
    Vp, Mp = packed_wgrad(d, y)
    keep = [0, 1, 3]
    same_bits(Vp[:, :, keep], V[:, :, keep], "V columns 0, 1, 3")
    same_bits(Mp[:, :, keep], M[:, :, keep], "M columns 0, 1, 3")
    for got, want, what in ((Vp[:, :, 2], V[:, :, 2], "V"), (Mp[:, :, 2], M[:, :, 2], "M")):
        nz = want != 0
        assert (~nz).sum() > 1000, "TEST BUG: no exact zeros among the column-2 values"
        same_bits(got[nz], (-want)[nz], f"negated column 2 of {what}, non-zero values")
        assert np.all(got[~nz] == 0), f"column 2 of {what}: a zero became non-zero"
    # products: what the MFMA multiplies.  Equal as numbers everywhere, equal bits wherever neither factor is zero
    P, Pp = V * M, Vp * Mp
    assert np.array_equal(P, Pp)
    both = (V != 0) & (M != 0)
    same_bits(Pp[both], P[both], "products of non-zero factors")
    assert np.any(np.signbit(P) != np.signbit(Pp)), "TEST BUG: no product differs in the sign of zero; the case is not exercised"
    # sums: an accumulator starts at +0 and adds 32 products in order; it never holds -0, so the sign of a zero term is lost
    acc, accp = np.zeros((N // 32, 4, 4), F), np.zeros((N // 32, 4, 4), F)
    for k in range(32):
        acc, accp = acc + P[k::32][: N // 32], accp + Pp[k::32][: N // 32]
    same_bits(accp, acc, "accumulated sums")


def pk4(name, a, b):
    """sisr_pk4_add / sisr_pk4_sub: the f32x4 operation as two packed ones on (.xy, .zw)"""
    return np.concatenate([pk(name, a[..., 0:2], b[..., 0:2]), pk(name, a[..., 2:4], b[..., 2:4])], axis=-1)


def test_conv_rows_columns_fold_and_bias_packed_equal_scalar():
    """rows_half, cols_step, the per-row fold of A^T M A and the epilogue's bias add: f32x4 values over the four ci (or
    tiles) of a register quad, same operands and order, so every result has the scalar form's bits, zeros included"""
    add, sub = (lambda a, b: pk4("sisr_pk_add", a, b)), (lambda a, b: pk4("sisr_pk_sub", a, b))
    d = patches(91, (4, 4, 4))  # [halo row][column][e]
    for xr, (ra, rb) in enumerate(((0, 2), (2, 1), (2, 1), (3, 1))):
        da, db = d[:, ra], d[:, rb]
        want = da - db if xr in (0, 2) else (db + da if xr == 1 else db - da)
        got = sub(da, db) if xr in (0, 2) else (add(db, da) if xr == 1 else sub(db, da))
        same_bits(got, want, f"rows, xr = {xr}")
        rr = want
        same_bits(sub(rr[:, 0], rr[:, 2]), rr[:, 0] - rr[:, 2], "column 0")
        same_bits(add(rr[:, 1], rr[:, 2]), rr[:, 1] + rr[:, 2], "column 1")
        same_bits(sub(rr[:, 2], rr[:, 1]), rr[:, 2] - rr[:, 1], "column 2")
        same_bits(sub(rr[:, 1], rr[:, 3]), rr[:, 1] - rr[:, 3], "column 3")
    acc = patches(92, (4, 4, 4))  # [xr][xc][reg]
    y0, y1 = np.empty((2, N, 2, 4), F), np.empty((2, N, 2, 4), F)  # [scalar | packed][patch][out col j][reg]
    for xr in range(4):
        a = acc[:, xr]
        t = [np.stack([a[:, 0] + a[:, 1] + a[:, 2], a[:, 1] - a[:, 2] - a[:, 3]], axis=1),
             np.stack([add(add(a[:, 0], a[:, 1]), a[:, 2]), sub(sub(a[:, 1], a[:, 2]), a[:, 3])], axis=1)]
        same_bits(t[1], t[0], f"fold terms, xr = {xr}")
        if xr == 0:
            y0[0], y0[1] = t[0], t[1]
        if xr in (1, 2):
            y0[0], y0[1] = y0[0] + t[0], add(y0[1], t[1])
        if xr == 1:
            y1[0], y1[1] = t[0], t[1]
        if xr >= 2:
            y1[0], y1[1] = y1[0] - t[0], sub(y1[1], t[1])
    same_bits(y0[1], y0[0], "output row 0")
    same_bits(y1[1], y1[0], "output row 1")
    bias = np.broadcast_to(patches(93, (1, 1))[:, :, :1], y0[0].shape).astype(F)
    same_bits(add(y0[1], bias), y0[0] + bias, "bias add")
