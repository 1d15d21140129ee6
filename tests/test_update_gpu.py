"""The update step's optional parts against float64 (pytest -m gpu): the gradient-norm / clip-coefficient kernels and the
extended Adam pass of csrc/update.hip, optim.FlatAdam with max_norm / weight_decay / ema_decay, the handlers' fused_clip and
averaged_weights(), and train_sisr / eval_sisr with an averaged network.

House style of tests/test_glue_gpu.py: the native entry points are called directly through hip.lib(); references are
tests/_update.py (checked against torch.optim.AdamW, clip_grad_norm_ and swa_utils by tests/test_update_cpu.py); every
buffer starts as NaN, so an element the kernel must write and does not fails, and what it must not touch -- or, for the norm,
must not READ: the stale ranges between segments -- is NaN.  Tiers:

1. Exact (zero tolerance).  Norm: integer gradients in {0, +-1, +-3}; the sum of squares is an exact integer in double, the
   norm its correctly rounded root, the coefficient clip_coef_ref bit for bit, below and above max_norm.  Update: the dyadic
   construction of test_glue_gpu.adam_exact_case with a power-of-two device coefficient, decay_factor = one_minus_decay =
   0.5 and averages on the 2^-6 grid: zero mismatches in p, m, v and e through the grid-stride sizes and the tails.  With
   the additions off the kernel is bitwise sisr_adam_flat on general data.
2. Bounded: |got - ref64| <= c * 2^-24 * mag, c derived next to each test.  Norm on general data: relative error <= 1e-12
   (chain length x 2^-53), coefficient within one fp32 unit.  Largest err / bound ratios measured on an MI355X (the bar
   is 1):
   update kernel (t in {1, 2, 1000}; each addition alone and all together) -- m 0.73, v 0.66, p 0.17, e 0.08;
   average-only kernel -- e 0.65;
   optim.FlatAdam (three steps, 4.2 M floats, all three options) -- m 0.48, v 0.38, p 0.18, e 0.06, and 0.32 for the
   average of the parameter the step skips;
   norm, general data -- largest relative error 1.5e-16.
3. Handlers: fused_clip against clip_grad_norm_ at the project's figure for two arithmetically equivalent trajectories of
   the small VDSR (rtol 1e-5, atol 1e-7), eager and under graph replay; averaged_weights(), 'network_ema' checkpoints and
   eval_sisr(use_ema) at equality.

Each kernel family has a detector: one input element moved in the copy only the kernel sees must change exactly the outputs
it feeds.
"""
import collections
import os
import time

import numpy as np
import pytest
import torch

import _basic as B
import _exact as X
import _gates as G
import _glue as R
import _update as U
import sisr_amd
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
hip = sisr_amd.hip
DEV = "cuda:0"
NAN = float("nan")
ERR_ARG, ERR_ALIGN = -1, -2
RATIOS = {}

ADAM_CAP = 4096 * 256 * 4    # floats one pass of the update kernels' capped grid covers
ADAM_N = [1, 3, 4, 5, 7, 1023, 1024, 1027, ADAM_CAP, ADAM_CAP + 4, ADAM_CAP + 4 * 300 + 3]
SUMSQ_CAP = 1024 * 256 * 4   # ... and of the norm kernel's (1024 partial blocks)
SUMSQ_N = [1, 3, 4, 5, 7, 1023, 1024, 1027, SUMSQ_CAP, SUMSQ_CAP + 4, SUMSQ_CAP + 8, SUMSQ_CAP + 4 * 300 + 3]
OFF = 12  # floats: 48 bytes, a 16-byte boundary that is no 32- or 64-byte one
EXACT_SC = dict(beta2=0.5, omb1=0.5, omb2=0.5, eps=1.0, step_size=0.125)


def lib():
    return hip.lib()


_LIVE = collections.deque(maxlen=64)


def P(t, off=0):
    """device pointer of t (+ off elements), which stays referenced over the next calls"""
    if t is None:
        return None
    _LIVE.append(t)
    return t.data_ptr() + t.element_size() * off


def St():
    return hip.stream()


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def dd(t):
    return t.to(DEV, torch.float64)


def ok(rc, what):
    hip.check(rc, what)


def arena(t, o):
    """t inside a NaN arena at offset o, 8 NaN floats behind it"""
    a = nan(o + t.numel() + 8)
    a[o:o + t.numel()] = t.to(DEV)
    return a


def bits(t):
    return t.contiguous().view(torch.int32)


def bounded(got, ref, mag, c, what):
    r = R.worst_ratio(got, ref, mag, c)
    RATIOS[what] = max(RATIOS.get(what, 0.0), r) if r == r else NAN
    print(f"{what}: max err / bound = {r:.3f} (c = {c})")
    G.assert_bounded(got, ref, mag, c, what)


def word(value):
    """a float in device memory between two NaN floats -> (buffer, pointer to the word)"""
    buf = nan(3)
    buf[1] = value
    return buf, P(buf, 1)


# ============================================================================ 1. the norm and the clip coefficient
def layout(lengths, first=OFF, gap=8):
    """[(offset, n)] of ranges of the given lengths in one arena: each starts on a 16-byte boundary, `gap` (+ the alignment
    rest) floats behind the previous one"""
    segs, o = [], first
    for n in lengths:
        segs.append((o, n))
        o = (o + n + 3) // 4 * 4 + gap
    return segs, o


def norm_launch(ga, segs, max_norm):
    """the partial launches of every range and the final one -> (norm as double, norm as float, coefficient); everything
    around the outputs and behind the partials must still be NaN"""
    L = lib()
    counts = [L.sisr_sumsq_workspace_bytes(n) // 8 for _, n in segs]
    ws, o64, o32 = nan(sum(counts) + 2, dtype=torch.float64), nan(3, dtype=torch.float64), nan(4)
    k = 0
    for (o, n), c in zip(segs, counts):
        assert c == min(max(-(-(n // 4) // 256), 1), 1024)
        ok(L.sisr_sumsq_partial(P(ga, o), n, P(ws, k), St()), "sisr_sumsq_partial")
        k += c
    ok(L.sisr_clip_coef(P(ws), k, max_norm, P(o64, 1), P(o32, 1), P(o32, 2), St()), "sisr_clip_coef")
    torch.cuda.synchronize()
    assert not bool(ws[:k].isnan().any()) and R.untouched(ws[k:], o64[:1], o64[2:], o32[:1], o32[3:])
    return float(o64[1]), float(o32[1]), float(o32[2])


def int_grads(n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    table = torch.tensor([0.0, 1.0, -1.0, 3.0, -3.0], device=DEV)
    return table[torch.randint(0, 5, (n,), generator=gen, device=DEV)]


def norm_arena(pieces, segs, total):
    """the ranges filled with their gradients, NaN (a stale range, which must not be read) everywhere else"""
    ga = nan(total)
    for g, (o, n) in zip(pieces, segs):
        ga[o:o + n] = g
    return ga


def exact_norm_case(lengths, seed, what):
    segs, total = layout(lengths)
    pieces = [int_grads(n, seed + k) for k, n in enumerate(lengths)]
    pieces[0][0] = 3.0  # never an all-zero gradient
    ga = norm_arena(pieces, segs, total)
    s = sum(int((g.double() ** 2).sum().item()) for g in pieces)  # an integer below 2^53: exact
    norm = float(np.sqrt(np.float64(s)))                          # IEEE: the correctly rounded root
    assert U.sumsq_ref(*pieces) == float(s)
    for max_norm in (norm / 3.0, norm * 2.0, 0.1):
        n64, n32, coef = norm_launch(ga, segs, max_norm)
        assert n64 == norm and n32 == R.f32(norm), (what, n64, norm)
        assert coef == U.clip_coef_ref(norm, max_norm), (what, max_norm, coef)
        assert (coef == 1.0) == (max_norm > norm)
        again = norm_launch(ga, segs, max_norm)
        assert again == (n64, n32, coef), "two calls on the same data differ"


@pytest.mark.parametrize("o", [0, OFF])
@pytest.mark.parametrize("n", SUMSQ_N)
def test_norm_exact(n, o):
    """one range: the tail (n & 3), a range of tail only, the last size without striding, the first two with it and a tail
    behind the stride loop; at the arena's start and at a 16-byte-aligned offset inside it"""
    segs, total = layout([n], first=o)
    g = int_grads(n, seed=n + o)
    g[0] = 3.0
    ga = norm_arena([g], segs, total)
    s = int((g.double() ** 2).sum().item())
    norm = float(np.sqrt(np.float64(s)))
    for max_norm in (norm / 3.0, norm * 2.0):
        n64, n32, coef = norm_launch(ga, segs, max_norm)
        assert n64 == norm and n32 == R.f32(norm) and coef == U.clip_coef_ref(norm, max_norm), (n64, norm, coef)
        assert (coef == 1.0) == (max_norm > norm)
        assert norm_launch(ga, segs, max_norm) == (n64, n32, coef)


@pytest.mark.parametrize("lengths", [(1027,), (1027, 5), (7, SUMSQ_CAP + 4 * 3 + 1, 1023)])
def test_norm_exact_over_segments(lengths):
    """one, two and three ranges of unequal length with NaN between them: a single float read outside the ranges would make
    the norm NaN"""
    exact_norm_case(lengths, seed=31, what=f"segments {lengths}")


def general_grads(n, seed):
    """log-uniform over 1e-6 .. 1 with a random sign (on the device)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, device=DEV, generator=gen, dtype=torch.float64) * 6 - 6)
    return (mag * (torch.randint(0, 2, (n,), device=DEV, generator=gen) * 2 - 1)).float()


@pytest.mark.parametrize("lengths", [(n,) for n in SUMSQ_N] + [(1027, 5), (7, SUMSQ_CAP + 4 * 3 + 1, 1023)])
def test_norm_general(lengths):
    """general fp32 data: every product is exact in double and a sum of k non-negative terms carries at most (k - 1) 2^-53
    relative error whatever its order; the longest chain here -- a thread's products (4 per stride), the 8-level tree, the
    final workgroup's partials and tree -- is a few thousand adds at most, far inside 1e-12 (the issue's figure).  The
    float64 reference sums in another order with the same kind of bound.  The coefficient: within one fp32 unit."""
    segs, total = layout(lengths)
    pieces = [general_grads(n, seed=7 + n + k) for k, n in enumerate(lengths)]
    ga = norm_arena(pieces, segs, total)
    norm = U.norm_ref(*pieces)
    for max_norm in (norm / 3.0, norm * 2.0):
        n64, n32, coef = norm_launch(ga, segs, max_norm)
        err = abs(n64 - norm) / norm
        RATIOS["norm rel"] = max(RATIOS.get("norm rel", 0.0), err)
        print(f"norm over {lengths}: relative error {err:.2e}")
        assert err <= 1e-12
        assert n32 == R.f32(n64)
        want = U.clip_coef_ref(norm, max_norm)
        assert abs(coef - want) <= float(np.spacing(np.float32(want))), (coef, want)
        assert norm_launch(ga, segs, max_norm) == (n64, n32, coef), "two calls on the same data differ"


def test_norm_nonfinite():
    """clip_grad_norm_(error_if_nonfinite=False): a NaN gradient gives a NaN norm and a NaN coefficient, an infinite one an
    infinite norm and the coefficient max_norm / inf = 0, as torch computes them"""
    segs, total = layout([1027])
    for bad, check in ((NAN, lambda n, c: n != n and c != c), (float("inf"), lambda n, c: n == float("inf") and c == 0.0)):
        g = int_grads(1027, seed=2)
        g[700] = bad
        n64, _, coef = norm_launch_raw(norm_arena([g], segs, total), segs, 1.0)
        assert check(n64, coef), (bad, n64, coef)


def norm_launch_raw(ga, segs, max_norm):
    L = lib()
    ws, o64, o32 = nan(2048, dtype=torch.float64), nan(1, dtype=torch.float64), nan(2)
    k = 0
    for o, n in segs:
        ok(L.sisr_sumsq_partial(P(ga, o), n, P(ws, k), St()), "sisr_sumsq_partial")
        k += L.sisr_sumsq_workspace_bytes(n) // 8
    ok(L.sisr_clip_coef(P(ws), k, max_norm, P(o64), P(o32), P(o32, 1), St()), "sisr_clip_coef")
    torch.cuda.synchronize()
    return float(o64[0]), float(o32[0]), float(o32[1])


def test_norm_detector():
    """one gradient moved from +-1 to 3 changes the sum of squares by exactly 8: in the vector body, in the tail, beyond the
    first grid stride and in the second range the reported norm is that of the moved data and not the base's"""
    lengths = (SUMSQ_CAP + 4 * 300 + 3, 1027)
    segs, total = layout(lengths)
    pieces = [int_grads(n, seed=11 + k) for k, n in enumerate(lengths)]
    n0 = lengths[0]
    spots = [(0, 5), (0, n0 - 1), (0, SUMSQ_CAP + 4 * 17 + 2), (1, 1026), (1, 40)]
    assert spots[1][1] >= (n0 & ~3) and spots[2][1] < (n0 & ~3)
    for k, i in spots:
        pieces[k][i] = 1.0
    s = sum(int((g.double() ** 2).sum().item()) for g in pieces)
    base = norm_launch(norm_arena(pieces, segs, total), segs, 1.0)[0]
    assert base == float(np.sqrt(np.float64(s)))
    for k, i in spots:
        moved = [g.clone() for g in pieces]
        moved[k][i] = 3.0
        got = norm_launch(norm_arena(moved, segs, total), segs, 1.0)[0]
        assert got == float(np.sqrt(np.float64(s + 8))) != base, (k, i)


# ============================================================================ 2. the update kernel
def upd_launch(p, g, m, v, e, o, n, sc, gdev=None, decay=1.0, omd=0.0):
    return lib().sisr_update_flat(P(p, o), P(g, o), P(m, o), P(v, o), P(e, o), n, sc["beta2"], sc["omb1"], sc["omb2"],
                                  sc["eps"], sc["step_size"], sc["bc2_sqrt"], sc["grad_scale"], gdev, decay, omd, St())


def adam_launch(p, g, m, v, o, n, sc):
    return lib().sisr_adam_flat(P(p, o), P(g, o), P(m, o), P(v, o), n, sc["beta2"], sc["omb1"], sc["omb2"], sc["eps"],
                                sc["step_size"], sc["bc2_sqrt"], sc["grad_scale"], St())


def adam_general(n, seed):
    """g log-uniform over 1e-6 .. 1 with a random sign; m, v from three reference steps from zero, rounded to fp32; the
    average e a little off p (on the device: n goes to 4.2 M)"""
    p = (torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * 0.1).float()
    st = dict(p=p.double(), m=torch.zeros(n, dtype=torch.float64, device=DEV), v=torch.zeros(n, dtype=torch.float64, device=DEV))
    for t in (1, 2, 3):
        st = R.adam_ref(st["p"], general_grads(n, seed + t), st["m"], st["v"],
                        **R.adam_scalars(1e-4, 0.9, 0.999, 1e-8, t, rounded=False))
    e = (p.double() * 0.97 + 1e-3).float()
    return p, general_grads(n, seed + 4), st["m"].float(), st["v"].float(), e


@pytest.mark.parametrize("n", ADAM_N)
def test_update_with_the_additions_off_is_bitwise_adam_flat(n):
    """a null grad_scale_dev, decay_factor = 1 and a null ema: the same bits as sisr_adam_flat in p, m and v on general
    data, through the tails and the grid-stride sizes"""
    p, g, m, v, _ = adam_general(n, seed=n)
    for t, gs in ((1, 1.0), (1000, 0.37)):
        sc = R.adam_scalars(1e-4, 0.9, 0.999, 1e-8, t, grad_scale=gs)
        a = [arena(x, OFF) for x in (p, g, m, v)]
        b = [x.clone() for x in a]
        ok(adam_launch(*a, OFF, n, sc), "sisr_adam_flat")
        ok(upd_launch(*b, None, OFF, n, sc), "sisr_update_flat")
        torch.cuda.synchronize()
        for x, y, name in zip(a, b, "pgmv"):
            assert torch.equal(bits(x), bits(y)), f"{name} differs from sisr_adam_flat (n = {n}, t = {t})"
        assert not bool(b[0][OFF:OFF + n].isnan().any())


def exact_data(n, seed):
    """g0 in {0, +-1, +-3}, m integers in [-4, 4], p and e on the 2^-6 grid in [-1, 1] (on the device)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    g0 = int_grads(n, seed + 1000)
    m = torch.randint(-4, 5, (n,), generator=gen, device=DEV).float()
    p = torch.randint(-64, 65, (n,), generator=gen, device=DEV).float() / 64
    e = torch.randint(-64, 65, (n,), generator=gen, device=DEV).float() / 64
    return g0, m, p, e


def upd_exact_case(g0, m, p, e, bc2, gs, coef, o, what):
    """test_glue_gpu.adam_exact_case with the additions on: the stored gradient is g0 bc2 / (grad_scale coef), coef a power of
    two in device memory, so gg = g0 bc2 again, v' = gg^2 a perfect square and every denominator 1, 2 or 4; the parameter is
    halved (decay_factor = 0.5) before the dyadic update and the average moves half way to the new parameter
    (one_minus_decay = 0.5): every operation stays exact (budget checks).  Two launches on the same buffers, the second
    with -g."""
    n = g0.numel()
    sc = dict(EXACT_SC, bc2_sqrt=bc2, grad_scale=gs)
    g = g0 * (bc2 / (gs * coef))
    v = (g0 * bc2) ** 2
    ref = dict(p=p.double(), m=m.double(), v=v.double(), e=e.double())
    ap, am, av, ae = arena(p, o), arena(m, o), arena(v, o), arena(e, o)
    cbuf, cptr = word(coef)
    for k, sign in enumerate((1.0, -1.0)):
        ag = arena(g * sign, o)
        kw = dict(dev_scale=coef, decay=0.5, omd=0.5)
        mag = U.update_ref(ref["p"], g * sign, ref["m"], ref["v"], ref["e"], **sc, **kw, A=True)
        ref = U.update_ref(ref["p"], g * sign, ref["m"], ref["v"], ref["e"], **sc, **kw)
        for name in "mvpe":
            X.assert_budget(mag[name], X.granule(ref[name]), f"{what} launch {k} {name}")
        ok(upd_launch(ap, ag, am, av, ae, o, n, sc, gdev=cptr, decay=0.5, omd=0.5), "sisr_update_flat")
        for name, a in (("m", am), ("v", av), ("p", ap), ("e", ae)):
            X.assert_exact(a[o:o + n], ref[name], f"{what} launch {k} {name}")
        for a in (ap, ag, am, av, ae):
            assert R.untouched(a[:o], a[o + n:]), f"{what}: written outside [o, o + n)"
        assert torch.equal(ag[o:o + n], g * sign), "the gradient was modified"
        assert R.untouched(cbuf[:1], cbuf[2:]) and float(cbuf[1]) == coef, "the coefficient word was modified"


@pytest.mark.parametrize("o", [0, OFF])
@pytest.mark.parametrize("n", ADAM_N)
def test_update_exact(n, o):
    t0 = time.time()
    g0, m, p, e = exact_data(n, seed=n + o)
    for bc2, gs, coef in ((1.0, 1.0, 0.5), (0.5, 2.0, 0.25), (1.0, 0.5, 4.0)):
        upd_exact_case(g0, m, p, e, bc2, gs, coef, o, f"update n={n} o={o} bc2_sqrt={bc2} grad_scale={gs} coef={coef}")
    torch.cuda.synchronize()
    if n >= ADAM_CAP:
        print(f"update exact, n = {n}, offset {o}: {time.time() - t0:.2f} s for 6 launches and their comparisons")


# Roundings on the path, d = 1 with a device coefficient (0 without), w = 1 with a decay factor other than 1 (tests/
# test_glue_gpu.py derives the d = w = 0 case: m 4, v 6, p 13):
# gg = fl(fl(g grad_scale) coef): 1 + d roundings.
# m' = fl(m + fl(fl(gg - m) omb1)): gg's, the subtraction, the product, the addition, each relative to a value
#   <= |m| + (|gg| + |m|) omb1 -> c = 4 + d.
# v' = fl(fl(v beta2) + fl(fl(gg gg) omb2)): gg enters twice (2 (1 + d)), the two products of the second term (2), v beta2 (1),
#   the addition (1), all terms non-negative -> c = 6 + 2 d of v'.
# den = fl(fl(sqrt(v') / bc2_sqrt) + eps): sqrt halves v's (3 + d) and rounds (1), the division (1), the addition of eps to a
#   non-negative value (1) -> 6 + d.
# p' = fl(fl(p decay) - fl(step fl(m' / den))): the quotient m's (4 + d) + den's (6 + d) + its own (1) = 11 + 2 d; times step
#   (1); the subtraction (1); the decay product (w), relative to |p| decay -> c = 13 + 2 d + w of |p| decay + step A(m') / den.
# e' = fl(e + fl(fl(p' - e) omd)): p' carries c_p 2^-24 A(p') and enters with weight omd (A(e') holds A(p') omd), then the
#   subtraction, the product and the addition (3), each relative to a value <= A(e') -> c = c_p + 3.
# Division and square root are correctly rounded on this target.  The average-only kernel reads an exact p: c = 3.
def c_update(d, w):
    cp = 13 + 2 * d + w
    return dict(m=4 + d, v=6 + 2 * d, p=cp, e=cp + 3)


C_EMA_ONLY = 3
DECAY32, OMD32, COEF32 = R.f32(0.97), R.f32(1 - 0.999), R.f32(0.37)


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("n", [4099, 65543])
def test_update_bounded(n, t):
    """each addition alone and all together, at the grad_scales of the Adam tier"""
    p, g, m, v, e = adam_general(n, seed=n + t)
    cbuf, cptr = word(COEF32)
    cases = [("coef", True, 1.0, False), ("decay", False, DECAY32, False), ("ema", False, 1.0, True), ("all", True, DECAY32, True)]
    for gs in (1.0, 0.37):
        sc = R.adam_scalars(1e-4, 0.9, 0.999, 1e-8, t, grad_scale=gs)
        for what, dev, decay, ema in cases:
            ap, ag, am, av = (arena(x, 4) for x in (p, g, m, v))
            ae = arena(e, 4) if ema else None
            ok(upd_launch(ap, ag, am, av, ae, 4, n, sc, gdev=cptr if dev else None, decay=decay, omd=OMD32 if ema else 0.0),
               "sisr_update_flat")
            kw = dict(dev_scale=COEF32 if dev else None, decay=decay, omd=OMD32 if ema else None)
            args = (dd(p), dd(g), dd(m), dd(v), dd(e) if ema else None)
            ref, mag = U.update_ref(*args, **sc, **kw), U.update_ref(*args, **sc, **kw, A=True)
            c = c_update(int(dev), int(decay != 1.0))
            for name, a in (("m", am), ("v", av), ("p", ap)) + ((("e", ae),) if ema else ()):
                bounded(a[4:4 + n], ref[name], mag[name], c[name], f"update {name}")
                assert R.untouched(a[:4], a[4 + n:])
            assert torch.equal(ag[4:4 + n], g) and R.untouched(ag[:4], ag[4 + n:]), "the gradient was modified"


@pytest.mark.parametrize("n", ADAM_N)
def test_average_only(n):
    """sisr_ema_flat: the average alone moves -- exact on dyadic data (one_minus_decay = 0.5), bounded on general data -- and
    the parameters it reads are bitwise what they were; nothing outside [o, o + n)"""
    _, _, p, e = exact_data(n, seed=n + 3)
    ap, ae = arena(p, OFF), arena(e, OFF)
    keep = ap.clone()
    for k in range(2):
        ref, mag = U.ema_ref(p, ae[OFF:OFF + n], 0.5), U.ema_ref(p, ae[OFF:OFF + n], 0.5, A=True)
        X.assert_budget(mag, X.granule(ref), f"average-only launch {k}")
        ok(lib().sisr_ema_flat(P(ap, OFF), P(ae, OFF), n, 0.5, St()), "sisr_ema_flat")
        X.assert_exact(ae[OFF:OFF + n], ref, f"average-only n={n} launch {k}")
    assert torch.equal(bits(ap), bits(keep)) and R.untouched(ae[:OFF], ae[OFF + n:])
    p, _, _, _, e = adam_general(n, seed=n + 5)
    ap, ae = arena(p, OFF), arena(e, OFF)
    ok(lib().sisr_ema_flat(P(ap, OFF), P(ae, OFF), n, OMD32, St()), "sisr_ema_flat")
    bounded(ae[OFF:OFF + n], U.ema_ref(dd(p), dd(e), OMD32), U.ema_ref(dd(p), dd(e), OMD32, A=True), C_EMA_ONLY, "average-only e")
    assert torch.equal(ap[OFF:OFF + n], p) and R.untouched(ap[:OFF], ap[OFF + n:], ae[:OFF], ae[OFF + n:])


def test_update_refusals():
    """a null p, g, m or v or n <= 0: SISR_ERR_ARG; any array 4 bytes off a 16-byte boundary (the average included), or a
    coefficient pointer off a 4-byte one: SISR_ERR_ALIGN; nothing written"""
    L = lib()
    bufs = [nan(24) for _ in range(5)]
    cbuf, cptr = word(0.5)
    tail = (0.5, 0.5, 0.5, 1.0, 0.125, 1.0, 1.0)

    def call(ptrs, n=8, gdev=cptr):
        return L.sisr_update_flat(*ptrs, n, *tail, gdev, 0.5, 0.5, St())
    for k in range(5):
        if k < 4:  # (a null average is the kernel without one)
            ptrs = [P(b, 4) for b in bufs]
            ptrs[k] = None
            assert call(ptrs) == ERR_ARG
        ptrs = [P(b, 4) for b in bufs]
        ptrs[k] = P(bufs[k], 5)
        assert ptrs[k] % 16 == 4
        assert call(ptrs) == ERR_ALIGN
    for n in (0, -4):
        assert call([P(b, 4) for b in bufs], n=n) == ERR_ARG
    assert call([P(b, 4) for b in bufs], gdev=cptr + 2) == ERR_ALIGN
    for ptrs in ((None, P(bufs[1], 4)), (P(bufs[0], 4), None)):
        assert L.sisr_ema_flat(*ptrs, 8, 0.5, St()) == ERR_ARG
    assert L.sisr_ema_flat(P(bufs[0], 5), P(bufs[1], 4), 8, 0.5, St()) == ERR_ALIGN
    assert L.sisr_ema_flat(P(bufs[0], 4), P(bufs[1], 5), 8, 0.5, St()) == ERR_ALIGN
    assert L.sisr_ema_flat(P(bufs[0], 4), P(bufs[1], 4), 0, 0.5, St()) == ERR_ARG
    torch.cuda.synchronize()
    assert R.untouched(*bufs)


def test_update_detector():
    """g0 moved from 3 to 21 at one element (v' = (9 + 441) / 2 = 225 = 15^2 and the denominator 16: still exact) in the
    vector body, in the tail and beyond the first grid stride: exactly that element of m, v, p and e mismatches; an element of
    the average moved: exactly that element of e, and nothing of p, m or v"""
    n = ADAM_N[-1]
    g0, m, p, e = exact_data(n, seed=5)
    sc = dict(EXACT_SC, bc2_sqrt=1.0, grad_scale=1.0)
    kw = dict(dev_scale=0.5, decay=0.5, omd=0.5)
    cbuf, cptr = word(0.5)
    spots = (5, n - 1, ADAM_CAP + 4 * 17 + 2)
    assert spots[1] >= (n & ~3) and spots[2] < (n & ~3)
    for i in spots:
        g0[i], m[i] = 3.0, 0.0
    v = g0 ** 2
    base = U.update_ref(p, g0 * 2, m, v, e, **sc, **kw)

    def run(gp, ep):
        ap, am, av, ae = arena(p, 0), arena(m, 0), arena(v, 0), arena(ep, 0)
        ok(upd_launch(ap, arena(gp * 2, 0), am, av, ae, 0, n, sc, gdev=cptr, decay=0.5, omd=0.5), "sisr_update_flat")
        return dict(m=am, v=av, p=ap, e=ae)
    for i in spots:
        gp = g0.clone()
        gp[i] = 21.0
        moved = U.update_ref(p, gp * 2, m, v, e, **sc, **kw)
        got = run(gp, e)
        for name in "mvpe":
            want = moved[name] != base[name]
            assert int(want.sum()) == 1 and bool(want[i]), name
            R.expect_detected(X.mismatch(got[name][:n], base[name]), want, f"update {name}, element {i}")
            assert float(got[name][i]) == float(moved[name][i])
        ep = e.clone()
        ep[i] = e[i] + 2.0
        got = run(g0, ep)
        want = torch.zeros(n, dtype=torch.bool, device=DEV)
        want[i] = True
        R.expect_detected(X.mismatch(got["e"][:n], base["e"]), want, f"update e, average element {i}")
        for name in "mvp":
            X.assert_exact(got[name][:n], base[name], f"update {name} under a moved average")


# ============================================================================ 3. optim.FlatAdam
SHAPES = [(2048, 2049), (7,), (3, 5), (1027,), (1,), (64, 3, 3, 3)]


def make_params(shapes, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, device=DEV, generator=gen) * 0.1) for s in shapes]


def set_grads(ps, gen, skip=()):
    for k, p in enumerate(ps):
        if k in skip:
            p.grad = None
            continue
        mag = 10.0 ** (torch.rand(p.shape, device=DEV, generator=gen) * 6 - 6)
        p.grad = mag * (torch.randint(0, 2, p.shape, device=DEV, generator=gen) * 2 - 1)


# The coefficient FlatAdam's update reads may differ from clip_coef_ref by one fp32 unit (asserted below), 2 x 2^-24 relative:
# gg carries 2 more than in c_update(1, 1) -> m 5 + 2, v 8 + 4, den 7 + 2, quotient 7 + 9 + 1, times step, minus, decay:
# p 20, e 23.
C_FLAT = dict(m=7, v=12, p=20, e=23)


def test_flat_adam_with_all_options_above_the_grid_cap():
    """optim.FlatAdam(max_norm, weight_decay, ema_decay) over more than 4 194 304 floats (one 2048 x 2049 tensor and
    odd-sized ones; the fourth without a gradient in step 2): every step matches update_ref driven by clip_coef_ref of the
    float64 norm of that step's live gradients, started from the arenas as they were before it; the stale gradient of the
    skipped parameter stays out of the norm, its p, m, v are untouched and its average still moves by the lerp; the padding
    floats stay zero in all five arenas"""
    t0 = time.time()
    gen = torch.Generator(device=DEV).manual_seed(3)
    ps = make_params(SHAPES, seed=3)
    lr, b1, b2, eps, wd, max_norm, ema = 1e-4, 0.9, 0.999, 1e-8, 0.05, 100.0, 0.999
    opt = sisr_amd.optim.FlatAdam(ps, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, max_norm=max_norm, ema_decay=ema)
    assert opt.total > ADAM_CAP and opt.param_groups[0]["weight_decay"] == wd and opt.param_groups[0]["decoupled_weight_decay"]
    assert torch.equal(opt.flat_e, opt.flat_p) and opt.flat_e.data_ptr() != opt.flat_p.data_ptr()
    pad = torch.ones(opt.total, dtype=torch.bool, device=DEV)
    for p in ps:
        pad[opt.offsets[p]:opt.offsets[p] + p.numel()] = False
    assert int(pad.sum()) == 1 + 1 + 1 + 3
    arenas = lambda: (opt.flat_p, opt.flat_m, opt.flat_v, opt.flat_e)  # noqa: E731
    steps = [0] * len(ps)
    decay, omd = R.f32(1.0 - lr * wd), R.f32(1.0 - ema)
    for step in range(3):
        before = [a.clone() for a in arenas()]
        set_grads(ps, gen, skip=(3,) if step == 1 else ())
        live = [p.grad for p in ps if p.grad is not None]
        for k, p in enumerate(ps):
            steps[k] += p.grad is not None
        opt.step()
        norm = U.norm_ref(*live)
        coef = U.clip_coef_ref(norm, max_norm)
        assert coef < 1.0 and abs(float(opt.grad_norm) - norm) <= 1e-12 * norm and opt.grad_norm.dtype == torch.float64
        assert float(opt.grad_norm32) == R.f32(float(opt.grad_norm))
        assert abs(float(opt.clip_coef) - coef) <= float(np.spacing(np.float32(coef))), (float(opt.clip_coef), coef)
        if step == 1:  # the stale range would have raised the norm
            assert U.norm_ref(*live, opt.grad_views[ps[3]]) > norm * (1 + 1e-9)
        for k, p in enumerate(ps):
            o, n = opt.offsets[p], p.numel()
            got = [a[o:o + n] for a in arenas()]
            was = [a[o:o + n] for a in before]
            if p.grad is None:
                assert all(torch.equal(a, b) for a, b in zip(got[:3], was[:3])), "a skipped parameter was updated"
                assert not torch.equal(got[3], was[3]), "a skipped parameter's average did not move"
                bounded(got[3], U.ema_ref(was[0], was[3], omd), U.ema_ref(was[0], was[3], omd, A=True), C_EMA_ONLY,
                        "FlatAdam e (skipped)")
                continue
            sc = R.adam_scalars(lr, b1, b2, eps, steps[k])
            kw = dict(dev_scale=coef, decay=decay, omd=omd)
            args = (was[0], p.grad.reshape(-1), was[1], was[2], was[3])
            ref, mag = U.update_ref(*args, **sc, **kw), U.update_ref(*args, **sc, **kw, A=True)
            for name, a in (("p", got[0]), ("m", got[1]), ("v", got[2]), ("e", got[3])):
                bounded(a, ref[name], mag[name], C_FLAT[name], f"FlatAdam {name}")
        for a in arenas() + (opt.flat_g,):
            assert bool((a[pad] == 0).all()), "a padding float between parameters is no longer zero"
    assert steps == [3, 3, 3, 2, 3, 3] and float(opt.state_dict()["state"][3]["step"]) == 2.0
    assert all(torch.equal(v, opt._view(opt.flat_e, ps[k])) and v.data_ptr() == opt._view(opt.flat_e, ps[k]).data_ptr()
               for k, v in opt.ema_state().items())
    torch.cuda.synchronize()
    print(f"FlatAdam with all options over {opt.total} floats, three steps and their comparisons: {time.time() - t0:.2f} s")


SMALL = [(64, 64, 3, 3), (64,), (5, 7), (1027,), (3,)]


def three_steps(opt, ps, seed, skip_at=1):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    for step in range(3):
        set_grads(ps, gen, skip=(3,) if step == skip_at else ())
        opt.step()


def test_flat_adam_state_dict_keeps_torchs_schema_and_round_trips():
    opts = dict(lr=1e-3, weight_decay=0.05, max_norm=1.0, ema_decay=0.9)
    ps = make_params(SMALL, seed=1)
    opt = sisr_amd.optim.FlatAdam(ps, **opts)
    three_steps(opt, ps, seed=2)
    sd = opt.state_dict()
    plain = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()
    assert set(sd) == set(plain) and set(sd["param_groups"][0]) == set(plain["param_groups"][0])
    assert sd["param_groups"][0]["weight_decay"] == 0.05 and sd["param_groups"][0]["decoupled_weight_decay"] is True
    assert all(set(st) == {"step", "exp_avg", "exp_avg_sq"} for st in sd["state"].values()) and len(sd["state"]) == len(ps)
    assert float(sd["state"][3]["step"]) == 2.0 and float(sd["state"][0]["step"]) == 3.0
    # a fresh FlatAdam over copies of the parameters: state from the dict, the average handed over separately
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt2 = sisr_amd.optim.FlatAdam(qs, **opts)
    opt2.load_state_dict({"state": {k: {n: (t.clone() if torch.is_tensor(t) else t) for n, t in st.items()}
                                    for k, st in sd["state"].items()}, "param_groups": sd["param_groups"]})
    assert torch.equal(opt2.flat_e, opt2.flat_p), "without an average supplied it restarts from the parameters"
    opt2.load_ema({k: v.clone() for k, v in opt.ema_state().items()})
    for a, b in ((opt.flat_p, opt2.flat_p), (opt.flat_m, opt2.flat_m), (opt.flat_v, opt2.flat_v), (opt.flat_e, opt2.flat_e)):
        assert torch.equal(a, b)
    gen = torch.Generator(device=DEV).manual_seed(9)
    set_grads(ps, gen)
    for p, q in zip(ps, qs):
        q.grad = p.grad.clone()
    opt.step()
    opt2.step()
    for a, b in ((opt.flat_p, opt2.flat_p), (opt.flat_m, opt2.flat_m), (opt.flat_v, opt2.flat_v), (opt.flat_e, opt2.flat_e)):
        assert torch.equal(a, b), "the reloaded optimiser's next step differs"
    assert float(opt.grad_norm) == float(opt2.grad_norm) and float(opt.clip_coef) == float(opt2.clip_coef)
    with pytest.raises(ValueError):
        opt2.load_ema({0: opt.ema_state()[0]})


def test_flat_adam_with_the_options_off_is_the_flat_adam_of_before():
    """weight_decay=0, max_norm=None, ema_decay=None spelled out: bitwise the parameters of a FlatAdam built without the
    arguments after three steps (one parameter skipped in step 2), and the same launches -- sisr_update_flat is never called.
    An average alone (the extended kernel with a null coefficient and decay_factor 1) leaves the trajectory bitwise as well;
    the L2 form of weight decay, amsgrad and maximize are still refused."""
    runs = {}
    for name, kw in (("before", {}), ("off", dict(weight_decay=0.0, max_norm=None, ema_decay=None)), ("ema", dict(ema_decay=0.99))):
        ps = make_params(SMALL, seed=1)
        opt = sisr_amd.optim.FlatAdam(ps, lr=1e-3, **kw)
        called = []
        if name == "off":
            opt._step_with_options = lambda *a, **k: called.append(1)
        three_steps(opt, ps, seed=2)
        assert not called
        runs[name] = (opt.flat_p.clone(), opt.flat_m.clone(), opt.flat_v.clone(), opt)
    for name in ("off", "ema"):
        for a, b in zip(runs["before"][:3], runs[name][:3]):
            assert torch.equal(bits(a), bits(b)), name
    off = runs["off"][3]
    assert off.flat_e is None and off.grad_norm is None and off.clip_coef is None
    assert off.state_dict()["param_groups"][0] == runs["before"][3].state_dict()["param_groups"][0]
    with pytest.raises(RuntimeError, match="no average"):
        off.ema_state()
    for key, value in (("decoupled_weight_decay", False), ("amsgrad", True), ("maximize", True)):
        ps = make_params(SMALL[:2], seed=1)
        opt = sisr_amd.optim.FlatAdam(ps, lr=1e-3, weight_decay=0.01)
        opt.param_groups[0][key] = value
        set_grads(ps, torch.Generator(device=DEV).manual_seed(1))
        with pytest.raises(NotImplementedError):
            opt.step()
    for bad in (dict(max_norm=0.0), dict(max_norm=float("inf")), dict(ema_decay=1.0), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            sisr_amd.optim.FlatAdam(make_params(SMALL[:2], seed=1), **bad)


# ============================================================================ 4. handlers
VDSR = dict(kernel_pattern=[3] * 5, channel_pattern=[1, 64, 64, 64, 64, 1])


def vdsr(save_dir, eval_mode=False, **extra):
    torch.manual_seed(8)
    return sisr_amd.available_models["vdsr"](device=0, model_save_dir=str(save_dir), eval_mode=eval_mode, lr=1e-4, **VDSR, **extra)


def train3(h):
    g = torch.Generator().manual_seed(5)
    for _ in range(3):
        x, y = torch.rand(2, 1, 24, 40, generator=g), torch.rand(2, 1, 24, 40, generator=g)
        h.train_step(x, y)
    return [p.detach().clone() for p in h.net.parameters()]


@pytest.mark.parametrize("grad_clip", [0.1, 0.01])
@pytest.mark.parametrize("graph", [False, True])
def test_fused_clip_follows_clip_grad_norm(tmp_path, monkeypatch, graph, grad_clip):
    """grad_clip = 0.1 (VDSR's default) by clip_grad_norm_ and inside FlatAdam's pass: the two trajectories differ only by
    the rounding of the coefficient; the fused handler never calls clip_grad_norm_.  This small net's gradient norm is about
    0.04, so 0.1 leaves the gradients as they are; at 0.01 every step is clipped (asserted), with the same tolerance."""
    calls = []
    real = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    runs = {}
    for fused in (False, True):
        h = vdsr(tmp_path, grad_clip=grad_clip, fused_clip=fused)
        h.use_graph = graph
        assert h.optimizer.max_norm == (grad_clip if fused else None)
        del calls[:]
        runs[fused] = train3(h)
        assert len(calls) == (0 if fused else 3)
        if fused:
            n, c = float(h.optimizer.grad_norm), float(h.optimizer.clip_coef)
            print(f"fused clip (graph={graph}, grad_clip={grad_clip}): last norm {n:.6g}, coefficient {c:.6g}")
            assert n > 0 and c == U.clip_coef_ref(n, grad_clip) and (c < 1.0) == (grad_clip == 0.01)
    for a, b in zip(runs[False], runs[True]):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)


def test_averaged_weights_checkpoints_and_ema_loading(tmp_path):
    h = vdsr(tmp_path, ema_decay=0.9)
    assert h.has_ema()
    start = h.optimizer.flat_p.clone()
    assert torch.equal(h.optimizer.flat_e, start)
    train3(h)
    opt = h.optimizer
    p_keep, e_keep = opt.flat_p.clone(), opt.flat_e.clone()
    assert not torch.equal(p_keep, e_keep) and not torch.equal(e_keep, start)
    ptrs = [p.data_ptr() for p in h.net.parameters()]
    x = torch.rand(1, 1, 24, 40, generator=torch.Generator().manual_seed(11))
    plain = h.run_eval(x)[0]
    with h.averaged_weights():
        assert torch.equal(opt.flat_p, e_keep) and torch.equal(opt.flat_e, p_keep)
        averaged = h.run_eval(x)[0]
        with pytest.raises(RuntimeError, match="nested"):
            with h.averaged_weights():
                pass
        with pytest.raises(RuntimeError, match="averaged_weights"):
            h.save_model("inside", 0)
    assert torch.equal(bits(opt.flat_p), bits(p_keep)) and torch.equal(bits(opt.flat_e), bits(e_keep)), "not restored bitwise"
    assert ptrs == [p.data_ptr() for p in h.net.parameters()] and not h._averaged
    assert torch.equal(h.run_eval(x)[0], plain) and not torch.equal(averaged, plain)
    # a second handler loaded with the averaged state dict, assembled here from ema_state()
    sd = {k: v.detach().clone() for k, v in h.net.state_dict().items()}
    for (name, _), (_, avg) in zip(h.net.named_parameters(), sorted(opt.ema_state().items())):
        sd[name] = avg.detach().clone()
    h2 = vdsr(tmp_path, eval_mode=True)
    h2.net.load_state_dict(sd)
    assert torch.equal(h2.run_eval(x)[0], averaged)
    # checkpoint: the average travels as 'network_ema'
    h.save_model("avg", 0)
    state = torch.load(os.path.join(str(tmp_path), "avg_0"), weights_only=True)
    assert set(state) == {"network", "network_ema", "optimizer", "model_name", "model_epoch"}
    assert list(state["network_ema"]) == list(state["network"])
    assert all(torch.equal(state["network_ema"][k].cpu(), sd[k].cpu()) for k in sd)
    h3 = vdsr(tmp_path, ema_decay=0.9)
    h3.load_model("avg", 0)
    assert torch.equal(h3.optimizer.flat_p, p_keep) and torch.equal(h3.optimizer.flat_e, e_keep)
    h4 = vdsr(tmp_path, eval_mode=True)
    h4.load_model("avg", 0, ema=True)
    assert torch.equal(h4.run_eval(x)[0], averaged)
    # a checkpoint without the key: ema=True raises naming the file; a training handler starts its average from the weights
    h5 = vdsr(tmp_path)
    assert not h5.has_ema()
    h5.save_model("noavg", 0)
    assert set(torch.load(os.path.join(str(tmp_path), "noavg_0"), weights_only=True)) == {"network", "optimizer", "model_name",
                                                                                         "model_epoch"}
    with pytest.raises(RuntimeError, match="noavg_0"):
        vdsr(tmp_path, eval_mode=True).load_model("noavg", 0, ema=True)
    h6 = vdsr(tmp_path, ema_decay=0.9)
    train3(h6)
    h6.load_model("noavg", 0)
    assert torch.equal(h6.optimizer.flat_e, h6.optimizer.flat_p) and torch.equal(h6.optimizer.flat_p, h5.optimizer.flat_p)
    with pytest.raises(RuntimeError, match="no average"):
        with h5.averaged_weights():
            pass


def test_options_without_a_flat_adam_on_a_hip_handler_name_the_switch(tmp_path, monkeypatch):
    monkeypatch.setenv("SISR_FLAT_ADAM", "0")
    with pytest.raises(RuntimeError, match="SISR_FLAT_ADAM"):
        vdsr(tmp_path, ema_decay=0.9)
    assert type(vdsr(tmp_path).optimizer) is torch.optim.Adam


# ============================================================================ 5. train_sisr and eval_sisr
def test_train_sisr_validates_and_eval_sisr_loads_the_averaged_network(tmp_path):
    """one epoch of the b4 configuration (srcnn on Set5) with ema_decay and fused_clip in internal_params: the checkpoint
    holds 'network_ema', validation ran on the averaged weights, and eval_sisr(use_ema=true) writes '<experiment>@ema' rows
    with the PSNR run_eval gives under averaged_weights() on the same images"""
    from PIL import Image
    cfg = B.b4_config(tmp_path)
    cfg["model"]["internal_params"].update(ema_decay=0.9, fused_clip=True, grad_clip=0.1)
    cfg["training"].update(gpu="single", sp_gpu=0)
    total = sisr_amd.cli.train_sisr(cfg)
    exp = cfg["experiment"]
    assert os.path.isfile(os.path.join(str(tmp_path), exp, "result_outputs", "summary.csv"))
    ckpt = os.path.join(str(tmp_path), exp, "saved_models", "train_model_0")
    state = torch.load(ckpt, weights_only=True)
    assert "network_ema" in state and list(state["network_ema"]) == list(state["network"])
    assert any(not torch.equal(state["network_ema"][k], state["network"][k]) for k in state["network"])
    set5 = os.path.join(GOLDEN, "set5")
    common = dict(model_and_epoch=[[exp, "0"]], model_loc=str(tmp_path), gpu=True, hr_dir=os.path.join(set5, "hr"),
                  lr_dir=os.path.join(set5, "lr_random_blur"), full_directory=True, scale=4, out_loc=str(tmp_path))
    df, avg = sisr_amd.cli.eval_sisr(results_name="ev_ema", use_ema=True, **common)
    assert set(df["Model"]) == {exp + "@ema"} and len(df) == 5 and list(avg["Model"]) == [exp + "@ema"]
    # the same images through a training-mode interface resumed from the checkpoint, under averaged_weights()
    mi = sisr_amd.ModelInterface(str(tmp_path), exp, gpu="single", sp_gpu=0, mode="train", load_epoch=0)
    assert mi.model.has_ema()
    want = {}
    for name in sorted(f for f in os.listdir(os.path.join(set5, "hr")) if f.endswith(".png")):
        lr, hr = (sisr_amd.data.to_tensor(Image.open(os.path.join(set5, d, name)).convert("RGB"))[None]
                  for d in ("lr_random_blur", "hr"))
        x = torch.from_numpy(sisr_amd.metrics.batch_rgb_to_ycbcr(sisr_amd.cli._low_res_prep(lr, 4).numpy()))
        y_proc = sisr_amd.ModelInterface.colorspace_convert(hr, colorspace="rgb")
        with mi.model.averaged_weights():
            _, ycbcr, _, _ = mi.net_run_and_process(lr=x, hr=None)
        want[name] = sisr_amd.metrics.psnr(ycbcr[0, 0], y_proc[0, 0], 1)
    got = dict(zip(df["Image_Name"], df["PSNR"]))
    print(got, want, total["val-PSNR"])
    assert got == want
    # train_sisr's validation ran on the averaged weights too (its images are a Pillow-made folder: the project's 5e-3 dB)
    assert abs(float(avg["PSNR"].iloc[0]) - total["val-PSNR"][-1]) < 5e-3
    plain, _ = sisr_amd.cli.eval_sisr(results_name="ev_plain", **common)
    assert set(plain["Model"]) == {exp} and dict(zip(plain["Image_Name"], plain["PSNR"])) != want
