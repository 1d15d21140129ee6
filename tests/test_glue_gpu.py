"""The small kernels around the convs against float64 (pytest -m gpu): the flat Adam step, the layout and bf16 rounding
kernels (csrc/misc.hip), the SFTMD glue -- weight composition and its split, the SFT combine and its backward, the strided
64-channel maps, the clamp (csrc/sft.hip, without the 9x9 conv, pinned in tests/test_exact_gpu.py) -- and the blur / noise
quantisers (csrc/degrade.hip).

The native entry points are called directly through hip.lib(); ops.sft_layer, optim.FlatAdam and degrade.blur_quant where
a wrapper's rule is under test.  References are tests/_glue.py (checked against PyTorch's float64 autograd, torch.optim.Adam
and the oracle by tests/test_glue_cpu.py).  Every output buffer starts as NaN: an element the kernel must write and does not
fails, and what it must not touch (stride gaps, arena floats outside [o, o + n), the parameters a split has no source for)
has to be NaN afterwards.  Tiers:

1. Exact (zero tolerance): copies and layout maps on distinct values; Adam, the SFT combine, the blur and the noise
   quantiser on dyadic data on which every fp32 operation is exact (tests/_exact.py, a budget check before each); the
   LeakyReLU ops and the noise quantiser on general data against their one-rounding fp32 statement; bf16 rounding bit for
   bit on all 65 536 upper halves x five lower halves.  All report zero mismatches.  The capped grids are run at
   the first sizes at which they stride: 4 194 304 + 4 floats (Adam), 1 048 560 + 37 pixels (SFT combine), 16 776 960
   elements (layout kernels).
2. Bounded: |got - ref64| <= c * 2^-24 * mag, mag the `A=True` form, c derived next to each test from the roundings on the
   path.  Largest err / bound ratios measured on an MI355X (the bar is 1):
   Adam kernel (t in {1, 2, 1000}, grad_scale in {1, 0.37}) -- m 0.77, v 0.71, p 0.17;
   optim.FlatAdam (three steps, 4.2 M floats) -- m 0.66, v 0.47, p 0.30;
   SFT combine -- out 0.21, dx 0.32, dm 0.32 (da is exact).
3. ops.sft_layer at the metadata widths where its two sparsity rules switch (M in {16, 17, 32, 33}) against the four-conv
   formulation in float64, at the project's own figures for this composition (2e-6 forward, 5e-6 on gradients, relative
   L2), the metadata columns of the first convs' weight gradients one by one.

Each family has a detector: one input element moved in the copy only the kernel sees must make the exact comparison
mismatch at exactly the outputs that element feeds.

The mask-consistency test has no float64 value: with a = -fl32(x s) the pre-activation x s + a is rounding residue, and
what is asserted is that the backward kernel's recomputed ReLU mask agrees with the sign the forward kernel stored, element
by element.  Both kernels compute it with one explicit fused multiply-add (sft_pre in csrc/sft.hip).
"""
import collections
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _exact as X
import _gates as G
import _glue as R
import sisr_amd

pytestmark = pytest.mark.gpu
hip = sisr_amd.hip
ops = sisr_amd.ops
DEV = "cuda:0"
NAN = float("nan")
U = 2.0 ** -24
ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -4
C_SIG = 8  # a sigmoid of an exact fp32 argument (expf, 1 + e, 1 / .): tests/test_spar_han_gpu.py, tests/test_gates_gpu.py
RATIOS = {}


def lib():
    return hip.lib()


_LIVE = collections.deque(maxlen=64)


def P(t, off=0):
    """device pointer of t (+ off floats), which stays referenced over the next calls"""
    if t is None:
        return None
    _LIVE.append(t)
    return t.data_ptr() + 4 * off


def St():
    return hip.stream()


def nan(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def dev(t):
    return t.to(DEV, torch.float32).contiguous()


def dd(t):
    return t.to(DEV, torch.float64)


def ok(rc, what):
    hip.check(rc, what)


def strided(t, stride, off=0):
    """t [npix][64] as the chunk at channel `off` of a NaN [npix][stride] buffer"""
    buf = nan(t.shape[0], stride)
    buf[:, off:off + 64] = t.to(DEV)
    return buf


def gaps_untouched(buf, *chunks):
    """everything outside the 64-channel chunks at the given offsets is still NaN"""
    keep = torch.ones(buf.shape[1], dtype=torch.bool, device=buf.device)
    for c in chunks:
        keep[c:c + 64] = False
    return bool(buf[:, keep].isnan().all())


def bounded(got, ref, mag, c, what):
    r = R.worst_ratio(got, ref, mag, c)
    RATIOS[what] = max(RATIOS.get(what, 0.0), r) if r == r else NAN
    print(f"{what}: max err / bound = {r:.3f} (c = {c})")
    G.assert_bounded(got, ref, mag, c, what)


def misaligned(n):
    """(an aligned view, a view 4 bytes past a 16-byte boundary) of n floats each"""
    buf = torch.zeros(n + 8, device=DEV)
    a, b = buf[4:4 + n], buf[1:1 + n]
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 4
    return a, b


# ============================================================================ 1. Adam
ADAM_CAP = 4096 * 256 * 4  # floats one pass of the capped grid covers: the grid-stride loop first runs above it
ADAM_N = [1, 3, 4, 5, 7, 1023, 1024, 1027, ADAM_CAP, ADAM_CAP + 4, ADAM_CAP + 4 * 300 + 3]
ADAM_OFF = 12  # floats: 48 bytes, a 16-byte boundary that is no 32- or 64-byte one
EXACT_SC = dict(beta2=0.5, omb1=0.5, omb2=0.5, eps=1.0, step_size=0.125)


def adam_launch(p, g, m, v, o, n, sc):
    return lib().sisr_adam_flat(P(p, o), P(g, o), P(m, o), P(v, o), n, sc["beta2"], sc["omb1"], sc["omb2"], sc["eps"],
                                sc["step_size"], sc["bc2_sqrt"], sc["grad_scale"], St())


def arena(t, o):
    """t inside a NaN arena at offset o, 8 NaN floats behind it"""
    a = nan(o + t.numel() + 8)
    a[o:o + t.numel()] = t.to(DEV)
    return a


def adam_exact_data(n, seed):
    """g0 in {0, +-1, +-3}, m integers in [-4, 4], p on the 2^-6 grid in [-1, 1] (on the device: n goes to 4.2 M)"""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    table = torch.tensor([0.0, 1.0, -1.0, 3.0, -3.0], device=DEV)
    g0 = table[torch.randint(0, 5, (n,), generator=gen, device=DEV)]
    m = torch.randint(-4, 5, (n,), generator=gen, device=DEV).float()
    p = torch.randint(-64, 65, (n,), generator=gen, device=DEV).float() / 64
    return g0, m, p


def adam_exact_case(g0, m, p, bc2, gs, o, what):
    """With one_minus_beta1 = beta2 = one_minus_beta2 = 0.5, eps = 1, step_size = 2^-3 and the stored gradient
    g = g0 bc2 / grad_scale (a power-of-two multiple of g0): gg = g0 bc2, v = gg^2 on entry so v' = gg^2 is a perfect square,
    sqrt(v') / bc2 = |g0| and every denominator is 1, 2 or 4; m' = m + (gg - m) / 2 and the update are dyadic.  Two launches
    on the same buffers, the second with -g (v' stays gg^2, m' carries over).  Returns the arenas after both."""
    n = g0.numel()
    sc = dict(EXACT_SC, bc2_sqrt=bc2, grad_scale=gs)
    g = g0 * (bc2 / gs)
    v = (g0 * bc2) ** 2
    ref = dict(p=p.double(), m=m.double(), v=v.double())
    ap, am, av = arena(p, o), arena(m, o), arena(v, o)
    for k, sign in enumerate((1.0, -1.0)):
        ag = arena(g * sign, o)
        mag = R.adam_ref(ref["p"], g * sign, ref["m"], ref["v"], **sc, A=True)
        ref = R.adam_ref(ref["p"], g * sign, ref["m"], ref["v"], **sc)
        for name in "mvp":
            X.assert_budget(mag[name], X.granule(ref[name]), f"{what} launch {k} {name}")
        ok(adam_launch(ap, ag, am, av, o, n, sc), "sisr_adam_flat")
        for name, a in (("m", am), ("v", av), ("p", ap)):
            X.assert_exact(a[o:o + n], ref[name], f"{what} launch {k} {name}")
        for a in (ap, ag, am, av):
            assert R.untouched(a[:o], a[o + n:]), f"{what}: written outside [o, o + n)"
        assert torch.equal(ag[o:o + n], g * sign), "the gradient was modified"
    return ap, am, av


@pytest.mark.parametrize("o", [0, ADAM_OFF])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_exact(n, o):
    """the tail (n & 3), a range of tail only, the last size without striding and the first with it, alone and behind the
    stride loop's last float4; at the arena's start and at a 16-byte-aligned offset inside it"""
    t0 = time.time()
    g0, m, p = adam_exact_data(n, seed=n + o)
    for bc2 in (1.0, 0.5):
        for gs in (1.0, 0.5, 2.0):
            adam_exact_case(g0, m, p, bc2, gs, o, f"Adam n={n} o={o} bc2_sqrt={bc2} grad_scale={gs}")
    torch.cuda.synchronize()
    if n >= ADAM_CAP:
        print(f"Adam exact, n = {n}, offset {o}: {time.time() - t0:.2f} s for 12 launches and their comparisons")


def adam_general(n, seed):
    """g log-uniform over 1e-6 .. 1 with a random sign; m, v from three reference steps from zero, rounded to fp32"""
    gen = torch.Generator().manual_seed(seed)

    def grad():
        return (10.0 ** (torch.rand(n, generator=gen, dtype=torch.float64) * 6 - 6) *
                (torch.randint(0, 2, (n,), generator=gen) * 2 - 1)).float()
    p = (torch.randn(n, generator=gen) * 0.1).float()
    st = dict(p=p.double(), m=torch.zeros(n, dtype=torch.float64), v=torch.zeros(n, dtype=torch.float64))
    for t in (1, 2, 3):
        st = R.adam_ref(st["p"], grad(), st["m"], st["v"], **R.adam_scalars(1e-4, 0.9, 0.999, 1e-8, t, rounded=False))
    return p, grad(), st["m"].float(), st["v"].float()


# gg = fl(g grad_scale): one rounding.
# m' = fl(m + fl(fl(gg - m) omb1)): gg's rounding, the subtraction, the product, the addition, each relative to a value
#   <= |m| + (|gg| + |m|) omb1 -> c = 4.
# v' = fl(fl(v beta2) + fl(fl(gg gg) omb2)): gg enters twice (2), the two products of the second term (2), v beta2 (1), the
#   addition (1), all terms non-negative -> c = 6 of v'.
# p' = fl(p - fl(step fl(m' / den))), den = fl(fl(sqrt(v') / bc2_sqrt) + eps): sqrt halves v's 6 (3) and rounds (1), the
#   division by bc2_sqrt (1), the addition of eps to a non-negative value (1) -> den carries 6; the quotient: m's 4 (of its
#   A-form) + den's 6 + its own rounding (1) = 11; times step (1) = 12 of step A(m') / den; the subtraction (1) of |p'| ->
#   c = 13 of |p| + step A(m') / den.  Division and square root are correctly rounded on this target.
C_ADAM = dict(m=4, v=6, p=13)


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("n", [4099, 65543])
def test_adam_bounded(n, t):
    p, g, m, v = adam_general(n, seed=n + t)
    for gs in (1.0, 0.37):
        sc = R.adam_scalars(1e-4, 0.9, 0.999, 1e-8, t, grad_scale=gs)
        ap, ag, am, av = arena(p, 4), arena(g, 4), arena(m, 4), arena(v, 4)
        ok(adam_launch(ap, ag, am, av, 4, n, sc), "sisr_adam_flat")
        ref, mag = R.adam_ref(dd(p), dd(g), dd(m), dd(v), **sc), R.adam_ref(dd(p), dd(g), dd(m), dd(v), **sc, A=True)
        for name, a in (("m", am), ("v", av), ("p", ap)):
            bounded(a[4:4 + n], ref[name], mag[name], C_ADAM[name], f"Adam {name}")
            assert R.untouched(a[:4], a[4 + n:])


def test_adam_refusals():
    """a null pointer or n <= 0: SISR_ERR_ARG; a pointer 4 bytes off a 16-byte boundary: SISR_ERR_ALIGN; nothing written"""
    L = lib()
    bufs = [nan(24) for _ in range(4)]
    sc = dict(EXACT_SC, bc2_sqrt=1.0, grad_scale=1.0)
    tail = (sc["beta2"], sc["omb1"], sc["omb2"], sc["eps"], sc["step_size"], sc["bc2_sqrt"], sc["grad_scale"], St())
    for k in range(4):
        ptrs = [P(b, 4) for b in bufs]
        ptrs[k] = None
        assert L.sisr_adam_flat(*ptrs, 8, *tail) == ERR_ARG
        ptrs = [P(b, 4) for b in bufs]
        ptrs[k] = P(bufs[k], 5)
        assert ptrs[k] % 16 == 4
        assert L.sisr_adam_flat(*ptrs, 8, *tail) == ERR_ALIGN
    for n in (0, -4):
        assert L.sisr_adam_flat(*[P(b, 4) for b in bufs], n, *tail) == ERR_ARG
    assert R.untouched(*bufs)


def test_adam_detector():
    """g0 moved from 3 to 21 at one element (v' = (9 + 441) / 2 = 225 = 15^2 and the denominator 16: still exact) in the
    vector body, in the tail and beyond the first grid stride: exactly that element of m, v and p mismatches"""
    n = ADAM_N[-1]
    g0, m, p = adam_exact_data(n, seed=5)
    sc = dict(EXACT_SC, bc2_sqrt=1.0, grad_scale=1.0)
    spots = (5, n - 1, ADAM_CAP + 4 * 17 + 2)
    assert spots[1] >= (n & ~3) and spots[2] < (n & ~3)
    for i in spots:
        g0[i], m[i] = 3.0, 0.0
    v = g0 ** 2
    base = R.adam_ref(p, g0, m, v, **sc)
    for i in spots:
        gp = g0.clone()
        gp[i] = 21.0
        moved = R.adam_ref(p, gp, m, v, **sc)
        ap, am, av = arena(p, 0), arena(m, 0), arena(v, 0)
        ok(adam_launch(ap, arena(gp, 0), am, av, 0, n, sc), "sisr_adam_flat")
        for name, a in (("m", am), ("v", av), ("p", ap)):
            want = moved[name] != base[name]
            assert int(want.sum()) == 1 and bool(want[i])
            R.expect_detected(X.mismatch(a[:n], base[name]), want, f"Adam {name}, element {i}")
            assert float(a[i]) == float(moved[name][i])


def test_flat_adam_above_the_grid_cap():
    """optim.FlatAdam over more than 4 194 304 floats (one 2048 x 2049 tensor and odd-sized ones; the fourth without a
    gradient in step 2): every step matches the float64 reference of that step, started from the arenas as they were
    before it, within the bounded tier's bound for each parameter view; a skipped parameter's range is not touched and its
    step count stays behind; the padding floats between parameters stay zero in all four arenas"""
    t0 = time.time()
    gen = torch.Generator(device=DEV).manual_seed(3)
    shapes = [(2048, 2049), (7,), (3, 5), (1027,), (1,), (64, 3, 3, 3)]
    ps = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=gen) * 0.1) for s in shapes]
    lr, b1, b2, eps = 1e-4, 0.9, 0.999, 1e-8
    opt = sisr_amd.optim.FlatAdam(ps, lr=lr, betas=(b1, b2), eps=eps)
    assert opt.total > ADAM_CAP and opt.total == sum(-(-p.numel() // 4) * 4 for p in ps)
    pad = torch.ones(opt.total, dtype=torch.bool, device=DEV)
    for p in ps:
        pad[opt.offsets[p]:opt.offsets[p] + p.numel()] = False
    assert int(pad.sum()) == 1 + 1 + 1 + 3
    steps = [0] * len(ps)
    for step in range(3):
        before = [a.clone() for a in (opt.flat_p, opt.flat_m, opt.flat_v)]
        for k, p in enumerate(ps):
            if k == 3 and step == 1:
                p.grad = None
                continue
            mag = 10.0 ** (torch.rand(p.shape, device=DEV, generator=gen) * 6 - 6)
            p.grad = mag * (torch.randint(0, 2, p.shape, device=DEV, generator=gen) * 2 - 1)
            steps[k] += 1
        opt.step()
        for k, p in enumerate(ps):
            o, n = opt.offsets[p], p.numel()
            got = [a[o:o + n] for a in (opt.flat_p, opt.flat_m, opt.flat_v)]
            was = [a[o:o + n] for a in before]
            if p.grad is None:
                assert all(torch.equal(a, b) for a, b in zip(got, was)), "a skipped parameter was updated"
                continue
            sc = R.adam_scalars(lr, b1, b2, eps, steps[k])
            g = p.grad.reshape(-1)
            ref, mag = R.adam_ref(was[0], g, was[1], was[2], **sc), R.adam_ref(was[0], g, was[1], was[2], **sc, A=True)
            for name, a in (("p", got[0]), ("m", got[1]), ("v", got[2])):
                bounded(a, ref[name], mag[name], C_ADAM[name], f"FlatAdam {name}")
        for a in (opt.flat_p, opt.flat_g, opt.flat_m, opt.flat_v):
            assert bool((a[pad] == 0).all()), "a padding float between parameters is no longer zero"
    assert steps == [3, 3, 3, 2, 3, 3] and float(opt.state_dict()["state"][3]["step"]) == 2.0
    torch.cuda.synchronize()
    print(f"FlatAdam over {opt.total} floats, three steps and their comparisons: {time.time() - t0:.2f} s")


# ============================================================================ 2a. SFT weight composition
SFT_M = [0, 1, 10, 16, 17, 32, 33, 63, 64]


def sft_distinct_params(M, base=0):
    """the eight parameters, distinct non-zero integers (exact in fp32): arange offset per tensor"""
    return [torch.arange(1, int(np.prod(s)) + 1, dtype=torch.float32).reshape(s) + base + 200000 * k
            for k, s in enumerate(R.SFT_PARAM_SHAPES(M))]


def compose_launch(prm, merged, M, split):
    return lib().sisr_sft_compose(*[P(t) for t in prm], *[P(t) for t in merged], M, split, St())


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("M", SFT_M)
def test_sft_compose_places_every_weight_and_writes_positive_zeros(M):
    prm = sft_distinct_params(M)
    dprm = [dev(t) for t in prm]
    merged = [nan(*s) for s in R.SFT_MERGED_SHAPES]
    ok(compose_launch(dprm, merged, M, 0), "sisr_sft_compose")
    ref = R.sft_compose_ref([t.double() for t in prm], M)
    for name, got, want in zip(("WA", "bA", "WB", "bB"), merged, ref):
        X.assert_exact(got, want, f"{name}, M = {M}")
    za, zb = R.sft_structural(M)
    for got, z in ((merged[0], za), (merged[2], zb)):
        zeros = got.cpu()[z]
        assert bool((zeros == 0).all()) and not bool(torch.signbit(zeros).any()), "a structural zero is not +0.0"
    assert all(torch.equal(a.cpu(), b) for a, b in zip(dprm, prm)), "composing modified a parameter"


@pytest.mark.parametrize("M", SFT_M)
def test_sft_split_reads_only_the_real_blocks(M):
    """the merged gradients hold distinct values where a parameter sits and NaN at the structural zeros: the eight
    outputs equal the slices, no NaN arrives, and the merged tensors are left as they were"""
    src = [torch.arange(1, int(np.prod(s)) + 1, dtype=torch.float32).reshape(s) + 300000 * k for k, s in enumerate(R.SFT_MERGED_SHAPES)]
    za, zb = R.sft_structural(M)
    src[0][za], src[2][zb] = NAN, NAN
    merged = [dev(t) for t in src]
    keep = [bits(t).clone() for t in merged]
    outs = [nan(*s) for s in R.SFT_PARAM_SHAPES(M)]
    ok(compose_launch(outs, merged, M, 1), "sisr_sft_compose(split)")
    for k, (got, want) in enumerate(zip(outs, R.sft_split_ref(src, M))):
        assert not bool(got.isnan().any()), f"output {k}: a NaN arrived (unwritten, or read from a structural zero)"
        X.assert_exact(got, want.double(), f"split output {k}, M = {M}")
    assert all(torch.equal(bits(a), b) for a, b in zip(merged, keep)), "the split wrote into a merged tensor"


@pytest.mark.parametrize("layers", [1, 3, 40])
def test_sft_compose_many_equals_compose_per_layer(layers):
    """different M per record; the records' split field is 1, which sisr_sft_compose_many ignores (it always composes)"""
    L = lib()
    rec = np.zeros(layers, dtype=[("p", "<u8", (12,)), ("M", "<i4"), ("split", "<i4")])
    assert rec.dtype.itemsize == L.sisr_sft_compose_record_bytes() == 12 * 8 + 2 * 4
    Ms = [SFT_M[(3 * k + 1) % len(SFT_M)] for k in range(layers)]
    prms = [[dev(t) for t in sft_distinct_params(M, base=17 * k)] for k, M in enumerate(Ms)]
    many = [[nan(*s) for s in R.SFT_MERGED_SHAPES] for _ in range(layers)]
    for k in range(layers):
        rec[k] = ([t.data_ptr() for t in prms[k]] + [t.data_ptr() for t in many[k]], Ms[k], 1)
    table = torch.from_numpy(rec.view(np.uint8)).to(DEV)
    ok(L.sisr_sft_compose_many(P(table), layers, St()), "sisr_sft_compose_many")
    for k in range(layers):
        one = [nan(*s) for s in R.SFT_MERGED_SHAPES]
        ok(compose_launch(prms[k], one, Ms[k], 0), "sisr_sft_compose")
        for a, b in zip(many[k], one):
            assert not bool(a.isnan().any()) and torch.equal(bits(a), bits(b)), f"layer {k} (M = {Ms[k]})"
    assert all(torch.equal(a.cpu(), b) for a, b in zip(prms[-1], sft_distinct_params(Ms[-1], base=17 * (layers - 1))))


def test_sft_compose_refusals():
    L = lib()
    prm = [dev(t) for t in sft_distinct_params(1)]
    merged = [nan(*s) for s in R.SFT_MERGED_SHAPES]
    for M in (-1, 65):
        assert compose_launch(prm, merged, M, 0) == ERR_ARG
    for k in range(12):
        ptrs = [P(t) for t in prm + merged]
        ptrs[k] = None
        assert L.sisr_sft_compose(*ptrs, 1, 0, St()) == ERR_ARG
    table = torch.zeros(104, dtype=torch.uint8, device=DEV)
    assert L.sisr_sft_compose_many(P(table), 0, St()) == ERR_ARG
    assert L.sisr_sft_compose_many(P(table), 65536, St()) == ERR_ARG
    assert L.sisr_sft_compose_many(None, 1, St()) == ERR_ARG
    assert R.untouched(*merged)


def test_sft_compose_detector():
    """one element of add_conv1's weight moved in the kernel's copy: WA mismatches at exactly its place"""
    M = 17
    prm = sft_distinct_params(M)
    base = R.sft_compose_ref([t.double() for t in prm], M)
    moved = [t.clone() for t in prm]
    moved[2][31, 64 + M - 1, 2, 2] += 0.5
    merged = [nan(*s) for s in R.SFT_MERGED_SHAPES]
    ok(compose_launch([dev(t) for t in moved], merged, M, 0), "sisr_sft_compose")
    want = R.sft_compose_ref([t.double() for t in moved], M)[0] != base[0]
    assert int(want.sum()) == 1 and bool(want[63, 64 + M - 1, 2, 2])
    R.expect_detected(X.mismatch(merged[0], base[0]), want, "WA")
    X.assert_exact(merged[2], base[2], "WB")


# ============================================================================ 2b. SFT combine
SFT_CAP = 65535 * 256 // 16  # pixels one pass of the capped grid covers (one float4 per thread): 1 048 560
COMBINE_NPIX = [1, 15, 16, 17, 255, 257, 4099]


def combine_fwd(x, xs, y2, md, os_, relu):
    """x, md [npix][64], y2 [npix][128] on the host -> the NaN-pre-filled [npix][os_] output buffer"""
    npix = x.shape[0]
    out = nan(npix, os_)
    ok(lib().sisr_sft_combine_fwd(P(strided(x, xs)), xs, P(dev(y2)), P(dev(md)) if md is not None else None, P(out), os_, npix,
                                  int(relu), St()), "sisr_sft_combine_fwd")
    return out


def combine_bwd(dout, ds, x, xs, y2, relu):
    npix = x.shape[0]
    dx, dy2 = nan(npix, 64), nan(npix, 128)
    ok(lib().sisr_sft_combine_bwd(P(strided(dout, ds)), ds, P(strided(x, xs)), xs, P(dev(y2)), P(dx), P(dy2), npix, int(relu),
                                  St()), "sisr_sft_combine_bwd")
    return dx, dy2


def combine_exact_data(npix, seed):
    """y2[:, :64] = 0, so s = 1 / (1 + expf(-0)) = 0.5 exactly; x integers in [-2, 2], a = k / 8 with every third element
    set to -x / 2 (pre == 0 exactly), dout integers"""
    x, a, dout = X.ints((npix, 64), seed), X.weights((npix, 64), seed + 1), X.nonzero_ints((npix, 64), seed + 2)
    zero = torch.arange(npix * 64).reshape(npix, 64) % 3 == 0
    a = torch.where(zero, -x / 2, a)
    return x, torch.cat([torch.zeros(npix, 64), a], 1), dout


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("npix", COMBINE_NPIX)
def test_sft_combine_exact(npix, relu):
    x, y2, dout = combine_exact_data(npix, seed=10 * npix + relu)
    md = X.ints((npix, 64), npix + 7, -100, 100)
    f = R.sft_combine_fwd_ref(x, y2, relu)
    assert bool((f["pre"] == 0).sum() >= npix * 64 // 3) and bool((f["s"] == 0.5).all())
    X.assert_budget(R.sft_combine_fwd_ref(x, y2, relu, A=True)["out"], 1 / 8, "SFT combine")
    for xs in (64, 128, 192):
        for os_ in (64, 128, 192):
            out = combine_fwd(x, xs, y2, None, os_, relu)
            X.assert_exact(out[:, :64], f["out"], f"out, npix = {npix}, strides {xs} -> {os_}")
            assert gaps_untouched(out, 0), "the forward wrote into a stride gap"
        for os_ in (128, 192):
            out = combine_fwd(x, xs, y2, md, os_, relu)
            X.assert_exact(out[:, :64], f["out"], f"out (with md), npix = {npix}, strides {xs} -> {os_}")
            assert torch.equal(bits(out[:, 64:128]), bits(dev(md))), "the metadata chunk is not a bit copy"
            assert gaps_untouched(out, 0, 64), "the forward wrote behind the metadata chunk"
    b = R.sft_combine_bwd_ref(dout, x, y2, relu)
    if relu:
        assert bool((b["da"][f["pre"] == 0] == 0).all())  # the gradient at pre == 0 is 0
    for ds in (64, 128):
        for xs in (64, 128, 192):
            dx, dy2 = combine_bwd(dout, ds, x, xs, y2, relu)
            X.assert_exact(dx, b["dx"], f"dx, npix = {npix}")
            X.assert_exact(dy2[:, :64], b["dm"], f"dm, npix = {npix}")
            X.assert_exact(dy2[:, 64:], b["da"], f"da, npix = {npix}")


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("npix", [17, 4099])
def test_sft_combine_bounded(npix, relu):
    """|m| <= 12.  Forward: s carries C_SIG, the product and the sum one rounding each (fused or not) -> C_SIG + 2 of
    |x| s + |a|.  Backward, as derived for sisr_spar3d in tests/test_spar_han_gpu.py: dx = g s -> C_SIG + 1 of |g| s;
    dm = g x s (1 - s), (1 - s) carries s's absolute error -> C_SIG + 4 of the A-form |g x| s (1 + s); da = g exactly.
    The ReLU mask is taken from the kernel's own forward output (out > 0): an element whose float64 pre lies within
    rounding of zero may sit on either side, and the mask-consistency test below holds the two kernels to one answer."""
    g = torch.Generator().manual_seed(npix + relu)
    x, a, dout = (torch.randn(npix, 64, generator=g) for _ in range(3))
    y2 = torch.cat([(torch.rand(npix, 64, generator=g) * 2 - 1) * 12, a], 1)
    out = combine_fwd(x, 128, y2, None, 64, relu)
    f, fm = R.sft_combine_fwd_ref(x, y2, relu), R.sft_combine_fwd_ref(x, y2, relu, A=True)
    bounded(out, f["out"], fm["out"], C_SIG + 2, "SFT combine out")
    dx, dy2 = combine_bwd(dout, 128, x, 64, y2, relu)
    pre = torch.where(out.cpu() > 0, 1.0, -1.0) if relu else None
    b = R.sft_combine_bwd_ref(dout, x, y2, relu, pre=pre)
    bm = R.sft_combine_bwd_ref(dout, x, y2, relu, A=True, pre=pre)
    bounded(dx, b["dx"], bm["dx"], C_SIG + 1, "SFT combine dx")
    bounded(dy2[:, :64], b["dm"], bm["dm"], C_SIG + 4, "SFT combine dm")
    X.assert_exact(dy2[:, 64:], b["da"], "da")
    if relu:  # the float64 mask disagrees with the kernel's only where pre is within the forward bound of zero
        flip = (f["pre"] > 0) != (out.cpu() > 0)
        assert bool((f["pre"].abs()[flip] <= (C_SIG + 2) * U * fm["out"][flip]).all())


def test_sft_combine_above_the_grid_cap():
    """npix = 1 048 560 + 37: the first size at which the capped grid strides.  Exact-tier data generated on the device,
    compared there in slices"""
    t0 = time.time()
    npix = SFT_CAP + 37
    gen = torch.Generator(device=DEV).manual_seed(1)
    x = torch.randint(-2, 3, (npix, 64), device=DEV, generator=gen).float()
    a = torch.randint(-4, 5, (npix, 64), device=DEV, generator=gen).float() / 8
    a = torch.where(torch.randint(0, 3, (npix, 64), device=DEV, generator=gen) == 0, -x / 2, a)
    dout = torch.randint(1, 3, (npix, 64), device=DEV, generator=gen).float()
    y2 = torch.cat([torch.zeros(npix, 64, device=DEV), a], 1)
    out, dx, dy2 = nan(npix, 64), nan(npix, 64), nan(npix, 128)
    ok(lib().sisr_sft_combine_fwd(P(x), 64, P(y2), None, P(out), 64, npix, 1, St()), "sisr_sft_combine_fwd")
    ok(lib().sisr_sft_combine_bwd(P(dout), 64, P(x), 64, P(y2), P(dx), P(dy2), npix, 1, St()), "sisr_sft_combine_bwd")
    step = 1 << 18
    for p0 in range(0, npix, step):
        s = slice(p0, min(npix, p0 + step))
        f = R.sft_combine_fwd_ref(x[s], y2[s], 1)
        b = R.sft_combine_bwd_ref(dout[s], x[s], y2[s], 1)
        X.assert_exact(out[s], f["out"], f"out, pixels from {p0}")
        X.assert_exact(dx[s], b["dx"], f"dx, pixels from {p0}")
        X.assert_exact(dy2[s, :64], b["dm"], f"dm, pixels from {p0}")
        X.assert_exact(dy2[s, 64:], b["da"], f"da, pixels from {p0}")
    torch.cuda.synchronize()
    print(f"SFT combine forward + backward at {npix} pixels and their comparisons: {time.time() - t0:.2f} s")


def test_sft_combine_backward_mask_agrees_with_the_forward_sign():
    """s is the kernel's own sigmoid (a forward launch with x = 1, a = 0 and no ReLU returns it exactly, fused or not);
    a = -fl32(x s), the product rounded in fp32 on the host: x s + a is 0 when product and sum round separately and the
    product's rounding residue, of either sign, when they are fused.  Whatever the forward kernel stored, the backward
    kernel's recomputed mask must say the same, element by element: out > 0 exactly where da != 0"""
    npix = 4099
    g = torch.Generator().manual_seed(77)
    x = torch.randn(npix, 64, generator=g)
    m = (torch.rand(npix, 64, generator=g) * 2 - 1) * 12
    y2 = torch.cat([m, torch.zeros(npix, 64)], 1)
    s = combine_fwd(torch.ones(npix, 64), 64, y2, None, 64, 0).cpu()
    assert bool(((s > 0) & (s < 1)).all())
    a = -(x.double() * s.double()).float()
    y2 = torch.cat([m, a], 1)
    out = combine_fwd(x, 64, y2, None, 64, 1)
    _, dy2 = combine_bwd(torch.ones(npix, 64), 64, x, 64, y2, 1)
    da = dy2[:, 64:]
    assert not bool(out.isnan().any()) and not bool(da.isnan().any())
    pos = out > 0
    print(f"mask consistency: {int(pos.sum())} of {pos.numel()} pre-activations stored positive, "
          f"{int(((da != 0) != pos).sum())} masks disagree")
    assert torch.equal(pos, da != 0), f"{int(((da != 0) != pos).sum())} elements: the backward mask contradicts the forward output"
    assert bool((da[pos] == 1).all())


def test_sft_combine_refusals():
    L = lib()
    z, off = misaligned(4 * 192)
    outs = [nan(4 * 192) for _ in range(3)]
    o, dx, dy2 = outs
    for xs, os_ in ((60, 64), (66, 64), (64, 60), (64, 66)):
        assert L.sisr_sft_combine_fwd(P(z), xs, P(z), None, P(o), os_, 4, 1, St()) == ERR_ARG
    assert L.sisr_sft_combine_fwd(P(z), 64, P(z), P(z), P(o), 64, 4, 1, St()) == ERR_ARG  # md needs a second chunk
    assert L.sisr_sft_combine_fwd(P(z), 64, P(z), None, P(o), 64, 0, 1, St()) == ERR_ARG
    assert L.sisr_sft_combine_fwd(None, 64, P(z), None, P(o), 64, 4, 1, St()) == ERR_ARG
    for args in ((off, z, None), (z, off, None), (z, z, off)):
        assert L.sisr_sft_combine_fwd(P(args[0]), 64, P(args[1]), P(args[2]), P(o), 128, 4, 1, St()) == ERR_ALIGN
    assert L.sisr_sft_combine_fwd(P(z), 64, P(z), None, P(o, 1), 64, 4, 1, St()) == ERR_ALIGN
    for ds, xs in ((60, 64), (66, 64), (64, 60), (64, 66)):
        assert L.sisr_sft_combine_bwd(P(z), ds, P(z), xs, P(z), P(dx), P(dy2), 4, 1, St()) == ERR_ARG
    assert L.sisr_sft_combine_bwd(P(z), 64, P(z), 64, P(z), P(dx), None, 4, 1, St()) == ERR_ARG
    for k in range(3):
        ptrs = [P(z), P(z), P(z)]
        ptrs[k] = P(off)
        assert L.sisr_sft_combine_bwd(ptrs[0], 64, ptrs[1], 64, ptrs[2], P(dx), P(dy2), 4, 1, St()) == ERR_ALIGN
    assert L.sisr_sft_combine_bwd(P(z), 64, P(z), 64, P(z), P(dx, 1), P(dy2), 4, 1, St()) == ERR_ALIGN
    assert R.untouched(*outs)


def test_sft_combine_detector():
    """one x element of the last pixel moved in the kernel's copy: out, dm mismatch at that element only; one y2 add
    element moved across zero: out and all three gradients at that element"""
    npix = 257
    x, y2, dout = combine_exact_data(npix, seed=3)
    x[npix - 1, 62], y2[npix - 1, 64 + 62] = 2.0, 0.25  # pre = 1.25 > 0
    f, b = R.sft_combine_fwd_ref(x, y2, 1), R.sft_combine_bwd_ref(dout, x, y2, 1)
    xp = x.clone()
    xp[npix - 1, 62] = 1.0
    want = R.sft_combine_fwd_ref(xp, y2, 1)["out"] != f["out"]
    assert int(want.sum()) == 1
    R.expect_detected(X.mismatch(combine_fwd(xp, 64, y2, None, 64, 1), f["out"]), want, "out")
    dx, dy2 = combine_bwd(dout, 64, xp, 64, y2, 1)
    X.assert_exact(dx, b["dx"], "dx")
    R.expect_detected(X.mismatch(dy2[:, :64], b["dm"]), R.sft_combine_bwd_ref(dout, xp, y2, 1)["dm"] != b["dm"], "dm")
    yp = y2.clone()
    yp[npix - 1, 64 + 62] = -2.0  # pre = -1: masked
    R.expect_detected(X.mismatch(combine_fwd(x, 64, yp, None, 64, 1), f["out"]), want, "out (a)")
    dx, dy2 = combine_bwd(dout, 64, x, 64, yp, 1)
    for name, got in (("dx", dx), ("dm", dy2[:, :64]), ("da", dy2[:, 64:])):
        R.expect_detected(X.mismatch(got, b[name]), want, name)


# ============================================================================ 2c. strided 64-channel maps
NEEDS_B = (1, 3, 4, 6, 7)


def map64(op, a, a_stride, b, b_stride, out_stride, a_off=0, out_off=0):
    """a, b [npix][64] on the host (op 7: b [npix]) laid into NaN buffers of the given strides -> the NaN-pre-filled output"""
    npix = a.shape[0]
    out = nan(npix, out_stride)
    bb = None
    if b is not None:
        if op == 7:
            bb = nan(npix, b_stride)
            bb[:, 0] = b.to(DEV)
        else:
            bb = strided(b, b_stride)
    ok(lib().sisr_map64(P(strided(a, a_stride, a_off), a_off), a_stride, P(bb), b_stride, P(out, out_off), out_stride, npix, op,
                        St()), f"sisr_map64 op {op}")
    return out


def map64_data(op, npix, seed):
    """ops 0, 1, 4, 7: dyadic (sums and products exact); ops 2, 3, 5, 6: general fp32 values, whose references are exact
    by themselves, with +0.0, -0.0 and the smallest values of either sign in a"""
    if op in (0, 1, 4, 7):
        a, b = X.ints((npix, 64), seed, -100, 100), X.weights((npix, 64), seed + 1, nonzero=True)
        return a, (b[:, 0].clone() if op == 7 else b)
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(npix, 64, generator=g), torch.randn(npix, 64, generator=g)
    a[0, :6] = torch.tensor([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 1.0, -1.0])
    a[npix - 1, 60:] = torch.tensor([-0.0, 0.0, -3.0, 3.0])
    return a, b


@pytest.mark.parametrize("npix", [1, 17, 4099])
@pytest.mark.parametrize("op", range(8))
def test_map64_ops_exact(op, npix):
    a, b = map64_data(op, npix, seed=100 * op + npix)
    if op not in NEEDS_B:
        b = None
    ref = R.map64_ref(op, a, b)
    b_strides = (4, 64) if op == 7 else (64, 128)
    for a_stride in (64, 128):
        for b_stride in (b_strides if b is not None else (0,)):
            for out_stride in (64, 128):
                out = map64(op, a, a_stride, b, b_stride, out_stride)
                X.assert_exact(out[:, :64], ref, f"op {op}, npix = {npix}, strides {a_stride}, {b_stride} -> {out_stride}")
                assert gaps_untouched(out, 0)
    if op in (2, 3, 5, 6):  # at +-0 the activation is 0 and the gradient takes the `<= 0` branch
        out = map64(op, a, 64, b, 64, 64).cpu()
        zero = a == 0
        assert int(zero.sum()) >= 4
        if op == 3:
            assert torch.equal(out[zero].double(), X.fp32_round(b[zero].double() * X.SLOPE32))
        else:
            assert bool((out[zero] == 0).all())


def test_map64_copy_between_chunk_offsets_and_in_place_leaky():
    """op 0 from the second chunk of a into the second chunk of out (the metadata-chunk fill): the first chunk stays NaN.
    op 2 in place (out == a), as the SFTMD head runs it after its 3-channel conv, at strides 64 and 128"""
    npix = 4099
    a = X.ints((npix, 64), 5, -100, 100)
    out = map64(0, a, 128, None, 0, 128, a_off=64, out_off=64)
    X.assert_exact(out[:, 64:], a.double(), "copy into the second chunk")
    assert gaps_untouched(out, 64)
    out = map64(0, a, 192, None, 0, 128, a_off=128, out_off=0)
    X.assert_exact(out[:, :64], a.double(), "copy from the third chunk")
    assert gaps_untouched(out, 0)
    v, _ = map64_data(2, npix, seed=6)
    for stride in (64, 128):
        buf = strided(v, stride)
        ok(lib().sisr_map64(P(buf), stride, None, 0, P(buf), stride, npix, 2, St()), "sisr_map64 in place")
        X.assert_exact(buf[:, :64], R.map64_ref(2, v), f"in-place LeakyReLU, stride {stride}")
        assert gaps_untouched(buf, 0)


def test_map64_refusals():
    L = lib()
    z, off = misaligned(4 * 128)
    o = nan(4 * 128)
    for op in (-1, 8):
        assert L.sisr_map64(P(z), 64, P(z), 64, P(o), 64, 4, op, St()) == ERR_ARG
    for op in NEEDS_B:
        assert L.sisr_map64(P(z), 64, None, 64, P(o), 64, 4, op, St()) == ERR_ARG
    for sa, sb, so in ((60, 64, 64), (66, 64, 64), (64, 6, 64), (64, 64, 60), (64, 64, 66)):
        assert L.sisr_map64(P(z), sa, P(z), sb, P(o), so, 4, 1, St()) == ERR_ARG
    for op in (1, 3, 4, 6):  # a one-channel-padded b is op 7's alone: the others read 64 channels per pixel
        assert L.sisr_map64(P(z), 64, P(z), 4, P(o), 64, 4, op, St()) == ERR_ARG
    assert L.sisr_map64(P(z), 64, P(z), 6, P(o), 64, 4, 7, St()) == ERR_ARG
    assert L.sisr_map64(P(z), 64, None, 0, P(o), 64, 0, 0, St()) == ERR_ARG
    assert L.sisr_map64(None, 64, None, 0, P(o), 64, 4, 0, St()) == ERR_ARG
    assert L.sisr_map64(P(off), 64, P(z), 64, P(o), 64, 4, 1, St()) == ERR_ALIGN
    assert L.sisr_map64(P(z), 64, P(off), 64, P(o), 64, 4, 1, St()) == ERR_ALIGN
    assert L.sisr_map64(P(z), 64, P(z), 64, P(o, 1), 64, 4, 1, St()) == ERR_ALIGN
    assert R.untouched(o)


def test_map64_detector():
    """one b element moved: op 1 mismatches at that element; op 7 (b's channel 0 of one pixel): at that pixel's 64 features"""
    npix = 4099
    a, b = X.nonzero_ints((npix, 64), 1), X.weights((npix, 64), 2, nonzero=True)
    bp = b.clone()
    bp[npix - 1, 63] += 0.125
    base = R.map64_ref(1, a, b)
    want = R.map64_ref(1, a, bp) != base
    assert int(want.sum()) == 1
    R.expect_detected(X.mismatch(map64(1, a, 64, bp, 128, 64)[:, :64], base), want, "a + b")
    b0, b0p = b[:, 0].clone(), b[:, 0].clone()
    b0p[2048] += 0.125
    base = R.map64_ref(7, a, b0)
    want = R.map64_ref(7, a, b0p) != base
    assert int(want.sum()) == 64 and bool(want[2048].all())
    R.expect_detected(X.mismatch(map64(7, a, 64, b0p, 4, 64)[:, :64], base), want, "a * b[0]")


# ============================================================================ 2d. clamp
CLAMP_EDGES = [-1.0, -0.0, 0.0, 2.0 ** -149, 0.5, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23, 2.0]


def clamp_run(a, g):
    n = a.numel()
    out, da = nan(n), nan(n)
    ok(lib().sisr_clamp01(P(dev(a)), None, P(out), n, 0, St()), "sisr_clamp01")
    ok(lib().sisr_clamp01(P(dev(a)), P(dev(g)), P(da), n, 1, St()), "sisr_clamp01(backward)")
    return out, da


@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_clamp01_is_inclusive_at_both_ends(n):
    """the edge values (once at the front, once at the back of the range; n = 1: one launch each) in a random fill; the
    gradient passes at exactly 0, -0.0 and 1 and stops at the next value above 1"""
    gen = torch.Generator().manual_seed(n)
    edges = torch.tensor(CLAMP_EDGES, dtype=torch.float32)
    assert float(edges[5]) < 1.0 < float(edges[7]) and float(edges[3]) > 0.0
    g = X.nonzero_ints((max(n, 9),), n + 1, 4)
    cases = [edges[k:k + 1] for k in range(9)] if n == 1 else [torch.randn(n, generator=gen) * 0.7 + 0.5]
    for a in cases:
        if n > 1:
            a[:9], a[n - 9:] = edges, edges.flip(0)
        out, da = clamp_run(a, g[:n])
        X.assert_exact(out, R.clamp01_ref(a), f"clamp, n = {n}")
        X.assert_exact(da, R.clamp01_bwd_ref(a, g[:n]), f"clamp backward, n = {n}")
    o = nan(8)
    assert lib().sisr_clamp01(P(o), None, P(o), 0, 0, St()) == ERR_ARG and lib().sisr_clamp01(P(o), None, P(o), 8, 1, St()) == ERR_ARG
    assert R.untouched(o)


# ============================================================================ 2e. ops.sft_layer at its rule boundaries
def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("shape", [(2, 10, 37), (1, 5, 9)])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M", [16, 17, 32, 33])
def test_sft_layer_at_the_metadata_widths_where_its_sparsity_rules_switch(M, relu, shape):
    """M <= 16 promises the first conv that input channels >= 80 are zero, M <= 32 leaves dWA[:, 96:] uncomputed: at M = 16
    and 32 the last metadata channel is the last one inside the rule, at 17 and 33 the first outside.  Reference: the
    four-conv formulation of tests/test_sftmd_gpu.py (test_sft_layer_matches_the_four_conv_formulation) in float64; bounds:
    that test's rel < 2e-6 forward and 5e-6 on gradients; the metadata columns of the first convs' weight gradients are
    compared one by one, so a dropped or uncomputed channel shows"""
    B, H, W = shape
    g = torch.Generator().manual_seed(5 + M)
    torch.manual_seed(50 + M)
    mod = sisr_amd.sftmd.StandardSft(nf=64, para=M)
    x = torch.randn(B, 64, H, W, generator=g)
    md = torch.rand(B, M, H, W, generator=g) + 0.1
    assert bool((md[:, M - 1] != 0).all())
    cot = torch.randn(B, 64, H, W, generator=g)
    ref = sisr_amd.sftmd.StandardSft(nf=64, para=M).double()
    ref.load_state_dict({k: v.double() for k, v in mod.state_dict().items()})
    xr = x.double().requires_grad_(True)
    cat = torch.cat((xr, md.double()), 1)
    mul = torch.sigmoid(ref.mul_conv2(F.leaky_relu(ref.mul_conv1(cat), 0.2)))
    add = ref.add_conv2(F.leaky_relu(ref.add_conv1(cat), 0.2))
    want = xr * mul + add
    want = F.relu(want) if relu else want
    want.backward(cot.double())
    ref_g = {k: p.grad.clone() for k, p in ref.named_parameters()}
    mod.to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out = ops.sft_layer(xg, ops.nchw_to_nhwc_pad(md.to(DEV), 64), mod, relu)
    r = rel(out, want)
    print(f"sft_layer M={M} relu={relu} {shape}: rel(out) = {r:.2e}")
    assert r < 2e-6
    out.backward(cot.to(DEV))
    r = rel(xg.grad, xr.grad)
    print(f"  rel(dx) = {r:.2e}")
    assert r < 5e-6
    for k, p in mod.named_parameters():
        r = rel(p.grad, ref_g[k])
        print(f"  rel(d {k}) = {r:.2e}")
        assert r < 5e-6, k
    for name in ("mul_conv1.weight", "add_conv1.weight"):
        got = dict(mod.named_parameters())[name].grad
        worst = max((rel(got[:, 64 + c], ref_g[name][:, 64 + c]), c) for c in range(M))
        print(f"  d {name}, metadata columns: worst rel {worst[0]:.2e} at channel {worst[1]}")
        for c in range(M):
            assert rel(got[:, 64 + c], ref_g[name][:, 64 + c]) < 5e-6, (name, c)


# ============================================================================ 3. layout and rounding kernels
def distinct(*shape, base=1):
    """distinct non-zero integers, exact in fp32"""
    return torch.arange(base, base + int(np.prod(shape)), dtype=torch.float32).reshape(shape)


@pytest.mark.parametrize("B,C,H,W,Cp", [(1, 1, 1, 1, 4), (2, 13, 5, 7, 64), (1, 3, 9, 33, 64), (1, 64, 4, 4, 64), (2, 67, 3, 5, 128),
                                        (1, 5, 2, 3, 8)])
def test_nchw_to_nhwc_pad(B, C, H, W, Cp):
    x = distinct(B, C, H, W)
    y = nan(B, H, W, Cp)
    ok(lib().sisr_nchw_to_nhwc_pad(P(dev(x)), P(y), B, C, H, W, Cp, St()), "sisr_nchw_to_nhwc_pad")
    X.assert_exact(y, R.nchw_to_nhwc_pad_ref(x, Cp).double(), "NHWC map")
    assert not bool(torch.signbit(y[..., C:]).any()), "a padded channel is not +0.0"
    assert torch.equal(ops.nchw_to_nhwc_pad(dev(x), Cp).permute(0, 2, 3, 1), y)


MISC_CAP = 65535 * 256  # elements (float4 for the NHWC map, 8 floats for bf16) one pass of the capped grid covers


def test_layout_kernels_above_the_grid_cap():
    """the first sizes at which the capped grids of the layout kernels stride, data generated and compared on the device:
    a 1024 x 1025 RGB input into a 64-channel map (16 793 600 float4), a 600 x 600 x 48 map shuffled by 4 (17 280 000
    elements) and back, and 8 (MISC_CAP + 300) floats rounded to bf16 (against the device's own conversion)"""
    t0 = time.time()
    L = lib()
    B, C, H, W, Cp = 1, 3, 1024, 1025, 64
    assert H * W * (Cp // 4) > MISC_CAP
    x = torch.arange(1, C * H * W + 1, dtype=torch.float32, device=DEV).reshape(B, C, H, W)
    y = nan(B, H, W, Cp)
    ok(L.sisr_nchw_to_nhwc_pad(P(x), P(y), B, C, H, W, Cp, St()), "sisr_nchw_to_nhwc_pad")
    assert torch.equal(y[..., :C], x.permute(0, 2, 3, 1)) and bool((y[..., C:] == 0).all())
    del x, y
    C, r, H, W, Cp = 3, 4, 600, 600, 48
    assert C * H * r * W * r > MISC_CAP and H * W * Cp > MISC_CAP
    src = torch.arange(1, H * W * Cp + 1, dtype=torch.float32, device=DEV).reshape(1, H, W, Cp)
    out = nan(1, C, H * r, W * r)
    ok(L.sisr_shuffle_rgb(P(src), P(out), 1, C, r, H, W, Cp, 0, St()), "sisr_shuffle_rgb")
    assert torch.equal(out, F.pixel_shuffle(src.permute(0, 3, 1, 2), r))
    back = nan(1, H, W, Cp)
    ok(L.sisr_shuffle_rgb(P(out), P(back), 1, C, r, H, W, Cp, 1, St()), "sisr_shuffle_rgb(adjoint)")
    assert torch.equal(back, src)
    del src, out, back
    n = 8 * (MISC_CAP + 300)
    v = torch.randn(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    b16 = torch.full((n,), NAN, device=DEV, dtype=torch.bfloat16)
    ok(L.sisr_f32_to_bf16(P(v), b16.data_ptr(), n, St()), "sisr_f32_to_bf16")
    assert torch.equal(b16.view(torch.int16), v.to(torch.bfloat16).view(torch.int16))
    torch.cuda.synchronize()
    print(f"layout kernels above the grid cap: {time.time() - t0:.2f} s")


def test_nchw_to_nhwc_pad_refusals():
    L = lib()
    z, off = misaligned(64)
    y = nan(64)
    assert L.sisr_nchw_to_nhwc_pad(P(z), P(y), 1, 5, 1, 1, 4, St()) == ERR_ARG  # Cp < C
    for Cp in (6, 7, 9):
        assert L.sisr_nchw_to_nhwc_pad(P(z), P(y), 1, 5, 1, 1, Cp, St()) == ERR_ARG  # Cp & 3
    assert L.sisr_nchw_to_nhwc_pad(P(z), P(y), 0, 5, 1, 1, 8, St()) == ERR_ARG
    assert L.sisr_nchw_to_nhwc_pad(P(z), P(y, 1), 1, 5, 1, 1, 8, St()) == ERR_ALIGN
    assert L.sisr_nchw_to_nhwc_pad(P(off), P(y), 1, 5, 1, 1, 8, St()) == 0  # the source is read float by float
    torch.cuda.synchronize()
    assert bool((y[:8] == 0).all()) and R.untouched(y[8:])


# (co, ci, cop, cip, taps): the SRMD head / tail weights, one real row or column, 1 x 1, nothing to pad, and ops_chain._PadAxis'
# (outer, n, outer, P, inner) with an inner extent that is no tap count
PAD_CASES = [(42, 84, 64, 128, 9), (3, 64, 64, 64, 9), (64, 13, 64, 64, 9), (5, 7, 5, 12, 1), (1, 1, 1, 1, 81), (3, 5, 3, 8, 37),
             (1, 19, 1, 64, 37), (64, 2, 64, 3, 1)]


@pytest.mark.parametrize("co,ci,cop,cip,taps", PAD_CASES)
def test_pad_oihw_both_directions(co, ci, cop, cip, taps):
    L = lib()
    w = distinct(co, ci, taps)
    wp = nan(cop, cip, taps)
    ok(L.sisr_pad_oihw(P(dev(w)), P(wp), co, ci, cop, cip, taps, 0, St()), "sisr_pad_oihw")
    X.assert_exact(wp, R.pad_oihw_ref(w, cop, cip).double(), "padded weight")
    assert not bool(torch.signbit(wp).any()), "a padding zero is not +0.0"
    src = torch.full((cop, cip, taps), NAN)  # the crop must read the real block only
    src[:co, :ci] = distinct(co, ci, taps, base=1000)
    out = nan(co, ci, taps)
    ok(L.sisr_pad_oihw(P(dev(src)), P(out), co, ci, cop, cip, taps, 1, St()), "sisr_pad_oihw(crop)")
    assert not bool(out.isnan().any()), "the crop read outside the real block, or left an element unwritten"
    X.assert_exact(out, R.crop_oihw_ref(src, co, ci).double(), "cropped weight")
    back = nan(co, ci, taps)
    ok(L.sisr_pad_oihw(P(wp), P(back), co, ci, cop, cip, taps, 1, St()), "sisr_pad_oihw(crop)")
    X.assert_exact(back, w.double(), "pad, then crop")
    o = nan(4)
    assert L.sisr_pad_oihw(P(wp), P(o), co, ci, co - 1, cip, taps, 0, St()) == ERR_ARG
    assert L.sisr_pad_oihw(P(wp), P(o), co, ci, cop, ci - 1, taps, 1, St()) == ERR_ARG and R.untouched(o)


SHUFFLE_CASES = [(r, C, Cp, bhw) for r in (1, 2, 3, 4) for C in (1, 3) for Cp in sorted({-(-C * r * r // 4) * 4, 64})
                 for bhw in ((1, 1, 1), (2, 5, 7), (1, 9, 33))]


def shuffle_run(src, shape_out, B, C, r, H, W, Cp, adjoint):
    out = nan(*shape_out)
    ok(lib().sisr_shuffle_rgb(P(dev(src)), P(out), B, C, r, H, W, Cp, adjoint, St()), "sisr_shuffle_rgb")
    return out


@pytest.mark.parametrize("r,C,Cp,bhw", SHUFFLE_CASES)
def test_shuffle_rgb_and_its_adjoint(r, C, Cp, bhw):
    B, H, W = bhw
    y = distinct(B, H, W, Cp)
    out = shuffle_run(y, (B, C, H * r, W * r), B, C, r, H, W, Cp, 0)
    X.assert_exact(out, R.shuffle_rgb_ref(y, C, r).double(), "shuffle")
    g = distinct(B, C, H * r, W * r, base=7)
    dy = shuffle_run(g, (B, H, W, Cp), B, C, r, H, W, Cp, 1)
    X.assert_exact(dy, R.shuffle_rgb_adjoint_ref(g, C, r, Cp).double(), "adjoint")
    assert bool((dy[..., C * r * r:] == 0).all()) and not bool(torch.signbit(dy).any()), "padded channels of the adjoint"
    yi, gi = X.ints((B, H, W, Cp), r + C, -8, 8), X.ints((B, C, H * r, W * r), r + C + 1, -8, 8)  # <S y, g> == <y, S^T g>, exactly
    lhs = (shuffle_run(yi, (B, C, H * r, W * r), B, C, r, H, W, Cp, 0).double() * dd(gi)).sum()
    rhs = (dd(yi) * shuffle_run(gi, (B, H, W, Cp), B, C, r, H, W, Cp, 1).double()).sum()
    assert float(lhs) == float(rhs)


def test_shuffle_rgb_refusals_and_detector():
    """Cp < C r^2 is refused.  Detector of the layout family: one source element moved -> exactly one output of the
    shuffle, exactly one of the adjoint, and none when the element is a padded channel"""
    B, C, r, H, W, Cp = 2, 3, 2, 5, 7, 64
    o = nan(16)
    assert lib().sisr_shuffle_rgb(P(o), P(o), 1, 3, 2, 1, 1, 8, 0, St()) == ERR_ARG
    assert lib().sisr_shuffle_rgb(P(o), P(o), 1, 3, 0, 1, 1, 8, 0, St()) == ERR_ARG and R.untouched(o)
    y = distinct(B, H, W, Cp)
    base = R.shuffle_rgb_ref(y, C, r).double()
    yp = y.clone()
    yp[1, 4, 6, 11] += 0.5
    want = R.shuffle_rgb_ref(yp, C, r).double() != base
    assert int(want.sum()) == 1 and bool(want[1, 2, 9, 13])  # channel 11 = c 2, i 1, j 1
    R.expect_detected(X.mismatch(shuffle_run(yp, (B, C, H * r, W * r), B, C, r, H, W, Cp, 0), base), want, "shuffle")
    yp = y.clone()
    yp[1, 4, 6, 12] += 0.5  # the first padded channel: read by nobody
    X.assert_exact(shuffle_run(yp, (B, C, H * r, W * r), B, C, r, H, W, Cp, 0), base, "shuffle (padded channel moved)")
    g = distinct(B, C, H * r, W * r, base=7)
    gbase = R.shuffle_rgb_adjoint_ref(g, C, r, Cp).double()
    gp = g.clone()
    gp[0, 0, 0, 1] += 0.5
    want = R.shuffle_rgb_adjoint_ref(gp, C, r, Cp).double() != gbase
    assert int(want.sum()) == 1 and bool(want[0, 0, 0, 1])
    R.expect_detected(X.mismatch(shuffle_run(gp, (B, H, W, Cp), B, C, r, H, W, Cp, 1), gbase), want, "adjoint")


def to_bf16(x):
    """x fp32 on the host -> the kernel's 16-bit patterns (the buffer starts as bf16 NaN)"""
    n = x.numel()
    out = torch.full((n,), NAN, device=DEV, dtype=torch.bfloat16)
    ok(lib().sisr_f32_to_bf16(P(dev(x)), out.data_ptr(), n, St()), "sisr_f32_to_bf16")
    return R.bf16_bits(out.cpu())


def test_f32_to_bf16_rounds_every_pattern_to_nearest_even():
    """all 65 536 upper halves x the lower halves {0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF}: ties to even in both directions,
    carries into the exponent, the largest finite values rounding to infinity, +-0, subnormals, +-inf bit for bit; a NaN
    stays a NaN with its sign (the payload is free)"""
    x = R.bf16_patterns()
    got = to_bf16(x)
    want, isnan = R.bf16_rne_ref(x)
    fin = ~isnan
    bad = (got != want) & fin
    assert not bool(bad.any()), (f"{int(bad.sum())} patterns; first: fp32 {int(R.f32_bits(x)[bad][0]):#010x} -> "
                                 f"{int(got[bad][0]):#06x}, round to nearest even is {int(want[bad][0]):#06x}")
    assert torch.equal(got[fin], R.bf16_bits(x[fin].to(torch.bfloat16))) and torch.equal(got[fin], R.bf16_bits(X.bf16_of(x[fin].double())))
    assert bool(R.bf16_is_nan(got[isnan]).all()), "a NaN became a number"
    assert torch.equal(got[isnan] >> 15, R.f32_bits(x)[isnan] >> 31), "a NaN lost its sign"


@pytest.mark.parametrize("n", [8, 16, 2056])
def test_f32_to_bf16_random_and_refusals(n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g) * 10.0 ** float(torch.randint(-3, 4, (1,), generator=g))
    assert torch.equal(to_bf16(x), R.bf16_rne_ref(x)[0]) and torch.equal(to_bf16(x), R.bf16_bits(X.bf16_of(x.double())))
    L = lib()
    z, off = misaligned(16)
    out = torch.full((32,), NAN, device=DEV, dtype=torch.bfloat16)
    for bad_n in (12, 4, 0, -8):
        assert L.sisr_f32_to_bf16(P(z), out.data_ptr(), bad_n, St()) == ERR_ARG
    assert L.sisr_f32_to_bf16(P(off), out.data_ptr(), 8, St()) == ERR_ALIGN
    assert L.sisr_f32_to_bf16(P(z), out.data_ptr() + 4, 8, St()) == ERR_ALIGN
    assert L.sisr_f32_to_bf16(None, out.data_ptr(), 8, St()) == ERR_ARG
    assert R.untouched(out)


# ============================================================================ 4. blur and noise quantisers
BLUR_SHAPES = [(11, 11, 21), (11, 40, 21), (33, 65, 21), (32, 32, 8), (33, 31, 8), (5, 5, 8), (1, 1, 1), (64, 33, 15)]
U8_FILL = 0xA5


def blur_kernels(l, seed):
    """weights that are powers of two summing to 1: a one-hot at each corner and at the centre (a tap-order or flip mistake
    shows as a shifted image), (1/2, 1/4, 1/8, 1/16, 1/16) and sixteen taps of 1/16 at seeded places"""
    if l == 1:
        return [torch.ones(1, 1)]
    ks = []
    for i, j in ((0, 0), (0, l - 1), (l - 1, 0), (l - 1, l - 1), (l // 2, l // 2)):
        k = torch.zeros(l, l)
        k[i, j] = 1.0
        ks.append(k)
    g = torch.Generator().manual_seed(seed)
    for w in ([0.5, 0.25, 0.125, 0.0625, 0.0625], [0.0625] * 16):
        k = torch.zeros(l * l)
        k[torch.randperm(l * l, generator=g)[:len(w)]] = torch.tensor(w)
        ks.append(k.reshape(l, l))
    return ks


def blur_run(x, k, u8=True, f32=True):
    C, H, W = x.shape
    y = torch.full((C, H, W), U8_FILL, device=DEV, dtype=torch.uint8) if u8 else None
    yf = nan(C, H, W) if f32 else None
    rc = lib().sisr_blur_quant(P(dev(x)), P(dev(k)), y.data_ptr() if u8 else None, P(yf), C, H, W, k.shape[-1], St())
    return rc, y, yf


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("H,W,l", BLUR_SHAPES)
def test_blur_quant_exact(H, W, l, C):
    """x on the 1/256 grid in [0, 1] (0 and 1 included), power-of-two weights >= 1/16: every product is a multiple of 2^-12,
    the sum is exact in any order, fused or not, and so is acc * 255 (budget-checked): the float output and the byte,
    truncation included, must be equal -- zero differing bytes.  (11, 11, 21): the reflection at its limit l / 2 == H - 1;
    l = 8: an even kernel ((4, 3) padding) across the 32-pixel tile edge in both axes; u8 only, fp32 only, both"""
    x = X.ints((C, H, W), H * W + l + C, 0, 256) / 256
    for n, k in enumerate(blur_kernels(l, seed=l + H)):
        assert float(k.sum()) == 1.0
        ref = R.blur_ref(x, k)
        X.assert_budget(R.blur_mag(x, k) * 255, 2.0 ** -12, "blur times 255")
        want_u8 = R.quant_ref(ref)
        for u8, f32 in ((True, True), (True, False), (False, True)):
            rc, y, yf = blur_run(x, k, u8, f32)
            ok(rc, "sisr_blur_quant")
            if f32:
                X.assert_exact(yf, ref, f"blur {H}x{W} l={l}, kernel {n}")
            if u8:
                diff = int((y.cpu() != want_u8).sum())
                assert diff == 0, f"{diff} differing bytes, {H}x{W} l={l}, kernel {n}"
    if l > 1:
        y, yf = sisr_amd.degrade.blur_quant(dev(x), k, want_float=True)
        assert torch.equal(y.cpu(), want_u8) and torch.equal(yf.double().cpu(), ref)
        assert torch.equal(sisr_amd.degrade.blur_quant(dev(x), k), y)


def test_blur_quant_refusals_and_detector():
    """l = 22 and l / 2 >= H are unsupported, both outputs null is an argument error; one x element moved: the outputs
    whose taps reach it (through the reflection too) mismatch, no other"""
    L = lib()
    x = X.ints((1, 33, 40), 3, 0, 256) / 256
    k = blur_kernels(21, seed=4)[5]
    dx, dk = dev(x), dev(torch.zeros(22, 22))
    y, yf = torch.full((33 * 40,), U8_FILL, device=DEV, dtype=torch.uint8), nan(33 * 40)
    assert L.sisr_blur_quant(P(dx), P(dk), y.data_ptr(), P(yf), 1, 33, 40, 22, St()) == ERR_UNSUPPORTED
    assert L.sisr_blur_quant(P(dx), P(dk), y.data_ptr(), P(yf), 1, 10, 40, 21, St()) == ERR_UNSUPPORTED
    assert L.sisr_blur_quant(P(dx), P(dk), y.data_ptr(), P(yf), 1, 33, 10, 21, St()) == ERR_UNSUPPORTED
    assert L.sisr_blur_quant(P(dx), P(dk), y.data_ptr(), P(yf), 1, 4, 40, 8, St()) == ERR_UNSUPPORTED
    assert L.sisr_blur_quant(P(dx), P(dk), None, None, 1, 33, 40, 21, St()) == ERR_ARG
    assert R.untouched(yf) and bool((y == U8_FILL).all())
    base = R.blur_ref(x, k)
    xp = x.clone()
    xp[0, 1, 38] = (xp[0, 1, 38] + 0.5) % 1.0
    want = R.blur_ref(xp, k) != base
    rc, y, yf = blur_run(xp, k)
    ok(rc, "sisr_blur_quant")
    R.expect_detected(X.mismatch(yf, base), want, "blur")
    R.expect_detected(y.cpu() != R.quant_ref(base), R.quant_ref(R.blur_ref(xp, k)) != R.quant_ref(base), "blur bytes")


def noise_run(blur, noise, sigma):
    n = blur.numel()
    y = torch.full((n,), U8_FILL, device=DEV, dtype=torch.uint8)
    ok(lib().sisr_noise_quant(P(dev(blur)), P(dev(noise)), sigma, y.data_ptr(), n, St()), "sisr_noise_quant")
    return y.cpu()


@pytest.mark.parametrize("n", [1, 257, 4099])
def test_noise_quant(n):
    """dyadic blur, noise and sigma with sums exactly at 0 and 1, below 0 and above 1; sigma = 0 on k / 255 and its two
    neighbours (the byte boundary: fl32(v 255) decides); general data, product and sum rounded separately"""
    blur = X.ints((n,), n, 0, 256) / 256
    noise = X.ints((n,), n + 1, -8, 8)
    for sigma in (0.0, 0.125, 0.5):
        b, z = blur.clone(), noise.clone()
        edge = [(0.5, -4.0), (0.5, 4.0), (0.25, -8.0), (0.75, 8.0), (0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, -1.0)]
        for k, (bv, zv) in enumerate(edge[:n]):
            b[k], z[k] = bv, zv
        want, v = R.noise_quant_ref(b, z, sigma)
        if n > 8 and sigma == 0.125:
            assert float(v[0]) == 0.0 and float(v[1]) == 1.0 and float(v[2]) == 0.0 and float(v[3]) == 1.0
        diff = int((noise_run(b, z, sigma) != want).sum())
        assert diff == 0, f"{diff} differing bytes on dyadic data, sigma = {sigma}"
    k255 = (torch.arange(n) % 256).float() / 255
    for v in (k255, torch.nextafter(k255, torch.ones(())).clamp(0, 1), torch.nextafter(k255, -torch.ones(())).clamp(0, 1)):
        want, _ = R.noise_quant_ref(v, noise, 0.0)
        assert torch.equal(noise_run(v, noise, 0.0), want), "a byte boundary"
    g = torch.Generator().manual_seed(n)
    blur, noise = torch.rand(n, generator=g), torch.randn(n, generator=g)
    for sigma in (R.f32(0.0731), R.f32(0.31)):
        want, v = R.noise_quant_ref(blur, noise, sigma)
        diff = int((noise_run(blur, noise, sigma) != want).sum())
        assert diff == 0, f"{diff} differing bytes on general data, sigma = {sigma}"
    o = torch.full((8,), U8_FILL, device=DEV, dtype=torch.uint8)
    assert lib().sisr_noise_quant(P(dev(blur)), P(dev(noise)), 0.1, o.data_ptr(), 0, St()) == ERR_ARG
    assert lib().sisr_noise_quant(P(dev(blur)), None, 0.1, o.data_ptr(), n, St()) == ERR_ARG and bool((o == U8_FILL).all())
    if n > 1:  # detector: one noise element moved across the clamp
        b, z = torch.full((n,), 0.5), torch.zeros(n)
        z[n - 1] = 8.0
        want = R.noise_quant_ref(b, z, 0.125)[0] != R.noise_quant_ref(b, torch.zeros(n), 0.125)[0]
        assert int(want.sum()) == 1
        R.expect_detected(noise_run(b, z, 0.125) != R.noise_quant_ref(b, torch.zeros(n), 0.125)[0], want, "noise bytes")


def test_zz_report_the_bounded_ratios():
    """last in the file: the largest err / bound ratio of every bounded comparison of this run"""
    print("largest err / bound ratios of this run:", {k: round(v, 3) for k, v in sorted(RATIOS.items())})
    assert all(v == v and v <= 1.0 for v in RATIOS.values())
