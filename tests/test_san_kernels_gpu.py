"""SAN's second-order attention kernels (csrc/san.hip: covariance pooling, Newton-Schulz square root, the SOCA input
gradient, the streaming non-local attention) and the kernels around the attention (csrc/nonlocal.hip: projections, split /
pool, output projection, every gradient) against float64 (pytest -m gpu).

The native entry points are called directly through hip.lib().  References are tests/_san.py (checked against the oracle's
and PyTorch's float64 autograd by tests/test_san_cpu.py).  Every output buffer starts as NaN, so an element the kernel never
writes fails, and what it must not touch (dproj and z outside the attention domains) has to stay NaN.  Tiers:

1. Exact (zero tolerance) on dyadic data (tests/_exact.py), a budget check before each sum: covariance pooling (for a pixel
   count that is no power of two the exact sum times fl32(1 / M), rounded once), the SOCA input gradient at power-of-two
   pixel counts, the projection forward / dgrad / wgrad, split / pool and its scatter on tie windows, the output projection
   forward / backward, and the attention on selector data (logits 256 on a match, 0 or -256 otherwise).
2. Bounded, one-pass kernels behind a rounded scale: |got - ref| <= c * 2^-24 * mag, mag the `A=True` form, c derived next
   to each test from the summation depth D (the longest chain of dependent fp32 additions a term passes through).
3. Bounded, the chains (square root forward / backward, attention forward / backward on general data): per sample
   max|got - ref64| <= 8 * max(E32, 2 * 2^-24 * max|ref64|), E32 the same norm of the reference's own fp32 evaluation on
   the CPU minus its float64 one, on identical fp32 inputs.  8 covers the kernels' different summation order (4x4 register
   tiles, 4-wide k steps, 4-key softmax steps) and that E32 is one draw of rounding noise; the floor keeps a case where fp32
   happens to be exact (nk = 1) from demanding exactness.  Each case prints err / max(E32, floor).
   Largest ratios measured on an MI355X (the bar is 8): square root -- trace 0.90, pooled 2.38, last 1.49, Y_i 1.66,
   Z_i 1.16, G + G^T 1.49; attention -- y 1.78, lse 1.49, dtheta 2.57, dphi 2.03, dg 1.53, dsum 2.44.

Each family has a detector: one input element moved in the copy only the kernel sees must make the exact comparison
mismatch at exactly the outputs that element feeds; for the chains the smallest power-of-two move whose float64 effect
exceeds 4x the bar must make the bounded comparison fail.

Not tested: a zero covariance (a constant map) divides by a zero trace, in the reference as in the kernel.
The output projection's row counts are B nqy nqx hq wq with hq, wq >= 2, so 17 rows cannot be built: 18 and 34 stand in
for it next to 15 and 16.
"""
import collections
import ctypes
import math

import pytest
import torch

import _exact as X
import _gates as G
import _san as S
import sisr_amd

pytestmark = pytest.mark.gpu
hip = sisr_amd.hip
DEV = "cuda:0"
NAN = float("nan")
U = 2.0 ** -24
ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = -1, -2, -4
SENT = 32.0
CHAIN_FACTOR, CHAIN_FLOOR = 8.0, 2.0


def lib():
    return hip.lib()


_LIVE = collections.deque(maxlen=64)


def P(t):
    """device pointer of t, which stays referenced over the next calls"""
    if t is not None:
        _LIVE.append(t)
    return hip.ptr(t)


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


def cdom(dom):
    return (ctypes.c_int * 9)(*dom)


def untouched(*ts):
    torch.cuda.synchronize()
    return all(bool(t.isnan().all()) for t in ts)


def expect_detected(got_map, want_map, what):
    assert bool(want_map.any()), f"{what}: the perturbation changes no output (test bug)"
    assert torch.equal(got_map.cpu(), want_map.cpu()), \
        f"{what}: {int(got_map.sum())} mismatches, {int(want_map.sum())} expected, or at other outputs"


def assert_same_with_nan(got, ref, what):
    """exact equality where ref holds a value; where ref is NaN (outside the domains) got must still be NaN"""
    got, ref = got.detach().double(), ref.to(got.device)
    hole = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), hole), f"{what}: {int((torch.isnan(got) != hole).sum())} elements written outside " \
                                                f"the domains or left unwritten inside"
    X.assert_exact(torch.where(hole, torch.zeros_like(got), got), torch.where(hole, torch.zeros_like(ref), ref), what)


def assert_bounded_with_nan(got, ref, mag, c, what):
    got, ref, mag = got.detach().double(), ref.to(got.device), mag.to(got.device)
    hole = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), hole), f"{what}: written outside the domains or left unwritten inside"
    z = torch.zeros_like(got)
    G.assert_bounded(torch.where(hole, z, got), torch.where(hole, z, ref), torch.where(hole, z, mag), c, what)


# ============================================================================ 1. covariance pooling
def cov_geometry(M):
    """covpool_parts and the slab length: parts = clamp(ceil(M / 512), 1, 64), per = ceil(M / parts) rounded up to 64"""
    parts = max(1, min(64, -(-M // 512)))
    per = -(-(-(-M // parts)) // 64) * 64
    return parts, per


def cov_depth(M):
    """a thread adds its slab's pixels in order (per), sisr_sum_partials adds ceil(parts / 16) slabs per lane group and the
    16 groups in order"""
    parts, per = cov_geometry(M)
    return min(per, M) + -(-parts // 16) + 16


def cov_sentinel_pixels(M):
    """first and last pixel of every slab and of every 64-pixel LDS round inside it"""
    parts, per = cov_geometry(M)
    px = set()
    for s in range(parts):
        p0, p1 = s * per, min(M, (s + 1) * per)
        for q in range(p0, p1, 64):
            px.update((q, min(q + 63, p1 - 1)))
    return sorted(px)


def cov_data(B, M, seed):
    """integers in [-2, 2]; every sentinel pixel holds +-SENT in two channels that move with the pixel (all 64 channels at
    SENT would take the pixel sum of a 33000-pixel map over the exact-data budget); mean: dyadic k / 4"""
    x = X.ints((B, M, 64), seed)
    px = cov_sentinel_pixels(M)
    sign = X.nonzero_ints((B, len(px), 2), seed + 1, 1)
    for k, p in enumerate(px):
        x[:, p, k % 64] = SENT * sign[:, k, 0]
        x[:, p, (7 * k + 13) % 64] = SENT * sign[:, k, 1]
    return x, X.shifts((B, 64), seed + 2)


def cov_run(x, mean):
    B, M, _ = x.shape
    L = lib()
    nb = L.sisr_covpool_workspace_bytes(B, M)
    assert nb == B * cov_geometry(M)[0] * 64 * 64 * 4
    ws, cov = nan(nb // 4), nan(B, 64, 64)
    ok(L.sisr_covpool_fwd(P(x), P(mean), P(cov), P(ws), B, M, 64, St()), "sisr_covpool_fwd")
    return cov, ws.view(B, -1, 64 * 64)


def cov_exact(x, mean):
    """the exact pixel sum (budget-checked) times fl32(1 / M), rounded once: computed in fp32 on the CPU"""
    M = x.shape[1]
    X.assert_budget(S.covpool_ref(dd(x), dd(mean), A=True) * M, X.granule(x) * X.granule(mean), f"covariance sum, M = {M}")
    s = S.covpool_sum_ref(dd(x), dd(mean))
    s32 = s.float().cpu()
    assert torch.equal(s32.double(), s.cpu()), "test bug: the exact sum is not an fp32 value"
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(M), dtype=torch.float32)
    return (s32 * inv).double()


COV_M = [1, 63, 64, 65, 512, 513, 577, 1024, 32768, 33000]


def test_cov_cases_cover_the_slab_rules():
    assert cov_geometry(512) == (1, 512) and cov_geometry(513) == (2, 320) and cov_geometry(32768) == (64, 512)
    parts, per = cov_geometry(33000)
    assert (parts, per) == (64, 576) and 57 * per < 33000 <= 58 * per  # slabs 58 .. 63 are empty


@pytest.mark.parametrize("M", COV_M)
def test_covpool_exact(M):
    B = 2 if M <= 1024 else 1
    x, mean = cov_data(B, M, seed=100 + M)
    want = cov_exact(x, mean)
    cov, ws = cov_run(dev(x), dev(mean))
    X.assert_exact(cov, want, f"cov, M = {M}")
    parts, per = cov_geometry(M)
    first_empty = -(-M // per)
    assert not bool(ws.isnan().any()), "a slab partial was not written"
    assert bool((ws[:, first_empty:] == 0).all()), "an empty slab's partial is not zero"


@pytest.mark.parametrize("B,M", [(2, 120), (1, 577), (1, 16384), (1, 33000)])
def test_covpool_gaussian(B, M):
    """a = x - mean (one rounding), the product (one), D additions, the slab sum scaled by fl(1 / M) (two) -> c = D + 4"""
    g = torch.Generator().manual_seed(M)
    x = torch.randn(B, M, 64, generator=g) + 0.7
    mean = x.double().mean(1).float()
    cov, _ = cov_run(dev(x), dev(mean))
    G.assert_bounded(cov, S.covpool_ref(dd(x), dd(mean)), S.covpool_ref(dd(x), dd(mean), A=True), cov_depth(M) + 4, "cov")


@pytest.mark.parametrize("M", [577, 33000])
def test_covpool_detector(M):
    """the last slab's last-round sentinel negated in the kernel's copy: cov mismatches in its row and column only"""
    x, mean = cov_data(1, M, seed=7)
    px = cov_sentinel_pixels(M)
    k = len(px) - 2
    p, c = px[k], k % 64
    assert abs(float(x[0, p, c])) == SENT
    xp = x.clone()
    xp[0, p, c] = -x[0, p, c]
    base, moved = cov_exact(x, mean), cov_exact(xp, mean)
    want = moved != base
    rc = torch.zeros(64, 64, dtype=torch.bool)
    rc[c, :] = rc[:, c] = True
    assert not bool((want[0] & ~rc).any())
    cov, _ = cov_run(dev(xp), dev(mean))
    expect_detected(X.mismatch(cov, base), want, "covpool")


# ============================================================================ 2. SOCA input gradient
def soca_run(dy, gate, x, mean, dsym):
    B, M, _ = x.shape
    dx = nan(B, M, 64)
    ok(lib().sisr_soca_bwd_apply(P(dy), P(gate), P(x), P(mean), P(dsym), P(dx), B, M, 64, St()), "sisr_soca_bwd_apply")
    return dx


def soca_exact_data(B, M, seed):
    s = X.weights((B, 64, 64), seed)
    dsym = s + s.transpose(1, 2)
    return (X.ints((B, M, 64), seed + 1), X.scales((B, 64), seed + 2), X.ints((B, M, 64), seed + 3), X.shifts((B, 64), seed + 4),
            dsym)


@pytest.mark.parametrize("M", [1, 32, 64, 512, 1024, 2048])
def test_soca_bwd_apply_exact(M):
    """1 / M is a power of two: S = dsym / M, -(S mean), every product and the 64-term sums are exact on the budget"""
    dy, gate, x, mean, dsym = data = soca_exact_data(2, M, seed=200 + M)
    mag = S.soca_bwd_apply_ref(*map(dd, data), A=True)
    gran = min(X.granule(dsym) * X.granule(mean) * X.granule(x) / M, X.granule(dy) * X.granule(gate))
    X.assert_budget(mag, gran, f"SOCA dx, M = {M}")
    X.assert_exact(soca_run(*map(dev, data)), S.soca_bwd_apply_ref(*map(dd, data)), f"dx, M = {M}")


@pytest.mark.parametrize("M", [63, 65, 513, 577, 1100])
def test_soca_bwd_apply_bounded(M):
    """S = fl(fl(1 / M) dsym): 2; shift = -(S mean): 64 products added in order; the pixel's 64 products are added onto it
    in order: a term passes through at most 128 additions, one rounding for its product; dy gate + acc: 2
    -> c = 2 + 1 + 128 + 2 = 133"""
    g = torch.Generator().manual_seed(M)
    s = torch.randn(2, 64, 64, generator=g)
    data = (torch.randn(2, M, 64, generator=g), torch.rand(2, 64, generator=g), torch.randn(2, M, 64, generator=g) + 0.5,
            torch.randn(2, 64, generator=g) * 0.3 + 0.5, s + s.transpose(1, 2))
    G.assert_bounded(soca_run(*map(dev, data)), S.soca_bwd_apply_ref(*map(dd, data)),
                     S.soca_bwd_apply_ref(*map(dd, data), A=True), 133, f"dx, M = {M}")


def test_soca_bwd_apply_detector():
    """one x element of pixel 512 of a 1024-pixel map (the second workgroup's first pixel) moved: that pixel's dx
    mismatches in every channel whose dsym entry is nonzero, nothing else; one mean element moved: every pixel"""
    M = 1024
    dy, gate, x, mean, dsym = data = soca_exact_data(1, M, seed=9)
    base = S.soca_bwd_apply_ref(*map(dd, data))
    p = 512
    xp = x.clone()
    xp[0, p, 17] += 1.0
    moved = S.soca_bwd_apply_ref(dd(dy), dd(gate), dd(xp), dd(mean), dd(dsym))
    want = moved != base
    assert not bool(want[0, :p].any()) and not bool(want[0, p + 1:].any())
    expect_detected(X.mismatch(soca_run(dev(dy), dev(gate), dev(xp), dev(mean), dev(dsym)), base), want, "SOCA dx (x)")
    mp = mean.clone()
    mp[0, 3] += 0.25
    want = S.soca_bwd_apply_ref(dd(dy), dd(gate), dd(x), dd(mp), dd(dsym)) != base
    expect_detected(X.mismatch(soca_run(dev(dy), dev(gate), dev(x), dev(mp), dev(dsym)), base), want, "SOCA dx (mean)")


# ============================================================================ 3. projections 64 -> 24
def proj_params(seed):
    """w_theta, b_theta, w_phi, b_phi, w_g, b_g: k / 8, weights nonzero"""
    return tuple(X.weights((8, 64), seed + i, nonzero=True) if i % 2 == 0 else X.biases(8, seed + i) for i in range(6))


def proj_fwd_run(x, prm):
    npix = x.shape[0]
    proj = nan(npix, 24)
    ok(lib().sisr_nl_project_fwd(P(x), *[P(t) for t in prm], P(proj), npix, St()), "sisr_nl_project_fwd")
    return proj


def proj_bwd_run(x, dproj, dz, prm):
    npix = x.shape[0]
    L = lib()
    parts = L.sisr_nl_project_bwd_parts(npix)
    assert parts == 4 * max(1, min(256, -(-npix // 2048)))
    dx, part, pg = nan(npix, 64), nan(parts, 33, 64), nan(33, 64)
    ok(L.sisr_nl_project_bwd(P(x), P(dproj), P(dz), P(prm[0]), P(prm[2]), P(prm[4]), P(dx), P(part), npix, St()),
       "sisr_nl_project_bwd")
    ok(L.sisr_sum_partials(P(part), parts, 1, 33 * 64, 1.0, P(pg), St()), "sisr_sum_partials")
    return dx, part, pg


PROJ_NPIX = [4, 31, 32, 33, 127, 129, 2047, 2049, 16386, 131105]


def test_proj_cases_cover_the_grid_rules():
    assert -(-16386 // 2048) == 9  # past 8 wgrad blocks
    assert -(-131105 // 32) > 1024 * 4  # more 32-pixel tiles than the capped forward grid has waves


@pytest.mark.parametrize("npix", PROJ_NPIX)
def test_project_exact(npix):
    prm = proj_params(300)
    x, dproj, dz = X.ints((npix, 64), 301 + npix), X.ints((npix, 24), 302 + npix), X.ints((npix, 64), 303 + npix)
    dprm = [dev(t) for t in prm]
    X.assert_budget(S.project_fwd_ref(dd(x), *map(dd, prm), A=True), 1 / 8, "projection")
    X.assert_exact(proj_fwd_run(dev(x), dprm), S.project_fwd_ref(dd(x), *map(dd, prm)), f"proj, npix = {npix}")
    ws = (prm[0], prm[2], prm[4])
    X.assert_budget(S.project_dgrad_ref(dd(dproj), dd(dz), *map(dd, ws), A=True), 1 / 8, "projection dgrad")
    wmag = S.project_wgrad_ref(dd(x), dd(dproj), A=True)
    X.assert_budget(wmag["dW"], 1.0, "projection wgrad")
    X.assert_budget(wmag["db"], 1.0, "projection bias gradient")
    dx, part, pg = proj_bwd_run(dev(x), dev(dproj), dev(dz), dprm)
    X.assert_exact(dx, S.project_dgrad_ref(dd(dproj), dd(dz), *map(dd, ws)), f"dx, npix = {npix}")
    ref = S.project_wgrad_ref(dd(x), dd(dproj))
    X.assert_exact(pg[:24], ref["dW"], f"dWp, npix = {npix}")
    X.assert_exact(pg[32, :24], ref["db"], f"dbp, npix = {npix}")
    assert not bool(part.isnan().any()), "a wave's partial was not written"
    assert bool((part[:, 24:32] == 0).all()) and bool((part[:, 32, 24:] == 0).all()), "padding rows of the partials"
    assert bool((pg[24:32] == 0).all()) and bool((pg[32, 24:] == 0).all())


def test_project_detector():
    """one x element of the map's last pixel (the second tile of its wave at 131105 pixels) moved: proj mismatches in that
    pixel's 24 outputs, dWp in that channel's column where dproj is nonzero; one dproj element moved: that pixel's dx row,
    one dWp row and one bias sum"""
    npix = 131105
    prm = proj_params(300)
    dprm = [dev(t) for t in prm]
    ws = [dd(prm[0]), dd(prm[2]), dd(prm[4])]
    x, dproj, dz = X.ints((npix, 64), 5), X.nonzero_ints((npix, 24), 6), X.ints((npix, 64), 7)
    xp = x.clone()
    xp[npix - 1, 40] += 1.0
    base = S.project_fwd_ref(dd(x), *map(dd, prm))
    want = S.project_fwd_ref(dd(xp), *map(dd, prm)) != base
    assert int(want.sum()) == 24 and bool(want[npix - 1].all())
    expect_detected(X.mismatch(proj_fwd_run(dev(xp), dprm), base), want, "proj")
    wbase = S.project_wgrad_ref(dd(x), dd(dproj))
    _, _, pg = proj_bwd_run(dev(xp), dev(dproj), dev(dz), dprm)
    want = S.project_wgrad_ref(dd(xp), dd(dproj))["dW"] != wbase["dW"]
    assert int(want.sum()) == 24 and bool(want[:, 40].all())
    expect_detected(X.mismatch(pg[:24], wbase["dW"]), want, "dWp")
    dp = dproj.clone()
    dp[npix - 1, 23] += 1.0
    dbase = S.project_dgrad_ref(dd(dproj), dd(dz), *ws)
    dx, _, pg = proj_bwd_run(dev(x), dev(dp), dev(dz), dprm)
    expect_detected(X.mismatch(dx, dbase), S.project_dgrad_ref(dd(dp), dd(dz), *ws) != dbase, "dx")
    moved = S.project_wgrad_ref(dd(x), dd(dp))
    expect_detected(X.mismatch(pg[32, :24], wbase["db"]), moved["db"] != wbase["db"], "dbp")
    expect_detected(X.mismatch(pg[:24], wbase["dW"]), moved["dW"] != wbase["dW"], "dWp (dproj)")


# ============================================================================ 4. split / pool and the scatter
def quadrants(B, H, W):
    h1, w1 = H // 2, W // 2
    return [(B, H, W, y0, x0, hq, wq, 1, 1) for y0, hq in ((0, h1), (h1, H - h1)) for x0, wq in ((0, w1), (w1, W - w1))]


# B, H, W, y0, x0, hq, wq, nqy, nqx: a whole odd map; the 2x2 quadrant group of an even map; the four unequal quadrants of
# 5x7 and 37x51; the minimum 2x2 domain (nk = 1), alone and inside a map
SPLIT_DOMAINS = ([(2, 5, 7, 0, 0, 5, 7, 1, 1), (2, 6, 8, 0, 0, 3, 4, 2, 2), (1, 8, 12, 0, 0, 4, 6, 2, 2)] + quadrants(2, 5, 7) +
                 quadrants(1, 37, 51) + [(1, 2, 2, 0, 0, 2, 2, 1, 1), (2, 5, 7, 3, 4, 2, 2, 1, 1)])


def split_fwd_run(proj, dom):
    nd, nq, nk = dom[0] * dom[7] * dom[8], dom[5] * dom[6], (dom[5] // 2) * (dom[6] // 2)
    theta, phi, g = nan(nd, nq, 8), nan(nd, nk, 8), nan(nd, nk, 8)
    ok(lib().sisr_nl_split_pool_fwd(P(proj), P(theta), P(phi), P(g), cdom(dom), St()), "sisr_nl_split_pool_fwd")
    return theta, phi, g


def split_bwd_run(proj, dtheta, dphi, dg, dom):
    dproj = nan(dom[0] * dom[1] * dom[2], 24)
    ok(lib().sisr_nl_split_pool_bwd(P(proj), P(dtheta), P(dphi), P(dg), P(dproj), cdom(dom), St()), "sisr_nl_split_pool_bwd")
    return dproj


def split_grads(dom, seed):
    nd, nq, nk = dom[0] * dom[7] * dom[8], dom[5] * dom[6], (dom[5] // 2) * (dom[6] // 2)
    return X.nonzero_ints((nd, nq, 8), seed), X.nonzero_ints((nd, nk, 8), seed + 1), X.nonzero_ints((nd, nk, 8), seed + 2)


@pytest.mark.parametrize("dom", SPLIT_DOMAINS)
def test_split_pool_moves_values_and_routes_ties_to_the_first_maximum(dom):
    npix = dom[0] * dom[1] * dom[2]
    proj = S.tie_values((npix, 24), seed=sum(dom))
    if dom[5] * dom[6] >= 12:
        counts, mixed = S.tie_census(proj, dom)
        assert all(c > 0 for c in counts) and mixed > 0, (counts, mixed)
    ref = S.split_pool_fwd_ref(proj, dom)
    for name, got in zip(("theta", "phi", "g"), split_fwd_run(dev(proj), dom)):
        X.assert_exact(got, ref[name], name)
    dth, dph, dg = split_grads(dom, 400)
    dproj = split_bwd_run(dev(proj), dev(dth), dev(dph), dev(dg), dom)
    assert_same_with_nan(dproj, S.split_pool_bwd_ref(proj, dth, dph, dg, dom, npix), "dproj")


def test_split_pool_flat_region_routes_to_the_window_origin():
    """a constant map: every window a four-way tie, the whole gradient lands on member (0, 0)"""
    dom = (1, 6, 6, 0, 0, 6, 6, 1, 1)
    proj = torch.full((36, 24), 0.5)
    dth, dph, dg = split_grads(dom, 410)
    dproj = split_bwd_run(dev(proj), dev(dth), dev(dph), dev(dg), dom).cpu().view(6, 6, 24)
    want = torch.zeros(6, 6, 16)
    want[0::2, 0::2] = torch.cat([dph, dg], -1).view(3, 3, 16)
    assert torch.equal(dproj[..., 8:], want) and torch.equal(dproj[..., :8], dth.view(6, 6, 8))


def test_split_pool_detector():
    """one pooled-channel element raised above its window in the kernel's copy: phi mismatches at that window and channel,
    dproj at the two window members the gradient moves between"""
    dom = (2, 6, 8, 0, 0, 3, 4, 2, 2)
    npix = 96
    proj = S.tie_values((npix, 24), seed=sum(dom))
    pix = S.domain_pixels(dom)
    _, arg = S._first_max(S._windows(proj[pix.reshape(-1)].view(8, 3, 4, 24)[..., 8:], 3, 4))
    d, wy, wx, ch = [int(v) for v in (arg != 3).nonzero()[-1]]
    pp = proj.clone()
    pp[pix[d, 2 * wy + 1, 2 * wx + 1], 8 + ch] = 5.0
    base, moved = S.split_pool_fwd_ref(proj, dom), S.split_pool_fwd_ref(pp, dom)
    theta, phi, g = split_fwd_run(dev(pp), dom)
    X.assert_exact(theta, base["theta"], "theta")
    got = torch.cat([X.mismatch(phi, base["phi"]), X.mismatch(g, base["g"])], -1)
    want = torch.cat([moved["phi"] != base["phi"], moved["g"] != base["g"]], -1)
    assert int(want.sum()) == 1
    expect_detected(got, want, "phi | g")
    dth, dph, dg = split_grads(dom, 420)
    b = S.split_pool_bwd_ref(proj, dth, dph, dg, dom, npix, fill=0.0)
    want = S.split_pool_bwd_ref(pp, dth, dph, dg, dom, npix, fill=0.0) != b
    assert int(want.sum()) == 2
    expect_detected(X.mismatch(split_bwd_run(dev(pp), dev(dth), dev(dph), dev(dg), dom), b), want, "dproj")


# ============================================================================ 5. output projection 8 -> 64 + skip
# rows = B nqy nqx hq wq in {4, 15, 16, 18, 34, 511, 513, 1029} (17 is prime: see the module docstring), domains inside maps
OUT_DOMAINS = [(1, 3, 4, 1, 1, 2, 2, 1, 1), (1, 4, 6, 1, 1, 3, 5, 1, 1), (1, 4, 4, 0, 0, 2, 2, 2, 2), (1, 3, 7, 0, 1, 3, 6, 1, 1),
               (1, 2, 17, 0, 0, 2, 17, 1, 1), (1, 8, 73, 1, 0, 7, 73, 1, 1), (1, 27, 20, 0, 1, 27, 19, 1, 1),
               (3, 7, 50, 0, 1, 7, 49, 1, 1)]


def out_rows(dom):
    return dom[0] * dom[7] * dom[8] * dom[5] * dom[6]


def test_output_cases_cover_the_row_counts():
    assert [out_rows(d) for d in OUT_DOMAINS] == [4, 15, 16, 18, 34, 511, 513, 1029]


def out_fwd_run(y, x, w, bias, dom):
    z = nan(*x.shape)
    ok(lib().sisr_nl_output_fwd(P(y), P(x), P(w), P(bias), P(z), cdom(dom), St()), "sisr_nl_output_fwd")
    return z


def out_bwd_run(dz, y, w, dom):
    L = lib()
    parts = L.sisr_nl_output_bwd_parts(cdom(dom))
    assert parts == max(1, min(256, -(-out_rows(dom) // 512)))
    dy, part, out = nan(out_rows(dom), 8), nan(parts, 576), nan(576)
    ok(L.sisr_nl_output_bwd(P(dz), P(y), P(w), P(dy), P(part), cdom(dom), St()), "sisr_nl_output_bwd")
    ok(L.sisr_sum_partials(P(part), parts, 1, 576, 1.0, P(out), St()), "sisr_sum_partials")
    return dy, out[:512].view(64, 8), out[512:], part


def out_dz(dz, dom):
    """the cotangent with NaN at every pixel outside the domains: the backward must not read there"""
    inside = torch.zeros(dz.shape[0], dtype=torch.bool)
    inside[S.domain_pixels(dom).reshape(-1)] = True
    return torch.where(inside[:, None], dz, torch.full_like(dz, NAN))


def out_depth(dom):
    """dW / db: a thread adds its `rounds` pixels in order, the block its 16 slots in order, sisr_sum_partials
    ceil(parts / 16) blocks per lane group and the 16 groups in order"""
    parts = max(1, min(256, -(-out_rows(dom) // 512)))
    return -(-out_rows(dom) // (parts * 16)) + 16 + -(-parts // 16) + 16


@pytest.mark.parametrize("dom", OUT_DOMAINS)
def test_output_exact(dom):
    npix, rows = dom[0] * dom[1] * dom[2], out_rows(dom)
    y, x, w, bias = X.ints((rows, 8), 500 + rows), X.ints((npix, 64), 501 + rows), X.weights((64, 8), 502, nonzero=True), X.biases(64, 503)
    dz = X.ints((npix, 64), 504 + rows)
    mag = S.output_fwd_ref(dd(y), dd(x), dd(w), dd(bias), dom, A=True, fill=0.0)
    X.assert_budget(mag, 1 / 8, "output projection")
    assert_same_with_nan(out_fwd_run(dev(y), dev(x), dev(w), dev(bias), dom), S.output_fwd_ref(dd(y), dd(x), dd(w), dd(bias), dom), "z")
    bm = S.output_bwd_ref(dd(dz), dd(y), dd(w), dom, A=True)
    X.assert_budget(bm["dy"], 1 / 8, "dy")
    X.assert_budget(bm["dW"], 1.0, "dW")
    ref = S.output_bwd_ref(dd(dz), dd(y), dd(w), dom)
    dy, dW, db, part = out_bwd_run(dev(out_dz(dz, dom)), dev(y), dev(w), dom)
    X.assert_exact(dy, ref["dy"], "dy")
    X.assert_exact(dW, ref["dW"], "dW")
    X.assert_exact(db, ref["db"], "db")
    assert not bool(part.isnan().any())


@pytest.mark.parametrize("dom", OUT_DOMAINS)
def test_output_gaussian(dom):
    """z: 8 products added in order, + bias, + x, one rounding per product -> c = 8 + 2 + 1 = 11.
    dy: a lane's 4 products (4 additions), the 4-level xor tree, the products' rounding -> c = 9.
    dW, db: depth D (out_depth) plus the product -> c = D + 1."""
    npix, rows = dom[0] * dom[1] * dom[2], out_rows(dom)
    g = torch.Generator().manual_seed(rows)
    y, x, w, bias = (torch.randn(rows, 8, generator=g), torch.randn(npix, 64, generator=g), torch.randn(64, 8, generator=g) * 0.3,
                     torch.randn(64, generator=g))
    dz = torch.randn(npix, 64, generator=g)
    args = (dd(y), dd(x), dd(w), dd(bias), dom)
    assert_bounded_with_nan(out_fwd_run(dev(y), dev(x), dev(w), dev(bias), dom), S.output_fwd_ref(*args),
                            S.output_fwd_ref(*args, A=True), 11, "z")
    ref, mag = S.output_bwd_ref(dd(dz), dd(y), dd(w), dom), S.output_bwd_ref(dd(dz), dd(y), dd(w), dom, A=True)
    dy, dW, db, _ = out_bwd_run(dev(out_dz(dz, dom)), dev(y), dev(w), dom)
    D = out_depth(dom)
    G.assert_bounded(dy, ref["dy"], mag["dy"], 9, "dy")
    G.assert_bounded(dW, ref["dW"], mag["dW"], D + 1, "dW")
    G.assert_bounded(db, ref["db"], mag["db"], D + 1, "db")


def test_output_detector():
    """one y element of the last row (the third workgroup's) moved: z mismatches in that pixel's 64 channels, dW in column k
    where dz is nonzero; one dz element moved: dy of that row, one dW row, one db entry"""
    dom = OUT_DOMAINS[-1]
    npix, rows = dom[0] * dom[1] * dom[2], out_rows(dom)
    y, x, w, bias = X.ints((rows, 8), 1), X.ints((npix, 64), 2), X.weights((64, 8), 3, nonzero=True), X.biases(64, 4)
    dz = X.nonzero_ints((npix, 64), 5)
    yp = y.clone()
    yp[rows - 1, 6] += 1.0
    base = S.output_fwd_ref(dd(y), dd(x), dd(w), dd(bias), dom, fill=0.0)
    want = S.output_fwd_ref(dd(yp), dd(x), dd(w), dd(bias), dom, fill=0.0) != base
    assert int(want.sum()) == 64
    z = out_fwd_run(dev(yp), dev(x), dev(w), dev(bias), dom)
    expect_detected(X.mismatch(torch.where(z.isnan(), torch.zeros_like(z), z), base), want, "z")
    b = S.output_bwd_ref(dd(dz), dd(y), dd(w), dom)
    _, dW, _, _ = out_bwd_run(dev(out_dz(dz, dom)), dev(yp), dev(w), dom)
    want = S.output_bwd_ref(dd(dz), dd(yp), dd(w), dom)["dW"] != b["dW"]
    assert int(want.sum()) == 64 and bool(want[:, 6].all())
    expect_detected(X.mismatch(dW, b["dW"]), want, "dW")
    p = int(S.domain_pixels(dom).reshape(-1)[rows - 1])
    dzp = dz.clone()
    dzp[p, 9] += 1.0
    m = S.output_bwd_ref(dd(dzp), dd(y), dd(w), dom)
    dy, dW, db, _ = out_bwd_run(dev(out_dz(dzp, dom)), dev(y), dev(w), dom)
    expect_detected(X.mismatch(dy, b["dy"]), m["dy"] != b["dy"], "dy")
    expect_detected(X.mismatch(dW, b["dW"]), m["dW"] != b["dW"], "dW (dz)")
    expect_detected(X.mismatch(db, b["db"]), m["db"] != b["db"], "db")


# ============================================================================ 6. attention
def attn_fwd_run(theta, phi, g):
    nb, nq, _ = theta.shape
    y, lse = nan(nb, nq, 8), nan(nb, nq)
    ok(lib().sisr_nl_attn_fwd(P(theta), P(phi), P(g), P(y), P(lse), nb, nq, phi.shape[1], 8, St()), "sisr_nl_attn_fwd")
    return y, lse


def attn_bwd_run(theta, phi, g, y, lse, dy):
    nb, nq, _ = theta.shape
    nk = phi.shape[1]
    dth, dph, dg, dsum = nan(nb, nq, 8), nan(nb, nk, 8), nan(nb, nk, 8), nan(nb, nq)
    ok(lib().sisr_nl_attn_bwd(P(theta), P(phi), P(g), P(y), P(lse), P(dy), P(dth), P(dph), P(dg), P(dsum), nb, nq, nk, 8, St()),
       "sisr_nl_attn_bwd")
    return dict(dtheta=dth, dphi=dph, dg=dg, dsum=dsum)


def selector_positions(nk, power_of_two=False):
    """the matching keys: 0, 511, 512 (both sides of the 512-key LDS chunk boundary) and nk - 1; power_of_two: key 1 joins a
    set of three"""
    pos = sorted({p for p in (0, 511, 512, nk - 1) if p < nk})
    if power_of_two and len(pos) == 3:
        pos = sorted(set(pos) | {1})
    return pos


def selector_data(nb, nq, nk, same_class, seed):
    """theta_i = 16 e_class(i); the matching keys hold 16 e_class, every other key 0, 16 e_6, 16 e_7 or -16 e_c: logits are
    256 on a match and 0 or -256 otherwise, and expf(-256) is 0 in fp32.  g, dy: integers in [-2, 2]"""
    pos = selector_positions(nk, same_class)
    gen = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, 4, (nb, nk), generator=gen)
    axis = torch.randint(0, 6, (nb, nk), generator=gen)
    phi = torch.zeros(nb, nk, 8)
    phi.scatter_(2, torch.where(kind == 3, axis, kind + 5)[..., None], torch.where(kind == 3, -16.0, 16.0)[..., None])
    phi[kind == 0] = 0.0
    cls_q = torch.zeros(nq, dtype=torch.long) if same_class else torch.arange(nq) % len(pos)
    theta = torch.zeros(nb, nq, 8)
    theta[:, torch.arange(nq), cls_q] = 16.0
    for c, p in enumerate(pos):
        phi[:, p] = 0.0
        phi[:, p, 0 if same_class else c] = 16.0
    logits = theta.double() @ phi.double().transpose(1, 2)
    assert set(logits.unique().tolist()) <= {-256.0, 0.0, 256.0}
    match = logits == 256.0
    assert bool((match.sum(-1) == (len(pos) if same_class else 1)).all())
    return theta, phi, X.ints((nb, nk, 8), seed + 1), X.ints((nb, nq, 8), seed + 2), match.double()


@pytest.mark.parametrize("nk", [1, 2, 3, 5, 511, 512, 513, 1025])
def test_attention_selector_exact(nk):
    """one matching key per query: y = g of that key, lse = 256, dtheta = dphi = 0, dg = the sum of dy over the key's
    queries, dsum = dy . y, all exact.  2^k matching keys: y = their mean, exact"""
    nb = 2
    for nq in (1, 255, 256, 257):
        theta, phi, g, dy, match = selector_data(nb, nq, nk, False, seed=600 + nk + nq)
        y_ref = match @ g.double()
        X.assert_budget(match.transpose(1, 2) @ dy.double().abs(), 1.0, "dg")
        y, lse = attn_fwd_run(dev(theta), dev(phi), dev(g))
        X.assert_exact(y, y_ref, f"y, nq = {nq}, nk = {nk}")
        X.assert_exact(lse, torch.full((nb, nq), 256.0, dtype=torch.float64), f"lse, nq = {nq}, nk = {nk}")
        b = attn_bwd_run(dev(theta), dev(phi), dev(g), y, lse, dev(dy))
        X.assert_exact(b["dtheta"], torch.zeros(nb, nq, 8, dtype=torch.float64), "dtheta")
        X.assert_exact(b["dphi"], torch.zeros(nb, nk, 8, dtype=torch.float64), "dphi")
        X.assert_exact(b["dg"], match.transpose(1, 2) @ dy.double(), f"dg, nq = {nq}, nk = {nk}")
        X.assert_exact(b["dsum"], (dy.double() * y_ref).sum(-1), "dsum")
        if nk > 1:
            theta, phi, g, dy, match = selector_data(nb, nq, nk, True, seed=700 + nk + nq)
            n = int(match[0, 0].sum())
            assert n in (2, 4)
            y, lse = attn_fwd_run(dev(theta), dev(phi), dev(g))
            X.assert_exact(y, match @ g.double() / n, f"y ({n} matching keys), nq = {nq}, nk = {nk}")
            # lse = 256 + log n: logf within 2 ulp of 1.39 and the sum's rounding at 257 stay under 2 * 2^-24 * 512
            assert float((lse.double().cpu() - (256.0 + math.log(n))).abs().max()) <= 2 * U * 512


def test_attention_selector_detector():
    """one g element of the key at the chunk boundary moved in the kernel's copy: y mismatches at exactly the queries that
    select it, in that channel; one dy element moved: dg of the selected key and dsum of that query"""
    nb, nq, nk = 2, 257, 1025
    theta, phi, g, dy, match = selector_data(nb, nq, nk, False, seed=11)
    gp = g.clone()
    gp[1, 512, 3] += 1.0
    base = match @ g.double()
    want = (match @ gp.double()) != base
    assert 0 < int(want.sum()) == int(match[1, :, 512].sum())
    y, lse = attn_fwd_run(dev(theta), dev(phi), dev(gp))
    expect_detected(X.mismatch(y, base), want, "y")
    y, lse = attn_fwd_run(dev(theta), dev(phi), dev(g))
    dyp = dy.clone()
    dyp[0, 256, int(base[0, 256].nonzero()[0])] += 1.0  # a channel whose y is nonzero, so dsum moves too
    b = attn_bwd_run(dev(theta), dev(phi), dev(g), y, lse, dev(dyp))
    dg_base = match.transpose(1, 2) @ dy.double()
    want = (match.transpose(1, 2) @ dyp.double()) != dg_base
    assert int(want.sum()) == 1
    expect_detected(X.mismatch(b["dg"], dg_base), want, "dg")
    ds_base = (dy.double() * base).sum(-1)
    expect_detected(X.mismatch(b["dsum"], ds_base), (dyp.double() * base).sum(-1) != ds_base, "dsum")


# ============================================================================ 7. the chains
def chain_terms(got, ref64, ref32):
    """per sample: err = max|got - ref64|, scale = max(E32, floor) with E32 = max|ref32 - ref64| and floor = 2 * 2^-24 *
    max|ref64|; the bar is 8 * scale.  An unwritten (NaN) element makes err NaN, which fails every comparison"""
    B = ref64.shape[0]
    g, r, r32 = (t.detach().double().cpu().reshape(B, -1) for t in (got, ref64, ref32))
    err = (g - r).abs().max(1)[0]
    err = torch.where(torch.isnan(g).any(1), torch.full_like(err, NAN), err)
    scale = torch.maximum((r32 - r).abs().max(1)[0], CHAIN_FLOOR * U * r.abs().max(1)[0])
    return err, scale


def chain_check(got, ref64, ref32, what, case, ratios):
    err, scale = chain_terms(got, ref64, ref32)
    ratio = err / scale
    worst = float(ratio.max()) if not bool(torch.isnan(ratio).any()) else NAN
    ratios[what] = max(ratios.get(what, 0.0), worst) if worst == worst else NAN
    print(f"chain {case} {what}: err / max(E32, floor) per sample = {[round(float(v), 3) for v in ratio]}")
    assert bool((err <= CHAIN_FACTOR * scale).all()), \
        f"{case} {what}: err {err.tolist()} over 8 * max(E32, floor) = {(CHAIN_FACTOR * scale).tolist()}"


def chain_fails(got, ref64, ref32):
    err, scale = chain_terms(got, ref64, ref32)
    return not bool((err <= CHAIN_FACTOR * scale).all())


def sqrtm_fwd_run(cov, iters):
    B = cov.shape[0]
    n = lib().sisr_sqrtm_saved_bytes(B, 64, iters) // 4
    k = iters - 1
    assert n == B * (4 + (2 * k + 1) * 4096)
    saved, pooled = nan(n), nan(B, 64)
    ok(lib().sisr_sqrtm_fwd(P(cov), P(saved), P(pooled), B, 64, iters, St()), "sisr_sqrtm_fwd")
    sv = saved.view(B, -1)
    assert bool((sv[:, 1:4] == 0).all())
    out = dict(trace=sv[:, 0], Y=sv[:, 4:4 + k * 4096].view(B, k, 64, 64), Z=sv[:, 4 + k * 4096:4 + 2 * k * 4096].view(B, k, 64, 64),
               last=sv[:, 4 + 2 * k * 4096:].view(B, 64, 64), pooled=pooled)
    return out, saved


def sqrtm_bwd_run(cov, saved, dpooled, iters):
    dsym = nan(*cov.shape)
    ok(lib().sisr_sqrtm_bwd(P(cov), P(saved), P(dpooled), P(dsym), cov.shape[0], 64, iters, St()), "sisr_sqrtm_bwd")
    return dsym


def sqrtm_cov(B, M, r, seed):
    """the fp32 covariance of a seeded map (float64 pooling, rounded once): the kernels and both references take it as is"""
    x = S.correlated_maps(B, M, r, 0.01 + 0.04 * ((seed % 5) / 4), seed).double()
    return S.covpool_ref(x, x.mean(1)).float()


def sqrtm_compare(cov, iters, dpooled, case, ratios):
    f64, f32 = S.sqrtm_fwd_ref(cov, iters), S.sqrtm_fwd_ref(cov, iters, dt=torch.float32)
    got, saved = sqrtm_fwd_run(dev(cov), iters)
    for name in ("trace", "pooled", "last"):
        chain_check(got[name], f64[name], f32[name], name, case, ratios)
    for i in range(iters - 1):
        chain_check(got["Y"][:, i], f64["Y"][:, i], f32["Y"][:, i], f"Y_{i}", case, ratios)
        chain_check(got["Z"][:, i], f64["Z"][:, i], f32["Z"][:, i], f"Z_{i}", case, ratios)
    dsym = sqrtm_bwd_run(dev(cov), saved, dev(dpooled), iters)
    chain_check(dsym, S.sqrtm_bwd_ref(cov, iters, dpooled), S.sqrtm_bwd_ref(cov, iters, dpooled, dt=torch.float32), "dsym", case,
                ratios)


SQRTM_RATIOS, ATTN_RATIOS = {}, {}


@pytest.mark.parametrize("iters", [2, 3, 5])
@pytest.mark.parametrize("H,W", [(3, 3), (13, 9), (20, 20)])
def test_sqrtm_chain(iters, H, W):
    """forward (trace, every saved Y_i / Z_i, last, the column means) and backward (G + G^T) at B in {1, 3}, isotropic and
    rank-2 / rank-8 correlated maps (a 3x3 map's covariance has rank <= 8 whatever the data)"""
    for B in (1, 3):
        for r in (None, 2, 8):
            cov = sqrtm_cov(B, H * W, r, seed=800 + iters + H + B)
            dpooled = torch.randn(B, 64, generator=torch.Generator().manual_seed(801 + B))
            sqrtm_compare(cov, iters, dpooled, f"sqrtm iters={iters} map={H}x{W} B={B} r={r}", SQRTM_RATIOS)
    print("sqrtm chain maxima so far:", {k: round(v, 3) for k, v in SQRTM_RATIOS.items()})


def smallest_detected_move(x, idx, ref_of, bars):
    """the smallest power of two that, added to x[idx], moves some sample's float64 output by more than 4x its bar"""
    base = ref_of(x)
    for e in range(-30, 12):
        xp = x.clone()
        xp[idx] += 2.0 ** e
        if bool(torch.equal(xp, x)):
            continue
        moved = (ref_of(xp) - base).abs().reshape(base.shape[0], -1).max(1)[0]
        if bool((moved > 4 * bars).any()):
            return xp, e
    raise AssertionError("test bug: no power-of-two move is large enough")


@pytest.mark.parametrize("iters", [2, 5])
def test_sqrtm_chain_detector(iters):
    """one off-diagonal covariance element moved in the kernel's copy: pooled (forward) and G + G^T (backward, fed the
    unperturbed saved state's own run) leave the bar"""
    cov = sqrtm_cov(2, 117, 8, seed=21)
    dpooled = torch.randn(2, 64, generator=torch.Generator().manual_seed(22))
    f64, f32 = S.sqrtm_fwd_ref(cov, iters), S.sqrtm_fwd_ref(cov, iters, dt=torch.float32)
    _, scale = chain_terms(f64["pooled"], f64["pooled"], f32["pooled"])
    covp, e = smallest_detected_move(cov, (1, 5, 9), lambda c: S.sqrtm_fwd_ref(c, iters)["pooled"], CHAIN_FACTOR * scale)
    got, saved = sqrtm_fwd_run(dev(covp), iters)
    assert chain_fails(got["pooled"], f64["pooled"], f32["pooled"]), f"pooled: a move of 2^{e} passes"
    b64, b32 = S.sqrtm_bwd_ref(cov, iters, dpooled), S.sqrtm_bwd_ref(cov, iters, dpooled, dt=torch.float32)
    _, scale = chain_terms(b64, b64, b32)
    covp, e = smallest_detected_move(cov, (1, 5, 9), lambda c: S.sqrtm_bwd_ref(c, iters, dpooled), CHAIN_FACTOR * scale)
    got, saved = sqrtm_fwd_run(dev(covp), iters)
    assert chain_fails(sqrtm_bwd_run(dev(covp), saved, dev(dpooled), iters), b64, b32), f"dsym: a move of 2^{e} passes"


ATTN_CASES = [(2, 30, 6), (3, 300, 77), (1, 1000, 513), (1, 257, 1025)]


def attn_data(nb, nq, nk, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(nb, nq, 8, generator=g) * scale, torch.randn(nb, nk, 8, generator=g), torch.randn(nb, nk, 8, generator=g),
            torch.randn(nb, nq, 8, generator=g))


@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("nb,nq,nk", ATTN_CASES)
def test_attention_chain(nb, nq, nk, scale):
    theta, phi, g, dy = attn_data(nb, nq, nk, scale, seed=900 + nq)
    case = f"attention nb={nb} nq={nq} nk={nk} scale={scale}"
    print(case, "max|logit| =", round(float((theta.double() @ phi.double().transpose(1, 2)).abs().max()), 1))
    f64, f32 = S.attn_fwd_ref(theta, phi, g), S.attn_fwd_ref(theta, phi, g, dt=torch.float32)
    y, lse = attn_fwd_run(dev(theta), dev(phi), dev(g))
    chain_check(y, f64["y"], f32["y"], "y", case, ATTN_RATIOS)
    chain_check(lse, f64["lse"], f32["lse"], "lse", case, ATTN_RATIOS)
    b64, b32 = S.attn_bwd_ref(theta, phi, g, dy), S.attn_bwd_ref(theta, phi, g, dy, dt=torch.float32)
    got = attn_bwd_run(dev(theta), dev(phi), dev(g), y, lse, dev(dy))
    for name in ("dtheta", "dphi", "dg", "dsum"):
        chain_check(got[name], b64[name], b32[name], name, case, ATTN_RATIOS)
    print("attention chain maxima so far:", {k: round(v, 3) for k, v in ATTN_RATIOS.items()})


def test_attention_chain_detector():
    """one phi element of the key behind the chunk boundary moved in the kernel's copy: y and dtheta leave the bar"""
    nb, nq, nk = 1, 257, 1025
    theta, phi, g, dy = attn_data(nb, nq, nk, 1.0, seed=31)
    f64, f32 = S.attn_fwd_ref(theta, phi, g), S.attn_fwd_ref(theta, phi, g, dt=torch.float32)
    _, scale = chain_terms(f64["y"], f64["y"], f32["y"])
    php, e = smallest_detected_move(phi, (0, 512, 4), lambda p: S.attn_fwd_ref(theta, p, g)["y"], CHAIN_FACTOR * scale)
    y, lse = attn_fwd_run(dev(theta), dev(php), dev(g))
    assert chain_fails(y, f64["y"], f32["y"]), f"y: a move of 2^{e} passes"
    b64, b32 = S.attn_bwd_ref(theta, phi, g, dy), S.attn_bwd_ref(theta, phi, g, dy, dt=torch.float32)
    _, scale = chain_terms(b64["dtheta"], b64["dtheta"], b32["dtheta"])
    php, e = smallest_detected_move(phi, (0, 512, 4), lambda p: S.attn_bwd_ref(theta, p, g, dy)["dtheta"], CHAIN_FACTOR * scale)
    y, lse = attn_fwd_run(dev(theta), dev(php), dev(g))
    got = attn_bwd_run(dev(theta), dev(php), dev(g), y, lse, dev(dy))
    assert chain_fails(got["dtheta"], b64["dtheta"], b32["dtheta"]), f"dtheta: a move of 2^{e} passes"


# ============================================================================ 8. refusals (all return before any launch)
def test_unsupported_sizes_are_refused():
    """channels != 64, dim != 8, iters 1 and 17: SISR_ERR_UNSUPPORTED"""
    L = lib()
    z = dev(torch.zeros(2 * 64 * 64 * 12))
    cov, ws, dx, pooled, saved, dsym = nan(4096), nan(4096), nan(4096), nan(64), nan(4 + 33 * 4096), nan(4096)
    for ch in (32, 128):
        assert L.sisr_covpool_fwd(P(z), P(z), P(cov), P(ws), 1, 64, ch, St()) == ERR_UNSUPPORTED
        assert L.sisr_soca_bwd_apply(P(z), P(z), P(z), P(z), P(z), P(dx), 1, 64, ch, St()) == ERR_UNSUPPORTED
        assert L.sisr_sqrtm_fwd(P(z), P(saved), P(pooled), 1, ch, 5, St()) == ERR_UNSUPPORTED
        assert L.sisr_sqrtm_bwd(P(z), P(z), P(z), P(dsym), 1, ch, 5, St()) == ERR_UNSUPPORTED
    for iters in (1, 17):
        assert L.sisr_sqrtm_fwd(P(z), P(saved), P(pooled), 1, 64, iters, St()) == ERR_UNSUPPORTED
        assert L.sisr_sqrtm_bwd(P(z), P(z), P(z), P(dsym), 1, 64, iters, St()) == ERR_UNSUPPORTED
    assert L.sisr_sqrtm_saved_bytes(1, 64, 1) == 0 and L.sisr_sqrtm_saved_bytes(1, 32, 5) == 0
    y, lse, o1, o2, o3, o4 = nan(64), nan(8), nan(64), nan(64), nan(64), nan(8)
    for dim in (4, 16):
        assert L.sisr_nl_attn_fwd(P(z), P(z), P(z), P(y), P(lse), 1, 4, 4, dim, St()) == ERR_UNSUPPORTED
        assert L.sisr_nl_attn_bwd(P(z), P(z), P(z), P(z), P(z), P(z), P(o1), P(o2), P(o3), P(o4), 1, 4, 4, dim, St()) == ERR_UNSUPPORTED
    assert untouched(cov, ws, dx, pooled, saved, dsym, y, lse, o1, o2, o3, o4)


@pytest.mark.parametrize("dom", [(1, 4, 4, 0, 0, 1, 4, 1, 1), (1, 4, 4, 0, 0, 4, 1, 1, 1), (1, 4, 4, 2, 0, 3, 4, 1, 1),
                                 (1, 4, 4, 0, 0, 2, 2, 2, 3), (1, 4, 4, 0, -1, 2, 2, 1, 1)])
def test_bad_domains_are_refused(dom):
    """hq = 1, wq = 1, a domain past the bottom or right edge, a negative offset: SISR_ERR_ARG"""
    L = lib()
    z = dev(torch.zeros(16 * 64))
    o = [nan(16 * 64) for _ in range(6)]
    assert L.sisr_nl_split_pool_fwd(P(z), P(o[0]), P(o[1]), P(o[2]), cdom(dom), St()) == ERR_ARG
    assert L.sisr_nl_split_pool_bwd(P(z), P(z), P(z), P(z), P(o[3]), cdom(dom), St()) == ERR_ARG
    assert L.sisr_nl_output_fwd(P(z), P(z), P(z), P(z), P(o[4]), cdom(dom), St()) == ERR_ARG
    assert L.sisr_nl_output_bwd(P(z), P(z), P(z), P(o[5]), P(o[0]), cdom(dom), St()) == ERR_ARG
    assert L.sisr_nl_output_bwd_parts(cdom(dom)) == 0
    assert untouched(*o)


def test_too_many_attention_domains_are_refused():
    """nb = 65536 is past the grid's y extent: SISR_ERR_ARG"""
    L = lib()
    z = dev(torch.zeros(64))
    o = [nan(64) for _ in range(6)]
    assert L.sisr_nl_attn_fwd(P(z), P(z), P(z), P(o[0]), P(o[1]), 65536, 1, 1, 8, St()) == ERR_ARG
    assert L.sisr_nl_attn_bwd(P(z), P(z), P(z), P(z), P(z), P(z), P(o[2]), P(o[3]), P(o[4]), P(o[5]), 65536, 1, 1, 8, St()) == ERR_ARG
    assert L.sisr_nl_project_fwd(P(z), P(z), P(z), P(z), P(z), P(z), P(z), P(o[0]), 0, St()) == ERR_ARG
    assert L.sisr_nl_project_bwd_parts(0) == 0
    assert untouched(*o)


def test_misaligned_pointers_are_refused():
    """a pointer 4 bytes off a 16-byte boundary: SISR_ERR_ALIGN wherever the entry point reads or writes float4"""
    L = lib()
    buf = dev(torch.zeros(2 * 64 * 64 * 12 + 4))
    z, off = buf[4:], buf[1:]
    assert hip.ptr(z) % 16 == 0 and hip.ptr(off) % 16 == 4
    o = [nan(5 * 4096) for _ in range(6)]
    dom = cdom((1, 4, 4, 0, 0, 4, 4, 1, 1))
    assert L.sisr_covpool_fwd(P(off), P(z), P(o[0]), P(o[1]), 1, 64, 64, St()) == ERR_ALIGN
    assert L.sisr_covpool_fwd(P(z), P(off), P(o[0]), P(o[1]), 1, 64, 64, St()) == ERR_ALIGN
    assert L.sisr_sqrtm_fwd(P(off), P(o[0]), P(o[1]), 1, 64, 2, St()) == ERR_ALIGN
    assert L.sisr_sqrtm_bwd(P(off), P(z), P(z), P(o[0]), 1, 64, 2, St()) == ERR_ALIGN
    assert L.sisr_sqrtm_bwd(P(z), P(z), P(off), P(o[0]), 1, 64, 2, St()) == ERR_ALIGN
    assert L.sisr_soca_bwd_apply(P(off), P(z), P(z), P(z), P(z), P(o[0]), 1, 64, 64, St()) == ERR_ALIGN
    assert L.sisr_soca_bwd_apply(P(z), P(z), P(z), P(z), P(off), P(o[0]), 1, 64, 64, St()) == ERR_ALIGN
    assert L.sisr_nl_attn_fwd(P(off), P(z), P(z), P(o[0]), P(o[1]), 1, 4, 4, 8, St()) == ERR_ALIGN
    assert L.sisr_nl_attn_bwd(P(z), P(off), P(z), P(z), P(z), P(z), P(o[0]), P(o[1]), P(o[2]), P(o[3]), 1, 4, 4, 8, St()) == ERR_ALIGN
    assert L.sisr_nl_project_fwd(P(off), P(z), P(z), P(z), P(z), P(z), P(z), P(o[0]), 16, St()) == ERR_ALIGN
    assert L.sisr_nl_project_bwd(P(z), P(off), P(z), P(z), P(z), P(z), P(o[0]), P(o[1]), 16, St()) == ERR_ALIGN
    assert L.sisr_nl_split_pool_fwd(P(off), P(o[0]), P(o[1]), P(o[2]), dom, St()) == ERR_ALIGN
    assert L.sisr_nl_split_pool_bwd(P(z), P(off), P(z), P(z), P(o[0]), dom, St()) == ERR_ALIGN
    assert L.sisr_nl_output_fwd(P(off), P(z), P(z), P(z), P(o[0]), dom, St()) == ERR_ALIGN
    assert L.sisr_nl_output_bwd(P(off), P(z), P(z), P(o[0]), P(o[1]), dom, St()) == ERR_ALIGN
    assert untouched(*o)
