"""SPARNet's norm / activation / attention-product / geometry kernels (csrc/sparnet.hip) and HAN's LAM and CSAM
(csrc/han.hip) against float64 (pytest -m gpu).

The native entry points are called directly (shapes, null running buffers and refused arguments chosen freely), then once
through each ops wrapper.  References are tests/_spar_han.py (checked against PyTorch's and the oracle's autograd by
tests/test_spar_han_cpu.py).  Every output buffer starts as NaN, so an element the kernel never writes fails; padded
channels must come back exactly 0.  Two tiers:

1. Exact (zero tolerance) on dyadic data (tests/_exact.py), each sum preceded by a budget check: the geometry kernels and
   their adjoints, PReLU / LeakyReLU with a dyadic slope forward and backward and the slope gradient, the batch-norm
   mean (power-of-two pixel counts) and the backward's dbeta / dgamma at dyadic saved statistics (every chunk, partial and
   remainder of the partial-sum path shows there), the group-norm mean and per-sample dbeta / dgamma, the 1-channel
   attention product's backward at a dyadic attention.
2. Bounded.  Everything behind sqrt, exp or a division: |got - ref| <= c * 2^-24 * mag, mag the float64 computation on
   absolute values (`A=True`), c derived next to each test from the kernel's summation structure -- for the reductions a
   depth D: the longest chain of dependent fp32 additions any one term passes through (recursive summation errs by at most
   D * 2^-24 of the sum of magnitudes).

Each family has a detector: one input element moved in what the kernel sees only must make the exact comparison mismatch
at exactly the outputs it feeds, or make the bounded comparison fail.
"""
import collections
import math

import pytest
import torch

import _exact as X
import _gates as G
import _spar_han as S
import sisr_amd

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
hip = sisr_amd.hip
DEV = "cuda:0"
NAN = float("nan")
ERR_ARG, ERR_UNSUPPORTED = -1, -4
C_SIG = 8  # a sigmoid of an exact fp32 argument (expf, 1 + e, 1 / .): tests/test_gates_gpu.py
M32 = 0.10000000149011612  # float32(0.1): the momentum the kernels multiply by


def f32(v):
    """the fp32 value of a float argument"""
    return float(torch.tensor(v, dtype=torch.float32))


def lib():
    return hip.lib()


_LIVE = collections.deque(maxlen=64)


def P(t):
    """device pointer of t, which stays referenced over the next calls: a temporary made inside a call expression
    (P(dev(x)), P(dev(dy))) must not hand its freed block to the next temporary of the same call"""
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


def expect_detected(got_map, want_map, what):
    assert bool(want_map.any()), f"{what}: the perturbation changes no output (test bug)"
    assert torch.equal(got_map.cpu(), want_map.cpu()), \
        f"{what}: {int(got_map.sum())} mismatches, {int(want_map.sum())} expected, or at other outputs"


def padded(x_real, C):
    """[..., Cr] -> [..., C] with zero channels appended"""
    out = torch.zeros(x_real.shape[:-1] + (C,), dtype=x_real.dtype, device=x_real.device)
    out[..., :x_real.shape[-1]] = x_real
    return out


def nchw_view(t):
    """[B][H][W][C] (device) -> the NCHW channels-last view the ops wrappers take"""
    return t.permute(0, 3, 1, 2)


def rows_of(t):
    """NCHW -> [B * H * W][C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# ============================================================================ 1. batch norm + LeakyReLU
# sp_bn_geometry: rows = 1024 / C pixel lanes; nblk = min(256, ceil(npix / (rows * 8))), chunk = ceil(npix / nblk);
# npix <= 256 * 16 = 4096 takes the register-resident bn_small_* kernels instead.
def bn_geometry(npix, C):
    rows = 1024 // C
    nblk = max(1, min(256, -(-npix // (rows * 8))))
    return rows, nblk, -(-npix // nblk)


def bn_depth(npix, C):
    """the longest chain of dependent fp32 additions of a per-channel sum.  Small path: 16 pixels per thread, the xor tree
    (6 levels), 4 waves in order.  Partial path: ceil(chunk / rows) pixels per lane, rows lanes in order, then
    sp_sum_parts_wg: slice j adds partials j, j + J, ... (ceil(nblk / J)), the J = 256 / C slices in order."""
    if npix <= 4096:
        return 16 + 6 + 4
    rows, nblk, chunk = bn_geometry(npix, C)
    J = max(1, 256 // C)
    return -(-chunk // rows) + rows + -(-nblk // J) + J


def bn_sentinel_pixels(npix, C):
    """the first and last pixel of every chunk of the partial path (pixels 0 and npix - 1 on the small path)"""
    if npix <= 4096:
        return [0, npix - 1]
    _, nblk, chunk = bn_geometry(npix, C)
    px = set()
    for k in range(nblk):
        p0, p1 = k * chunk, min(npix, (k + 1) * chunk)
        if p0 < p1:
            px.update((p0, p1 - 1))
    return sorted(px | {npix - 1})


SENT = 32.0  # sentinel magnitude (inputs elsewhere are integers in [-2, 2])


def bn_data(npix, C, Cr, seed):
    """x [npix][C] (padded channels 0): nonzero integers in [-2, 2], +-SENT at every chunk's first and last pixel and at
    the map's last pixel (a sentinel dropped or double-counted moves the mean by SENT / npix and the variance by ~SENT^2 /
    npix: far outside every bound below)"""
    x = X.nonzero_ints((npix, Cr), seed, 2)
    px = torch.tensor(bn_sentinel_pixels(npix, C))
    x[px] = SENT * X.nonzero_ints((len(px), Cr), seed + 1, 1)
    return padded(x, C)


def bn_params(Cr, seed):
    return X.weights((Cr,), seed, nonzero=True), X.biases(Cr, seed + 1)


def bn_fwd_run(x, gamma, beta, C, Cr, training, slope, rm=None, rv=None, momentum=M32, eps=1e-5):
    npix = x.shape[0]
    L = lib()
    nb = L.sisr_bn_workspace_bytes(npix, C)
    ws = nan(nb // 4)
    y, mean, inv = nan(npix, C), nan(C), nan(C)
    ok(L.sisr_bn_act_fwd(P(x), P(y), P(gamma), P(beta), P(rm), P(rv), P(mean), P(inv), npix, C, Cr, int(training),
                         float(momentum), float(eps), float(slope), P(ws), nb, St()), "sisr_bn_act_fwd")
    return y, mean, inv


def bn_y_bound(x, g, b, mean, inv, slope):
    """y recomputed from the kernel's own statistics: sc = fl(g * inv), sh = fma(-mean, sc, b), z = fma(x, sc, sh), y = z or
    fl(z * slope): three roundings of magnitude <= |x sc| + |b| + |mean sc|, a fourth where a sign differs -> c = 4"""
    sc = (dd(g) * dd(inv)).float().double()
    z = dd(x) * sc + (dd(b) - dd(mean) * sc)
    ref = torch.where(z > 0, z, z * f32(slope))
    mag = (dd(x) * sc).abs() + dd(b).abs() + (dd(mean) * sc).abs()
    return ref, mag


def bn_y_direct_mag(x, ref, g, b):
    """y against float64 directly: the statistics' errors (mean D + 2 of mean|x|, invstd (D + 4) / 2 + 2) plus the apply's 4
    -> c = 1.5 D + 10 of (|x| + |mean| + mean|x|) invstd |g| + |b|"""
    xa = dd(x).abs()
    return (xa + ref["mean"].abs() + xa.mean(0)) * ref["invstd"] * dd(g).abs() + dd(b).abs()


# (B, H, W, C, C_real, slope): the rules -- npix 4096 (small) | 4097 (partial: nblk 33, not a multiple of 16; chunk 125,
# not a multiple of rows = 16); nblk 254 (below 256), 256 (at: 2 x 128^2), capped at 256 (16 x 128^2 wants 2048);
# C 64 / 128 / 192 (rows 5, J 1) / 256 (rows 4) with C_real < C; power-of-two npix (the exact mean) and not.
BN_CASES = [(1, 64, 64, 64, 48, 0.2), (1, 17, 241, 64, 64, 0.0), (2, 127, 128, 64, 40, 1.0), (2, 128, 128, 64, 42, 0.2),
            (16, 128, 128, 64, 64, 0.2), (1, 33, 40, 128, 100, 0.0), (1, 65, 67, 128, 96, 0.2), (1, 16, 16, 192, 150, 1.0),
            (1, 61, 83, 192, 150, 0.2), (1, 64, 128, 256, 200, 0.2), (3, 100, 100, 256, 256, 0.0), (1, 70, 70, 256, 255, 1.0)]


def test_bn_cases_sit_on_both_sides_of_every_rule():
    geo = [(B * H * W, C) for B, H, W, C, _, _ in BN_CASES]
    assert any(n == 4096 for n, _ in geo) and any(n == 4097 for n, _ in geo)
    nblks = [bn_geometry(n, C)[1] for n, C in geo if n > 4096]
    assert any(k < 256 for k in nblks) and 256 in nblks and any(-(-n // (1024 // C * 8)) > 256 for n, C in geo)
    assert any(bn_geometry(n, C)[2] % bn_geometry(n, C)[0] for n, C in geo if n > 4096)
    assert any(k % 16 for k in nblks)
    assert {C for _, C in geo} == {64, 128, 192, 256}


@pytest.mark.parametrize("B,H,W,C,Cr,slope", BN_CASES)
def test_bn_forward_train(B, H, W, C, Cr, slope):
    """mean: exact where npix is a power of two (S exact on the budget, / npix exact), else c = D + 2 of mean|x|.
    invstd = 1 / sqrtf(var + eps): var sums nonnegative terms (one rounding each for x - mean and the square, D for the
    sum, one for / npix; the mean's own error enters var only squared: sum (x - m - d)^2 = sum (x - m)^2 + n d^2), + eps,
    sqrt halves the relative error and adds one, 1 / . one more -> c = (D + 4) / 2 + 2.
    running mean (1 - m) rm + m mean: the mean's c plus 3 roundings -> D + 5 of (1 - m)|rm| + m mean|x|; running var
    (1 - m) rv + m var n / (n - 1): var's D + 3, n / (n - 1) one, 4 more -> D + 8."""
    npix = B * H * W
    D = bn_depth(npix, C)
    x = bn_data(npix, C, Cr, seed=npix + C)
    g, b = bn_params(Cr, seed=C + Cr)
    rm0, rv0 = X.shifts((Cr,), 7), X.scales((Cr,), 8)
    rm, rv = dev(rm0), dev(rv0)
    y, mean, inv = bn_fwd_run(dev(x), dev(g), dev(b), C, Cr, True, slope, rm, rv)
    ref = S.bn_fwd_ref(dd(x[:, :Cr]), dd(g), dd(b), 1e-5, slope, dd(rm0), dd(rv0), momentum=M32)
    mabs = dd(x[:, :Cr]).abs().mean(0)
    if npix & (npix - 1) == 0:
        X.assert_budget(dd(x).abs().sum(0), 1.0, "BN pixel sum")
        X.assert_exact(mean[:Cr], ref["mean"], "mean (power-of-two npix: exact)")
    else:
        G.assert_bounded(mean[:Cr], ref["mean"], mabs, D + 2, "mean")
    assert bool((mean[Cr:] == 0).all()), "padded channels' mean"
    G.assert_bounded(inv[:Cr], ref["invstd"], ref["invstd"], (D + 4) / 2 + 2, "invstd")
    G.assert_bounded(rm, ref["rm"], (1 - M32) * dd(rm0).abs() + M32 * mabs, D + 5, "running mean")
    G.assert_bounded(rv, ref["rv"], ref["rv"].abs(), D + 8, "running var (unbiased)")
    yref, ymag = bn_y_bound(x[:, :Cr], g, b, mean[:Cr], inv[:Cr], slope)
    G.assert_bounded(y[:, :Cr], yref, ymag, 4, "y (from the kernel's statistics)")
    G.assert_bounded(y[:, :Cr], ref["y"], bn_y_direct_mag(x[:, :Cr], ref, g, b), 1.5 * D + 10, "y (float64)")
    assert bool((y[:, Cr:] == 0).all()), "padded channels of y"


@pytest.mark.parametrize("B,H,W,C,Cr,slope", [(1, 64, 64, 64, 48, 0.2), (2, 127, 128, 64, 40, 0.0), (1, 16, 16, 192, 150, 1.0),
                                               (1, 64, 128, 256, 200, 0.2)])
def test_bn_forward_eval(B, H, W, C, Cr, slope):
    """running statistics: inv = 1 / sqrtf(rv + eps) (3 roundings), sc, sh, z (3), the slope (1) -> c = 8 of
    (|x| + |rm|) inv |g| + |b|.  The running buffers are read only, the batch statistics not written."""
    npix = B * H * W
    x = bn_data(npix, C, Cr, seed=npix)
    g, b = bn_params(Cr, seed=3)
    rm0, rv0 = X.shifts((Cr,), 9), X.scales((Cr,), 10)
    rm, rv = dev(rm0), dev(rv0)
    y, mean, inv = bn_fwd_run(dev(x), dev(g), dev(b), C, Cr, False, slope, rm, rv)
    ref = S.bn_fwd_ref(dd(x[:, :Cr]), dd(g), dd(b), 1e-5, slope, dd(rm0), dd(rv0), training=False)
    mag = (dd(x[:, :Cr]).abs() + dd(rm0).abs()) * ref["invstd"] * dd(g).abs() + dd(b).abs()
    G.assert_bounded(y[:, :Cr], ref["y"], mag, 8, "eval y")
    assert bool((y[:, Cr:] == 0).all())
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0), "eval mode changed the running statistics"
    assert bool(mean.isnan().all()) and bool(inv.isnan().all()), "eval mode wrote the batch statistics"


@pytest.mark.parametrize("npix,C,Cr", [(4096, 64, 64), (4097, 64, 48), (32768, 64, 64), (262144, 64, 64), (8192, 256, 200)])
def test_bn_forward_without_running_buffers(npix, C, Cr):
    """the instance-norm call (running_mean = running_var = NULL): the same statistics and output, nothing else touched"""
    x = bn_data(npix, C, Cr, seed=5)
    g, b = bn_params(Cr, seed=6)
    y, mean, inv = bn_fwd_run(dev(x), dev(g), dev(b), C, Cr, True, 0.2)
    ref = S.bn_fwd_ref(dd(x[:, :Cr]), dd(g), dd(b), 1e-5, 0.2)
    D = bn_depth(npix, C)
    G.assert_bounded(mean[:Cr], ref["mean"], dd(x[:, :Cr]).abs().mean(0), D + 2, "mean")
    G.assert_bounded(inv[:Cr], ref["invstd"], ref["invstd"], (D + 4) / 2 + 2, "invstd")
    G.assert_bounded(y[:, :Cr], ref["y"], bn_y_direct_mag(x[:, :Cr], ref, g, b), 1.5 * D + 10, "y")
    assert bool((y[:, Cr:] == 0).all())


def bn_bwd_data(npix, C, Cr, seed):
    """dyadic saved statistics (mean k/4, invstd in {0.5, 1, 2}), gamma k/8, beta k/4: z = x sc + sh is exact, so the
    LeakyReLU mask is the float64 one; dy integers in [-1, 1], at most ~16 K of them nonzero per channel (the budget of
    sum dz xhat)"""
    x = padded(X.ints((npix, Cr), seed, -2, 2), C)
    dy = padded(X.ints((npix, Cr), seed + 1, -1, 1, zeros=max(0.0, 1 - 16384 / npix)), C)
    g, b = X.weights((Cr,), seed + 2, nonzero=True), X.shifts((Cr,), seed + 3)
    mean = padded(X.shifts((Cr,), seed + 4), C)
    inv = padded(2.0 ** X.ints((Cr,), seed + 5, -1, 1), C)
    inv[Cr:] = 1.0
    return x, dy, g, b, mean, inv


def bn_bwd_run(x, dy, g, b, mean, inv, C, Cr, slope):
    npix = x.shape[0]
    L = lib()
    nb = L.sisr_bn_workspace_bytes(npix, C)
    ws = nan(nb // 4)
    dx, dg, db = nan(npix, C), nan(Cr), nan(Cr)
    ok(L.sisr_bn_act_bwd(P(dev(x)), P(dev(dy)), P(dev(g)), P(dev(b)), P(dev(mean)), P(dev(inv)), P(dx), P(dg), P(db), npix, C,
                         Cr, float(slope), P(ws), nb, St()), "sisr_bn_act_bwd")
    return dx, dg, db


def bn_bwd_refs(x, dy, g, b, mean, inv, Cr, slope):
    args = (dd(x[:, :Cr]), dd(dy[:, :Cr]), dd(g), dd(b), dd(mean[:Cr]), dd(inv[:Cr]), slope)
    return S.bn_bwd_ref(*args), S.bn_bwd_ref(*args, A=True)


@pytest.mark.parametrize("B,H,W,C,Cr,slope", [(b, h, w, c, cr, s if s != 0.2 else 0.5) for b, h, w, c, cr, s in BN_CASES])
def test_bn_backward_exact(B, H, W, C, Cr, slope):
    """dyadic slope (0, 0.5, 1) and saved statistics: dbeta = sum dz and dgamma = sum dz xhat are exact whatever the
    chunking; dx = gamma inv (dz - fl(dbeta / n) - fl(xhat fl(dgamma / n))): 2 divisions, a product, 2 subtractions and
    the final product -> c = 8 of the A-form"""
    npix = B * H * W
    data = bn_bwd_data(npix, C, Cr, seed=npix + 3 * C)
    ref, mag = bn_bwd_refs(*data, Cr, slope)
    X.assert_budget(mag["dbeta"], X.granule(ref["dz"]), "dbeta")
    X.assert_budget(mag["dgamma"], X.granule(ref["dz"]) * X.granule(ref["xhat"]), "dgamma")
    dx, dg, db = bn_bwd_run(*data, C, Cr, slope)
    X.assert_exact(db, ref["dbeta"], "dbeta")
    X.assert_exact(dg, ref["dgamma"], "dgamma")
    G.assert_bounded(dx[:, :Cr], ref["dx"], mag["dx"], 8, "dx")
    assert bool((dx[:, Cr:] == 0).all()), "padded channels of dx"


@pytest.mark.parametrize("B,H,W,C,Cr", [(1, 64, 64, 64, 48), (16, 128, 128, 64, 64), (1, 61, 83, 192, 150)])
def test_bn_backward_slope_02(B, H, W, C, Cr):
    """slope fl32(0.2): dz = fl(dy 0.2f) (one rounding), then D -> c = D + 1 for the sums, D + 8 for dx"""
    npix = B * H * W
    D = bn_depth(npix, C)
    data = bn_bwd_data(npix, C, Cr, seed=npix)
    ref, mag = bn_bwd_refs(*data, Cr, X.SLOPE32)
    dx, dg, db = bn_bwd_run(*data, C, Cr, 0.2)
    G.assert_bounded(db, ref["dbeta"], mag["dbeta"], D + 1, "dbeta")
    G.assert_bounded(dg, ref["dgamma"], mag["dgamma"], D + 1, "dgamma")
    G.assert_bounded(dx[:, :Cr], ref["dx"], mag["dx"], D + 8, "dx")


@pytest.mark.parametrize("npix,C", [(4096, 64), (262144, 64), (32768, 64), (8192, 256), (5120, 192)])
def test_bn_detector_one_sentinel(npix, C):
    """one chunk-boundary sentinel moved in the kernel's input only: the mean mismatches at exactly its channel (exact
    where npix is a power of two, out of bound otherwise); one dy element at the map's last pixel moved: dbeta mismatches
    at exactly its channel"""
    x = bn_data(npix, C, C, seed=11)
    g, b = bn_params(C, seed=12)
    px = bn_sentinel_pixels(npix, C)
    p, c = px[len(px) // 2], 5
    xp = x.clone()
    xp[p, c] -= 2 * x[p, c]
    _, mean, _ = bn_fwd_run(dev(xp), dev(g), dev(b), C, C, True, 0.2)
    want = torch.zeros(C, dtype=torch.bool)
    want[c] = True
    ref = dd(x).mean(0)
    if npix & (npix - 1) == 0:
        expect_detected(X.mismatch(mean, ref), want, "BN mean")
    else:
        expect_detected(~G.bound_ok(mean, ref, dd(x).abs().mean(0), bn_depth(npix, C) + 2), want, "BN mean")
    data = list(bn_bwd_data(npix, C, C, seed=13))
    rb, _ = bn_bwd_refs(*data, C, 1.0)
    data[1] = data[1].clone()
    data[1][npix - 1, c] += 1.0
    _, _, db = bn_bwd_run(*data, C, C, 1.0)
    expect_detected(X.mismatch(db, rb["dbeta"]), want, "BN dbeta")


def test_bn_ops_wrapper_partial_path():
    """ops.batch_norm_act on 1 x 17 x 241 (partial path): y, the running statistics and num_batches_tracked; the backward at
    slope 1 gives dbeta = sum dy exactly"""
    B, Cr, H, W, C = 1, 48, 17, 241, 64
    npix = B * H * W
    D = bn_depth(npix, C)
    x = bn_data(npix, C, Cr, seed=21)
    bn = torch.nn.BatchNorm2d(Cr)
    g, b = bn_params(Cr, seed=22)
    with torch.no_grad():
        bn.weight.copy_(g)
        bn.bias.copy_(b)
    bn.to(DEV).train()
    xg = nchw_view(dev(x).view(B, H, W, C)).requires_grad_(True)
    y = ops.batch_norm_act(xg, bn, slope=1.0)
    ref = S.bn_fwd_ref(dd(x[:, :Cr]), dd(g), dd(b), 1e-5, 1.0, dd(torch.zeros(Cr)), dd(torch.ones(Cr)), momentum=M32)
    yc = rows_of(y.detach())
    mabs = dd(x[:, :Cr]).abs().mean(0)
    G.assert_bounded(yc[:, :Cr], ref["y"], bn_y_direct_mag(x[:, :Cr], ref, g, b), 1.5 * D + 10, "y")
    assert bool((yc[:, Cr:] == 0).all())
    G.assert_bounded(bn.running_mean, ref["rm"], M32 * mabs, D + 5, "running mean")
    G.assert_bounded(bn.running_var, ref["rv"], ref["rv"], D + 8, "running var")
    assert int(bn.num_batches_tracked) == 1
    dy = padded(X.ints((npix, Cr), 23, -1, 1), C)
    y.backward(nchw_view(dev(dy).view(B, H, W, C)))
    X.assert_exact(bn.bias.grad, dd(dy[:, :Cr]).sum(0), "dbeta through the wrapper")
    assert bool((rows_of(xg.grad)[:, Cr:] == 0).all())


def test_bn_ops_instance_norm_per_sample():
    """ops.instance_norm_act runs the batch-norm kernels once per sample with no running buffers: each sample's output equals
    the float64 instance norm within the partial path's bound (64 x 65 pixels per sample)"""
    B, Cr, H, W, C = 3, 40, 64, 65, 64
    npix = H * W
    D = bn_depth(npix, C)
    xs = [bn_data(npix, C, Cr, seed=30 + k) for k in range(B)]
    x = torch.stack(xs).view(B, H, W, C)
    norm = torch.nn.InstanceNorm2d(Cr, affine=True)
    g, b = bn_params(Cr, seed=33)
    with torch.no_grad():
        norm.weight.copy_(g)
        norm.bias.copy_(b)
    norm.to(DEV)
    y = ops.instance_norm_act(nchw_view(dev(x)), norm, slope=0.2)
    for k in range(B):
        ref = S.bn_fwd_ref(dd(xs[k][:, :Cr]), dd(g), dd(b), 1e-5, 0.2)
        yk = rows_of(y[k:k + 1].detach())
        G.assert_bounded(yk[:, :Cr], ref["y"], bn_y_direct_mag(xs[k][:, :Cr], ref, g, b), 1.5 * D + 10,
                         f"instance norm sample {k}")


# ============================================================================ 2. group / instance norm
def gn_depth(hw, cg):
    """per-thread sum over ceil(hw cg / 256) elements, the xor tree (6), (r0 + r1) + (r2 + r3) (2)"""
    return -(-hw * cg // 256) + 6 + 2


def gn_fwd_run(x, g, b, B, hw, C, Cr, cg, eps=1e-5):
    y, mean, inv = nan(B, hw, C), nan(B * (Cr // cg)), nan(B * (Cr // cg))
    ok(lib().sisr_group_norm_fwd(P(dev(x)), P(y), P(dev(g)), P(dev(b)), P(mean), P(inv), B, hw, C, Cr, cg, float(eps), St()),
       "sisr_group_norm_fwd")
    return y, mean.view(B, -1), inv.view(B, -1)


def gn_bwd_run(x, dy, g, mean, inv, B, hw, C, Cr, cg):
    dx, dgb, dbb = nan(B, hw, C), nan(B, Cr), nan(B, Cr)
    ok(lib().sisr_group_norm_bwd(P(dev(x)), P(dev(dy)), P(dev(g)), P(dev(mean)), P(dev(inv)), P(dx), P(dgb), P(dbb), B, hw, C,
                                 Cr, cg, St()), "sisr_group_norm_bwd")
    return dx, dgb, dbb


# (B, H, W, C, C_real, cg): cg 1 (instance norm) / 2 / 4, padded channels, hw below / at / above 256, n = hw cg a power
# of two (the exact mean) and not
GN_CASES = [(2, 7, 9, 64, 48, 1), (2, 17, 19, 64, 64, 2), (1, 16, 16, 64, 64, 4), (3, 32, 32, 128, 96, 2), (2, 5, 3, 64, 60, 4),
            (2, 64, 64, 64, 64, 1), (1, 33, 31, 64, 32, 2)]


@pytest.mark.parametrize("B,H,W,C,Cr,cg", GN_CASES)
def test_group_norm_forward(B, H, W, C, Cr, cg):
    """mean exact where hw cg is a power of two, else c = D + 2 of mean|x|; invstd c = (D + 4) / 2 + 2 (as batch norm);
    y = fl(fl(fl(x - mean) inv) gamma) + beta from the kernel's statistics: 4 roundings -> c = 4 of
    (|x| + |mean|) inv |g| + |b|"""
    hw = H * W
    D = gn_depth(hw, cg)
    x = padded(X.nonzero_ints((B, hw, Cr), hw + cg, 2), C)
    x[:, -1, :Cr] = SENT
    g, b = bn_params(Cr, seed=cg)
    y, mean, inv = gn_fwd_run(x, g, b, B, hw, C, Cr, cg)
    ref = S.gn_fwd_ref(dd(x[..., :Cr]), dd(g), dd(b), cg, 1e-5)
    n = hw * cg
    if n & (n - 1) == 0:
        X.assert_exact(mean, ref["mean"], "group mean (power-of-two count: exact)")
    else:
        mabs = dd(x[..., :Cr]).abs().view(B, hw, Cr // cg, cg).mean(dim=(1, 3))
        G.assert_bounded(mean, ref["mean"], mabs, D + 2, "group mean")
    G.assert_bounded(inv, ref["invstd"], ref["invstd"], (D + 4) / 2 + 2, "group invstd")
    m = mean.double().repeat_interleave(cg, 1)[:, None, :]
    iv = inv.double().repeat_interleave(cg, 1)[:, None, :]
    xr = dd(x[..., :Cr])
    yref = (xr - m) * iv * dd(g) + dd(b)
    G.assert_bounded(y[..., :Cr], yref, (xr.abs() + m.abs()) * iv * dd(g).abs() + dd(b).abs(), 4, "y")
    assert bool((y[..., Cr:] == 0).all()), "padded channels of y"


@pytest.mark.parametrize("B,H,W,C,Cr,cg", GN_CASES)
def test_group_norm_backward(B, H, W, C, Cr, cg):
    """dyadic saved statistics: the per-sample dgamma_b / dbeta_b exact; dx = inv (dh - fl(S1 / n) - xhat fl(S2 / n)) with
    S1, S2 exact sums: c = 8 of the A-form (as batch norm)"""
    hw = H * W
    x = padded(X.ints((B, hw, Cr), hw, -2, 2), C)
    dy = padded(X.ints((B, hw, Cr), hw + 1, -1, 1), C)
    g = X.weights((Cr,), 3, nonzero=True)
    mean, inv = X.shifts((B, Cr // cg), 4), 2.0 ** X.ints((B, Cr // cg), 5, -1, 1)
    args = (dd(x[..., :Cr]), dd(dy[..., :Cr]), dd(g), dd(mean), dd(inv), cg)
    ref, mag = S.gn_bwd_ref(*args), S.gn_bwd_ref(*args, A=True)
    X.assert_budget(mag["dgamma_b"], 1 / 8, "dgamma_b")
    dx, dgb, dbb = gn_bwd_run(x, dy, g, mean, inv, B, hw, C, Cr, cg)
    X.assert_exact(dbb, ref["dbeta_b"], "dbeta_b")
    X.assert_exact(dgb, ref["dgamma_b"], "dgamma_b")
    G.assert_bounded(dx[..., :Cr], ref["dx"], mag["dx"], 8, "dx")
    assert bool((dx[..., Cr:] == 0).all()), "padded channels of dx"


def test_group_norm_ops_wrapper_and_detector():
    """ops.group_norm: the parameter gradients are the per-sample partials added in batch order by sisr_sum_partials
    (exact); one x element moved in the kernel's input only: the exact mean mismatches at exactly its (sample, group)"""
    B, H, W, C, cg = 3, 16, 16, 64, 2
    hw = H * W
    x = X.nonzero_ints((B, hw, C), 40, 2)
    g, b = bn_params(C, seed=41)
    xg = nchw_view(dev(x).view(B, H, W, C)).requires_grad_(True)
    gp, bp = dev(g).requires_grad_(True), dev(b).requires_grad_(True)
    y = ops.group_norm(xg, gp, bp, cg)
    dy = X.ints((B, hw, C), 42, -1, 1)
    y.backward(nchw_view(dev(dy).view(B, H, W, C)))
    X.assert_exact(bp.grad, dd(dy).sum(dim=(0, 1)), "dbeta")
    xp = x.clone()
    xp[1, 100, 7] += 1.0
    _, mean, _ = gn_fwd_run(xp, g, b, B, hw, C, C, cg)
    want = torch.zeros(B, C // cg, dtype=torch.bool)
    want[1, 7 // cg] = True
    expect_detected(X.mismatch(mean, S.gn_fwd_ref(dd(x), dd(g), dd(b), cg, 1e-5)["mean"]), want, "group mean")


# ============================================================================ 3. pixel norm
def pn_data(npix, C, seed):
    x = X.ints((npix, C), seed, -3, 3) / 4
    x[0] = 0.0                 # all-zero pixel
    x[npix // 2] = 1e-14       # norm below eps: x / eps
    x[npix - 1] = 0.0
    x[npix - 1, 0] = 3.0       # a single channel
    return x


@pytest.mark.parametrize("npix,C", [(1000, 64), (777, 128), (4099, 256)])
def test_pixel_norm_forward_backward(npix, C):
    """C / 4 = 16 / 32 / 64 lanes per pixel.  n2: products (1), the in-thread pair sums (2), the xor tree over log2(C / 4)
    lanes; sqrt halves and adds 1, the division 1 -> forward c = log2(C / 4) / 2 + 5 of |y|.  Backward: the same den, the
    <dy, y> tree (log2(C / 4) + 3), the product and the subtraction -> c = log2(C / 4) + 12 of the A-form"""
    L2 = math.log2(C // 4)
    x = pn_data(npix, C, npix)
    dy = X.ints((npix, C), npix + 1, -2, 2) / 2
    y = nan(npix, C)
    ok(lib().sisr_pixel_norm(P(dev(x)), None, P(y), npix, C, 0, St()), "sisr_pixel_norm")
    ref = S.pn_fwd_ref(dd(x))
    G.assert_bounded(y, ref["y"], ref["y"].abs(), L2 / 2 + 5, "y")
    assert bool((y[0] == 0).all())
    dx = nan(npix, C)
    ok(lib().sisr_pixel_norm(P(dev(x)), P(dev(dy)), P(dx), npix, C, 1, St()), "sisr_pixel_norm(bwd)")
    G.assert_bounded(dx, S.pn_bwd_ref(dd(x), dd(dy)), S.pn_bwd_ref(dd(x), dd(dy), A=True), L2 + 12, "dx")
    yw = ops.pixel_norm(nchw_view(dev(x).view(1, npix, 1, C)))
    assert torch.equal(rows_of(yw), y), "ops.pixel_norm differs from the direct call"
    xp = x.clone()
    xp[7, 3] += 0.25
    yp = nan(npix, C)
    ok(lib().sisr_pixel_norm(P(dev(xp)), None, P(yp), npix, C, 0, St()), "sisr_pixel_norm")
    bad = ~G.bound_ok(yp, ref["y"], ref["y"].abs(), L2 / 2 + 5)
    assert bool(bad[7].any()) and not bool(bad[:7].any()) and not bool(bad[8:].any()), "pixel norm detector"


# ============================================================================ 4. PReLU / LeakyReLU / SELU
def act_run(x, dy, a, npix, C, Cr, mode):
    y = nan(npix, C)
    ok(lib().sisr_act(P(dev(x)), None, P(a), P(y), None, npix, C, Cr, mode, 0, St()), "sisr_act")
    if dy is None:
        return y, None, None
    dx, dyx = nan(npix, C), (nan(npix, C) if mode == 0 else None)
    ok(lib().sisr_act(P(dev(x)), P(dev(dy)), P(a), P(dx), P(dyx), npix, C, Cr, mode, 1, St()), "sisr_act(bwd)")
    return y, dx, dyx


@pytest.mark.parametrize("npix,C,Cr", [(1000, 64, 64), (513, 64, 40), (4096, 128, 100), (7, 256, 256)])
def test_prelu_exact(npix, C, Cr):
    """dyadic slopes k/8 (zero and negative ones included) and x with exact zeros: y, dx, dyx exact; the slope gradient
    through ops._pixel_sums + sisr_sum_partials exact; padded channels 0"""
    x = padded(X.ints((npix, Cr), npix, -2, 2, zeros=0.2), C)
    dy = padded(X.ints((npix, Cr), npix + 1, -2, 2), C)
    a = X.weights((Cr,), npix + 2)
    y, dx, dyx = act_run(x, dy, dev(a), npix, C, Cr, 0)
    ref = S.prelu_bwd_ref(dd(x[:, :Cr]), dd(dy[:, :Cr]), dd(a))
    yref = padded(S.prelu_ref(dd(x[:, :Cr]), dd(a)), C)
    X.assert_exact(y, yref, "y")
    X.assert_exact(dx[:, :Cr], ref["dx"], "dx")
    X.assert_exact(dyx, padded(ref["dyx"], C), "dyx")
    assert bool((dx[:, Cr:] == 0).all())
    part, parts = ops._pixel_sums(dyx, None, 1, npix, 1, C)
    da = nan(C)
    ok(lib().sisr_sum_partials(P(part), parts, 1, C, 1.0, P(da), St()), "sisr_sum_partials")
    X.assert_exact(da[:Cr], ref["da"], "slope gradient")
    xp = x.clone()
    xp[npix - 1, 0] = -1.0 if x[npix - 1, 0] > 0 else 2.0
    yp, _, _ = act_run(xp, None, dev(a), npix, C, Cr, 0)
    want = torch.zeros(npix, C, dtype=torch.bool)
    want[npix - 1, 0] = True
    expect_detected(X.mismatch(yp, yref), want, "PReLU y")


def test_prelu_and_leaky_ops_wrappers():
    """ops.prelu (per-channel and one shared slope) and ops.leaky_relu at the dyadic slope 0.25: exact forward, input and
    slope gradients"""
    B, H, W, C = 2, 9, 11, 64
    x = X.ints((B, H, W, C), 50, -2, 2, zeros=0.2)
    dy = X.ints((B, H, W, C), 51, -2, 2)
    xr, dyr = dd(x).view(-1, C), dd(dy).view(-1, C)
    for a in (X.weights((C,), 52), torch.tensor([0.375])):
        xg = nchw_view(dev(x)).requires_grad_(True)
        ag = dev(a).requires_grad_(True)
        y = ops.prelu(xg, ag)
        y.backward(nchw_view(dev(dy)))
        af = dd(a.expand(C) if a.numel() == 1 else a)
        ref = S.prelu_bwd_ref(xr, dyr, af)
        X.assert_exact(rows_of(y.detach()), S.prelu_ref(xr, af), "ops.prelu y")
        X.assert_exact(rows_of(xg.grad), ref["dx"], "ops.prelu dx")
        X.assert_exact(ag.grad, ref["da"] if a.numel() > 1 else ref["da"].sum().reshape(1), "ops.prelu slope gradient")
    xg = nchw_view(dev(x)).requires_grad_(True)
    y = ops.leaky_relu(xg, 0.25)
    y.backward(nchw_view(dev(dy)))
    X.assert_exact(rows_of(y.detach()), torch.where(xr > 0, xr, 0.25 * xr), "leaky y")
    X.assert_exact(rows_of(xg.grad), torch.where(xr > 0, dyr, 0.25 * dyr), "leaky dx (x = 0: the slope)")


# SELU: x > 0: fl(SCALE32 x) (the constant's rounding and the product: 2).  x <= 0: expm1f (<= 2 ulp), ALPHA32 and
# SCALE32 (1 each), two products -> c = 6 of |y|.  Backward: expf (2), the constants (2), three products -> c = 8 of |dx|.
C_SELU_FWD, C_SELU_BWD = 6, 8


@pytest.mark.parametrize("npix,C", [(1000, 64), (33, 128)])
def test_selu(npix, C):
    g = torch.Generator().manual_seed(npix)
    x = torch.randn((npix, C), generator=g) * 3
    x[0, :4] = 0.0
    dy = torch.randn((npix, C), generator=g)
    y, dx, _ = act_run(x, dy, None, npix, C, C, 1)
    G.assert_bounded(y, S.selu_ref(dd(x)), S.selu_ref(dd(x), A=True), C_SELU_FWD, "selu y")
    ref = S.selu_bwd_ref(dd(x), dd(dy))
    G.assert_bounded(dx, ref, ref.abs(), C_SELU_BWD, "selu dx")
    yw = ops.selu(nchw_view(dev(x).view(1, npix, 1, C)))
    assert torch.equal(rows_of(yw), y)


def test_selu_small_negative_relative_error():
    """small |x| < 0: SCALE ALPHA (e^x - 1) computed as expf(x) - 1 cancels (x = -1e-6 comes out 5 % low); expm1f keeps the
    relative error within c = 6 ulps"""
    vals = [-1e-7, -3e-7, -1e-6, -2.5e-6, -1e-5, -1e-4, -1e-3, -0.01, -0.1, -1e-20, -1e-30]
    x = torch.zeros(4, 64)
    x.view(-1)[:len(vals)] = torch.tensor(vals)
    y, _, _ = act_run(x, None, None, 4, 64, 64, 1)
    G.assert_bounded(y, S.selu_ref(dd(x)), S.selu_ref(dd(x), A=True), C_SELU_FWD, "selu at small negative x")


# ============================================================================ 5. attention products
@pytest.mark.parametrize("npix,C,Cl,identity", [(1000, 64, 64, True), (333, 128, 4, False), (4097, 256, 64, True),
                                                (64, 64, 8, False)])
def test_spar_combine(npix, C, Cl, identity):
    """C / 4 = 16 / 32 / 64 lanes per pixel.  Forward: a = sigmoid (C_SIG of a), y = x a [+ idn] (2 more of |x| a + |idn|).
    Backward at a dyadic attention a in {1/4, 1/2, 3/4}: dx = dy a and dlogit[0] = fl(fl(<dy, x> a) (1 - a)) exact, every
    other logit channel exactly 0"""
    g = torch.Generator().manual_seed(npix)
    x, lg = torch.randn((npix, C), generator=g), torch.randn((npix, Cl), generator=g) * 4
    idn = torch.randn((npix, C), generator=g) if identity else None
    y, att = nan(npix, C), nan(npix)
    ok(lib().sisr_spar_combine_fwd(P(dev(x)), P(dev(lg)), P(dev(idn)) if identity else None, P(y), P(att), npix, C, Cl, St()),
       "sisr_spar_combine_fwd")
    ref = S.spar_combine_ref(dd(x), dd(lg[:, 0]), dd(idn) if identity else None)
    G.assert_bounded(att, ref["a"], ref["a"], C_SIG, "a")
    mag = dd(x).abs() * ref["a"][:, None] + (dd(idn).abs() if identity else 0)
    G.assert_bounded(y, ref["y"], mag, C_SIG + 2, "y")
    xi, dy = X.ints((npix, C), npix + 1, -2, 2), X.ints((npix, C), npix + 2, -2, 2)
    a = X.ints((npix,), npix + 3, 1, 3) / 4

    def bwd(dy_):
        dx, dl = nan(npix, C), nan(npix, Cl)
        ok(lib().sisr_spar_combine_bwd(P(dev(dy_)), P(dev(xi)), P(dev(a)), P(dx), P(dl), npix, C, Cl, St()),
           "sisr_spar_combine_bwd")
        return dx, dl

    dx, dl = bwd(dy)
    rb = S.spar_combine_bwd_ref(dd(dy), dd(xi), dd(a))
    X.assert_exact(dx, rb["dx"], "dx")
    X.assert_exact(dl[:, 0], rb["dlogit"], "dlogit[0]")
    assert bool((dl[:, 1:] == 0).all()), "other logit channels"
    dyp = dy.clone()
    dyp[npix - 1, C - 1] += 1.0
    xi[npix - 1, C - 1] = 1.0
    rb = S.spar_combine_bwd_ref(dd(dy), dd(xi), dd(a))
    dx2, dl2 = bwd(dyp)
    want = torch.zeros(npix, C, dtype=torch.bool)
    want[npix - 1, C - 1] = True
    expect_detected(X.mismatch(dx2, rb["dx"]), want, "dx")
    expect_detected(X.mismatch(dl2[:, 0], rb["dlogit"]), want.any(1), "dlogit")


def test_spar_combine_ops_wrapper():
    B, H, W, C = 2, 5, 7, 64
    g = torch.Generator().manual_seed(3)
    x, lg, idn, dy = (torch.randn((B, C, H, W), generator=g) for _ in range(4))
    xg, lgg, ig = (dev(t).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in (x, lg, idn))
    y = ops.spar_combine(xg, lgg, ig)
    xr = rows_of(dd(x))
    ref = S.spar_combine_ref(xr, rows_of(dd(lg))[:, 0], rows_of(dd(idn)))
    mag = xr.abs() * ref["a"][:, None] + rows_of(dd(idn)).abs()
    G.assert_bounded(rows_of(y.detach()), ref["y"], mag, C_SIG + 2, "ops.spar_combine y")
    y.backward(dev(dy))
    rb = S.spar_combine_bwd_ref(rows_of(dd(dy)), xr, ref["a"])
    mb = S.spar_combine_bwd_ref(rows_of(dd(dy)), xr, ref["a"], A=True)
    # the attention is the kernel's own (C_SIG); <dy, x> over 64 channels: 3 in-thread levels + the 4-level xor tree; two
    # products -> c = C_SIG + 10 of the A-form
    G.assert_bounded(rows_of(lgg.grad)[:, 0], rb["dlogit"], mb["dlogit"], C_SIG + 10, "ops.spar_combine dlogit")
    assert bool((lgg.grad[:, 1:] == 0).all())
    X.assert_exact(ig.grad, dd(dy), "identity gradient")


@pytest.mark.parametrize("n,identity", [(4, True), (1000, False), (64 * 4097, True)])
def test_spar3d(n, identity):
    """forward: sigmoid (C_SIG), x a [+ idn] -> C_SIG + 2 of |x| a + |idn|.  Backward: dy a -> C_SIG + 1 of |dy| a;
    dy x a (1 - a): (1 - a) carries a's absolute error -> C_SIG + 4 of the A-form |dy x| a (1 + a)"""
    g = torch.Generator().manual_seed(n)
    x, lg, idn, dy = (torch.randn(n, generator=g) * s for s in (1.0, 4.0, 1.0, 1.0))

    def fwd(x_):
        out = nan(n)
        ok(lib().sisr_spar3d(P(dev(x_)), P(dev(lg)), P(dev(idn)) if identity else None, P(out), None, n, 0, St()), "sisr_spar3d")
        return out

    out = fwd(x)
    ref = S.spar3d_ref(dd(x), dd(lg), dd(idn) if identity else None)
    mag = dd(x).abs() * ref["a"] + (dd(idn).abs() if identity else 0)
    G.assert_bounded(out, ref["y"], mag, C_SIG + 2, "y")
    dx, dl = nan(n), nan(n)
    ok(lib().sisr_spar3d(P(dev(x)), P(dev(lg)), P(dev(dy)), P(dx), P(dl), n, 1, St()), "sisr_spar3d(bwd)")
    rb, mb = S.spar3d_bwd_ref(dd(dy), dd(x), dd(lg)), S.spar3d_bwd_ref(dd(dy), dd(x), dd(lg), A=True)
    G.assert_bounded(dx, rb["dx"], mb["dx"], C_SIG + 1, "dx")
    G.assert_bounded(dl, rb["dlogits"], mb["dlogits"], C_SIG + 4, "dlogits")
    i = int(lg.argmax())
    xp = x.clone()
    xp[i] += 8.0
    bad = ~G.bound_ok(fwd(xp), ref["y"], mag, C_SIG + 2)
    assert bool(bad[i]) and int(bad.sum()) == 1, "spar3d detector"


def test_spar3d_ops_wrapper():
    B, C, H, W = 2, 64, 3, 5
    g = torch.Generator().manual_seed(9)
    x, lg = torch.randn((B, C, H, W), generator=g), torch.randn((B, C, H, W), generator=g)
    cl = torch.channels_last
    y = ops.spar_combine3d(dev(x).contiguous(memory_format=cl), dev(lg).contiguous(memory_format=cl))
    ref = S.spar3d_ref(dd(x), dd(lg))
    G.assert_bounded(y, ref["y"], dd(x).abs() * ref["a"], C_SIG + 2, "ops.spar_combine3d")


# ============================================================================ 6. geometry (exact)
def nhwc_ints(B, H, W, C, seed):
    return X.ints((B, H, W, C), seed, -100, 100)


@pytest.mark.parametrize("B,H,W,C,up", [(1, 2, 2, 4, 1), (2, 2, 3, 8, 2), (2, 7, 5, 64, 1), (1, 9, 4, 64, 2), (3, 33, 17, 12, 2),
                                        (1, 128, 128, 64, 1)])
def test_pad_reflect_up_and_adjoint(B, H, W, C, up):
    x = nhwc_ints(B, H, W, C, H * W + up)
    Hp, Wp = up * H + 2, up * W + 2
    y = nan(B, Hp, Wp, C)
    ok(lib().sisr_pad_reflect_up(P(dev(x)), P(y), B, H, W, C, up, 0, St()), "sisr_pad_reflect_up")
    X.assert_exact(y, S.pad_reflect_up_ref(dd(x), up), "padded map")
    dy = X.ints((B, Hp, Wp, C), H + W, -4, 4)

    def adj(dy_):
        dx = nan(B, H, W, C)
        ok(lib().sisr_pad_reflect_up(P(dev(dy_)), P(dx), B, H, W, C, up, 1, St()), "sisr_pad_reflect_up(adjoint)")
        return dx

    ref = S.pad_reflect_up_adj(dd(dy), H, W, up)
    X.assert_exact(adj(dy), ref, "adjoint")
    dyp = dy.clone()
    dyp[B - 1, 0, Wp - 1, C - 1] += 1.0  # the ring's corner: read from source pixel (src(0), src(Wp - 1))
    want = torch.zeros(B, H, W, C, dtype=torch.bool)
    want[B - 1, int(S._reflect_src(H, up)[0]), int(S._reflect_src(W, up)[Wp - 1]), C - 1] = True
    expect_detected(X.mismatch(adj(dyp), ref), want, "reflect adjoint corner")


@pytest.mark.parametrize("B,Hf,Wf,C,stride", [(1, 3, 3, 4, 1), (2, 7, 8, 8, 2), (1, 8, 7, 64, 2), (2, 34, 33, 64, 1), (1, 3, 4, 4, 2)])
def test_crop_stride_and_embed(B, Hf, Wf, C, stride):
    src = nhwc_ints(B, Hf, Wf, C, Hf + Wf)
    Ho, Wo = (Hf - 3) // stride + 1, (Wf - 3) // stride + 1
    y = nan(B, Ho, Wo, C)
    ok(lib().sisr_crop_stride(P(dev(src)), P(y), B, Hf, Wf, C, stride, 0, St()), "sisr_crop_stride")
    X.assert_exact(y, S.crop_stride_ref(dd(src), stride), "crop")
    e = nan(B, Hf, Wf, C)
    ok(lib().sisr_crop_stride(P(y), P(e), B, Hf, Wf, C, stride, 1, St()), "sisr_crop_stride(embed)")
    X.assert_exact(e, S.crop_stride_adj(dd(y), Hf, Wf, stride), "embed (zeros elsewhere)")


@pytest.mark.parametrize("B,H,W,C,up", [(1, 1, 1, 4, 2), (2, 3, 5, 8, 3), (1, 2, 2, 64, 4), (2, 4, 3, 12, 1), (1, 31, 17, 64, 2)])
def test_nearest_up_and_adjoint(B, H, W, C, up):
    x = nhwc_ints(B, H, W, C, H + up)
    y = nan(B, H * up, W * up, C)
    ok(lib().sisr_nearest_up(P(dev(x)), P(y), B, H, W, C, up, 0, St()), "sisr_nearest_up")
    X.assert_exact(y, S.nearest_up_ref(dd(x), up), "upsampled")
    dy = X.ints((B, H * up, W * up, C), W + up, -4, 4)
    dx = nan(B, H, W, C)
    ok(lib().sisr_nearest_up(P(dev(dy)), P(dx), B, H, W, C, up, 1, St()), "sisr_nearest_up(adjoint)")
    X.assert_exact(dx, S.nearest_up_adj(dd(dy), up), "adjoint")
    yw = ops.nearest_up(nchw_view(dev(x)), up)
    X.assert_exact(yw.permute(0, 2, 3, 1), S.nearest_up_ref(dd(x), up), "ops.nearest_up")


# ============================================================================ 7. LAM
# lam_parts = min(128, ceil(k4 / 256)), k4 = chw / 4; the apply grid ablocks = min(1024, ceil(k4 / 256)).
def lam_parts(k4):
    return max(1, min(128, -(-k4 // 256)))


def lam_depth(k4):
    """the Gram entries: ceil(k4 / (parts 256)) float4 iterations per thread, each the product (1) and (m0 + m1) +
    (m2 + m3) (2); wsum (6); ((r0 + r1) + r2) + r3 (3); the parts added in order by the consumer"""
    parts = lam_parts(k4)
    return -(-k4 // (parts * 256)) + 3 + 6 + 3 + parts


def lam_data(B, N, chw, seed, scale=None):
    """|X_i|^2 ~ 2 by default: the attention's arguments stay O(1), so no row collapses to one-hot"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, N, chw), generator=g) * (math.sqrt(2.0 / chw) if scale is None else scale)


def lam_fwd_run(X_, gamma, B, N, chw):
    L = lib()
    ws = nan(max(L.sisr_lam_workspace_bytes(B, N, chw) // 4, 1))
    y, attn = nan(B, N, chw), nan(B, N, N)
    ok(L.sisr_lam_fwd(P(dev(X_)), P(dev(torch.tensor([gamma]))), P(y), P(attn), P(ws), B, N, chw, St()), "sisr_lam_fwd")
    return y, attn


def lam_y_check(Xh, A, gamma):
    """y from the kernel's attention: coef = fl(gamma A + I) (2), N sequential products and sums -> c = N + 3 of
    sum_j (|gamma| A_ij + I_ij) |X_j|"""
    N = Xh.shape[1]
    eye = torch.eye(N, dtype=torch.float64, device=A.device)
    return gamma * (A @ dd(Xh)) + dd(Xh), (abs(gamma) * A + eye) @ dd(Xh).abs(), N + 3


def lam_check_fwd(Xh, y, attn, gamma, k4):
    """attention: E errs by D 2^-24 M (M = |X| |X|^T); the row max and top each by that, so an exponent argument by
    4 D Mrow + 3 R (R = the row's largest argument); expf adds 2; the denominator and the division (N + 2) ->
    |dA| <= (8 D Mrow + 6 R + N + 6) 2^-24 A"""
    N = Xh.shape[1]
    D = lam_depth(k4)
    ref = S.lam_fwd_ref(dd(Xh), gamma)
    M = dd(Xh).abs() @ dd(Xh).abs().transpose(1, 2)
    E = ref["E"]
    R = (E.max(-1, keepdim=True)[0] - E).max(-1, keepdim=True)[0]
    c_row = 8 * D * M.max(-1, keepdim=True)[0] + 6 * R + N + 6
    G.assert_bounded(attn, ref["A"], ref["A"] * c_row, 1, "attention")
    yref, mag, c = lam_y_check(Xh, attn.double(), gamma)
    G.assert_bounded(y, yref, mag, c, "y")


def lam_check_bwd(Xh, attn, gamma, dO, dx, dg, k4):
    """G = dO X^T errs by D of |dO| |X|^T; rowdot by D + N; dE by D + N + 3; C2 = dE + dE^T one more; dx sums 2N terms
    of C1 dO and C2 X -> c = D + 3N + 8 of the A-form.  dgamma: rowdot (N), the rows (N), the samples (B) ->
    c = D + 2N + B + 2"""
    B, N = Xh.shape[0], Xh.shape[1]
    D = lam_depth(k4)
    ref = S.lam_bwd_ref(dd(Xh), attn, gamma, dd(dO))
    mag = S.lam_bwd_ref(dd(Xh), attn, gamma, dd(dO), A=True)
    G.assert_bounded(dx, ref["dx"], mag["dx"], D + 3 * N + 8, "dx")
    G.assert_bounded(dg, ref["dgamma"].reshape(1), mag["dgamma"].reshape(1), D + 2 * N + B + 2, "dgamma")


# (B, N, chw): every N of LAM_DISPATCH; k4 = chw / 4 below 256 (one part), between, above 128 * 256 (parts capped at
# 128: two grid-stride rounds), and above 1024 * 256 (the apply grid capped at 1024)
LAM_CASES = [(2, 2, 960), (1, 3, 960), (2, 4, 64 * 20 * 20), (1, 5, 64 * 9 * 7), (2, 6, 64 * 48 * 48), (1, 8, 64 * 16 * 16),
             (1, 11, 64 * 48 * 48), (2, 11, 64 * 3 * 5), (1, 4, 64 * 130 * 130), (1, 11, 64 * 130 * 130)]


def test_lam_cases_sit_on_both_sides_of_every_rule():
    k4s = [chw // 4 for _, _, chw in LAM_CASES]
    assert {N for _, N, _ in LAM_CASES} == {2, 3, 4, 5, 6, 8, 11}
    assert any(k < 256 for k in k4s) and any(256 <= k <= 128 * 256 for k in k4s) and any(k > 128 * 256 for k in k4s)
    assert any(k > 1024 * 256 for k in k4s)


@pytest.mark.parametrize("B,N,chw", LAM_CASES)
def test_lam_forward_backward(B, N, chw):
    k4 = chw // 4
    Xh = lam_data(B, N, chw, seed=N * 1000 + chw % 997)
    gamma = 0.75
    y, attn = lam_fwd_run(Xh, gamma, B, N, chw)
    lam_check_fwd(Xh, y, attn, gamma, k4)
    dO = lam_data(B, N, chw, seed=N + 7, scale=1.0)
    L = lib()
    ws = nan(L.sisr_lam_workspace_bytes(B, N, chw) // 4)
    dx, dg = nan(B, N, chw), nan(1)
    ok(L.sisr_lam_bwd(P(dev(Xh)), P(attn), P(dev(torch.tensor([gamma]))), P(dev(dO)), P(dx), P(dg), P(ws), B, N, chw, St()),
       "sisr_lam_bwd")
    lam_check_bwd(Xh, attn.double(), gamma, dO, dx, dg, k4)


def test_lam_ops_wrapper_and_detector():
    """ops.lam on a [B][N][H][W][64] stack equals the direct call bit for bit; the last element of the last map moved in the
    kernel's input only breaks y's bound"""
    B, N, H, W = 2, 11, 12, 10
    chw = 64 * H * W
    Xh = lam_data(B, N, chw, seed=77)
    y = ops.lam(dev(Xh).view(B, N, H, W, 64), dev(torch.tensor([0.5])))
    y2, attn = lam_fwd_run(Xh, 0.5, B, N, chw)
    assert torch.equal(y.reshape(B, N, chw), y2)
    lam_check_fwd(Xh, y2, attn, 0.5, chw // 4)
    Xp = Xh.clone()
    Xp[B - 1, N - 1, chw - 1] += 1.0
    y3, _ = lam_fwd_run(Xp, 0.5, B, N, chw)
    yref, mag, c = lam_y_check(Xh, attn.double(), 0.5)
    assert not bool(G.bound_ok(y3, yref, mag, c).all()), "LAM detector: a moved element went unnoticed"


# ============================================================================ 8. CSAM
def csam_depth(npix):
    """csam_blocks = min(2048, ceil(npix / 16)); per thread 4 channels x ceil(npix / (16 blocks)) pixels in order, wsum (6),
    the 4 waves (3), the blocks' partials in order by csam_finish"""
    nb = max(1, min(2048, -(-npix // 16)))
    return 4 * -(-npix // (16 * nb)) + 6 + 3 + nb


def csam_data(B, H, W, seed):
    """dyadic x (k/4), w (k/16), bias (k/8), gamma 3/4: z = bias + conv3d(x) is exact in fp32 (granule 1/64, |z| < 8)"""
    x = X.ints((B, H, W, 64), seed, -4, 4) / 4
    w = X.ints((27,), seed + 1, -4, 4) / 16
    bias = X.ints((1,), seed + 2, -4, 4) / 8
    dy = X.ints((B, H, W, 64), seed + 3, -4, 4) / 4
    return x, w, bias, torch.tensor([0.75]), dy


def csam_fwd_run(x, w, bias, gamma, B, H, W):
    y = nan(B, H, W, 64)
    ok(lib().sisr_csam_fwd(P(dev(x)), P(dev(w)), P(dev(bias)), P(dev(gamma)), P(y), B, H, W, 64, St()), "sisr_csam_fwd")
    return y


# (B, H, W): H or W = 1, a single pixel, odd sizes, B H W just below and above 16 * 2048 = 32768 (the grid-stride rounds)
CSAM_CASES = [(1, 1, 7), (2, 5, 1), (1, 1, 1), (2, 9, 13), (3, 33, 17), (1, 181, 181), (2, 130, 130)]


@pytest.mark.parametrize("B,H,W", CSAM_CASES)
def test_csam_forward_backward(B, H, W):
    """exact z, so: y = x (1 + gamma s): s C_SIG, 3 more -> c = C_SIG + 3 of |x| (1 + |gamma| s).  Backward: dz = dy x gamma s
    (1 - s): (1 - s) carries s's absolute error -> C_SIG + 5 of the A-form; dgamma = sum dy x s: D + C_SIG + 2; dbias = sum
    dz: D + C_SIG + 5; dw = sum dz x: D + C_SIG + 6; dx = dy (1 + gamma s) + conv3d^T(dz): dz's C_SIG + 5, 27 taps + 1,
    the final add -> c = C_SIG + 34 of the A-form"""
    npix = B * H * W
    D = csam_depth(npix)
    x, w, bias, gamma, dy = csam_data(B, H, W, seed=npix)
    X.assert_budget(S.csam_conv(dd(x).abs(), dd(w).abs()) + dd(bias).abs(), 1 / 64, "CSAM z")
    y = csam_fwd_run(x, w, bias, gamma, B, H, W)
    ref = S.csam_fwd_ref(dd(x), dd(w), bias, gamma)
    G.assert_bounded(y, ref["y"], dd(x).abs() * (1 + 0.75 * ref["s"]), C_SIG + 3, "y")
    L = lib()
    ws = nan(L.sisr_csam_bwd_workspace_bytes(B, H, W, 64) // 4)
    dx, dw, db, dg = nan(B, H, W, 64), nan(27), nan(1), nan(1)
    ok(L.sisr_csam_bwd(P(dev(x)), P(dev(w)), P(dev(bias)), P(dev(gamma)), P(dev(dy)), P(dx), P(dw), P(db), P(dg), P(ws),
                       B, H, W, 64, St()), "sisr_csam_bwd")
    rb = S.csam_bwd_ref(dd(x), dd(w), bias, gamma, dd(dy))
    mb = S.csam_bwd_ref(dd(x), dd(w), bias, gamma, dd(dy), A=True)
    G.assert_bounded(dg, rb["dgamma"].reshape(1), mb["dgamma"].reshape(1), D + C_SIG + 2, "dgamma")
    G.assert_bounded(db, rb["dbias"].reshape(1), mb["dbias"].reshape(1), D + C_SIG + 5, "dbias")
    G.assert_bounded(dw, rb["dw"], mb["dw"], D + C_SIG + 6, "dw27")
    G.assert_bounded(dx, rb["dx"], mb["dx"], C_SIG + 34, "dx")


def test_csam_ops_wrapper_and_detector():
    """ops.csam (NCHW channels-last view) equals the direct call; one x element moved at the map's last pixel breaks y's
    bound there and at no pixel outside its 3 x 3 neighbourhood"""
    B, H, W = 2, 6, 5
    x, w, bias, gamma, _ = csam_data(B, H, W, seed=5)
    yw = ops.csam(nchw_view(dev(x)), dev(w).view(1, 1, 3, 3, 3), dev(bias), dev(gamma))
    y = csam_fwd_run(x, w, bias, gamma, B, H, W)
    assert torch.equal(yw.permute(0, 2, 3, 1), y)
    xp = x.clone()
    xp[B - 1, H - 1, W - 1, 63] += 1.0
    ref = S.csam_fwd_ref(dd(x), dd(w), bias, gamma)
    bad = ~G.bound_ok(csam_fwd_run(xp, w, bias, gamma, B, H, W), ref["y"], dd(x).abs() * (1 + 0.75 * ref["s"]), C_SIG + 3)
    assert bool(bad[B - 1, H - 1, W - 1, 63]), "CSAM detector"
    assert not bool(bad[:B - 1].any()) and not bool(bad[B - 1, :H - 2].any()) and not bool(bad[B - 1, :, :W - 2].any())


# ============================================================================ 9. refusals (host-side argument checks)
def untouched(*ts):
    torch.cuda.synchronize()
    return all(bool(t.isnan().all()) for t in ts)


@pytest.mark.parametrize("C,Cr", [(96, 96), (320, 320), (128, 129)])
def test_bn_refusals(C, Cr):
    """C % 64, C > 256 (SP_MAXC), C_real > C: SISR_ERR_ARG, nothing written"""
    L = lib()
    npix = 64
    x, g = dev(torch.zeros(npix, C)), dev(torch.ones(max(C, Cr)))
    y, mean, inv, ws = nan(npix, C), nan(C), nan(C), nan(2 * 256 * 512)
    assert L.sisr_bn_act_fwd(P(x), P(y), P(g), P(g), None, None, P(mean), P(inv), npix, C, Cr, 1, 0.1, 1e-5, 0.2, P(ws),
                             ws.numel() * 4, St()) == ERR_ARG
    dx, dg, db = nan(npix, C), nan(C), nan(C)
    assert L.sisr_bn_act_bwd(P(x), P(x), P(g), P(g), P(g), P(g), P(dx), P(dg), P(db), npix, C, Cr, 0.2, P(ws), ws.numel() * 4,
                             St()) == ERR_ARG
    assert untouched(y, mean, inv, dx, dg, db)


def test_pixel_norm_spar3d_spar_combine_group_norm_refusals():
    L = lib()
    y = nan(16, 192)
    assert L.sisr_pixel_norm(P(dev(torch.zeros(16, 192))), None, P(y), 16, 192, 0, St()) == ERR_UNSUPPORTED  # C / 4 = 48
    o0, o1 = nan(12), nan(12)
    t = dev(torch.zeros(12))
    assert L.sisr_spar3d(P(t), P(t), P(t), P(o0), P(o1), 10, 1, St()) == ERR_ARG  # n % 4
    dx, dl = nan(16, 64), nan(16, 8)
    z64, z1 = dev(torch.zeros(16, 64)), dev(torch.zeros(16))
    assert L.sisr_spar_combine_bwd(P(z64), P(z64), P(z1), P(dx), P(dl), 16, 64, 6, St()) == ERR_ARG  # C_logits % 4
    xg, w = dev(torch.zeros(2, 9, 64)), dev(torch.ones(64))
    gy, gm, gi = nan(2, 9, 64), nan(64), nan(64)
    assert L.sisr_group_norm_fwd(P(xg), P(gy), P(w), P(w), P(gm), P(gi), 2, 9, 64, 62, 4, 1e-5, St()) == ERR_ARG  # 62 % 4
    gdx, gdg, gdb = nan(2, 9, 64), nan(2, 64), nan(2, 64)
    assert L.sisr_group_norm_bwd(P(xg), P(xg), P(w), P(w), P(w), P(gdx), P(gdg), P(gdb), 2, 9, 64, 62, 4, St()) == ERR_ARG
    assert untouched(y, o0, o1, dx, dl, gy, gm, gi, gdx, gdg, gdb)


@pytest.mark.parametrize("N", [7, 9, 10, 12])
def test_lam_refuses_unbuilt_map_counts(N):
    """LAM_DISPATCH builds N in {2, 3, 4, 5, 6, 8, 11}: other counts SISR_ERR_UNSUPPORTED before any launch"""
    B, chw = 1, 256
    L = lib()
    x = dev(torch.zeros(B, N, chw))
    ws = nan(max(L.sisr_lam_workspace_bytes(B, N, chw) // 4, 1))
    y, attn = nan(B, N, chw), nan(B, N, N)
    g = dev(torch.ones(1))
    assert L.sisr_lam_fwd(P(x), P(g), P(y), P(attn), P(ws), B, N, chw, St()) == ERR_UNSUPPORTED
    dx, dg = nan(B, N, chw), nan(1)
    assert L.sisr_lam_bwd(P(x), P(attn), P(g), P(x), P(dx), P(dg), P(ws), B, N, chw, St()) == ERR_UNSUPPORTED
    assert untouched(y, attn, dx, dg)


@pytest.mark.parametrize("C", [32, 128])
def test_csam_refuses_other_channel_counts(C):
    L = lib()
    x = dev(torch.zeros(1, 3, 3, C))
    w, one = dev(torch.zeros(27)), dev(torch.ones(1))
    y = nan(1, 3, 3, C)
    assert L.sisr_csam_fwd(P(x), P(w), P(one), P(one), P(y), 1, 3, 3, C, St()) == ERR_UNSUPPORTED
    dx, dw, db, dg, ws = nan(1, 3, 3, C), nan(27), nan(1), nan(1), nan(4096)
    assert L.sisr_csam_bwd(P(x), P(w), P(one), P(one), P(x), P(dx), P(dw), P(db), P(dg), P(ws), 1, 3, 3, C, St()) == ERR_UNSUPPORTED
    assert untouched(y, dx, dw, db, dg)
