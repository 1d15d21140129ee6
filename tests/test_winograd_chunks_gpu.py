"""Chunked Winograd F(2x2,3x3) form of the fused-shuffle upsampler convs (conv3x3_c64_w4_kernel<..., CHUNKS>): the 64 -> 64 r^2
conv stored through view_shuffle and its 64 r^2 -> 64 input gradient read through it.  Packing bit for bit against the numpy
restatement, both launches forced on ragged shapes against float64 ATen and the direct form, exact dyadic data, one-hot
weights, the selection rule, determinism and ops.conv3x3(shuffle=2) under autograd.

Bounds.  Forward: the 64 -> 64 form's (tests/test_winograd_gpu.py): max_rel <= 3 x the direct form's + 1e-7 and inside
close(2e-5, 2e-6).  Input gradient: its reduction is r^2 times longer, so no absolute bound is fixed; the direct form's
max_rel against float64 is measured on the same inputs and 3 x that (+ 1e-7) is the bound.
Measured max_rel on the MI355X, Winograd / direct (ratio); the direct form's k-ordered chain of 576 r^2 terms rounds more
than the Winograd form's 16 shorter sums, so every ratio is below one:
    forward, with bias    r=2: 2.5e-7 / 9.9e-7 (0.26), 2.4e-7 / 9.8e-7 (0.24), 3.0e-7 / 1.3e-6 (0.23), 3.6e-7 / 1.5e-6 (0.24)
                          r=3: 2.5e-7 / 9.9e-7 (0.26), 2.9e-7 / 1.2e-6 (0.23)
    forward, no bias      r=2: 3.2e-7 / 7.2e-7 (0.45), 3.4e-7 / 8.7e-7 (0.39), 3.7e-7 / 9.6e-7 (0.39), 4.8e-7 / 1.2e-6 (0.39)
                          r=3: 3.1e-7 / 7.1e-7 (0.43), 3.7e-7 / 1.4e-6 (0.27)
    input gradient        r=2: 3.0e-7 / 1.2e-6 (0.24), 3.6e-7 / 2.1e-6 (0.17), 2.9e-7 / 2.0e-6 (0.15), 3.1e-7 / 2.3e-6 (0.13)
                          r=3: 3.5e-7 / 2.6e-6 (0.14), 3.3e-7 / 3.0e-6 (0.11)
    conv3x3(shuffle=2) at (3, 192, 256): y 3.1e-7 / 1.7e-6, dx 3.1e-7 / 2.5e-6, dw 8.2e-7 / 8.7e-7, db 1.7e-7 / 1.7e-7
(shapes in the order of SHAPES).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sisr_amd
from test_winograd_chunks_cpu import BLOCK, chunked_u

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
hip = sisr_amd.hip
DEV = "cuda:0"
CL = torch.channels_last
DIRECT, WINO = 7, ops.SELECT_WINOGRAD_FORCE

SHAPES = {2: [(1, 13, 9), (2, 16, 16), (3, 37, 70), (3, 100, 250)], 3: [(1, 13, 9), (3, 37, 70)]}
CASES = [(r, *s) for r in (2, 3) for s in SHAPES[r]]


def close(got, want, rtol, atol, msg=""):
    got = got.detach().double().cpu().numpy()
    want = want.detach().double().cpu().numpy()
    scale = max(1.0, float(np.abs(want).max()))
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol * scale, err_msg=msg)


def max_rel(got, want):
    want = want.detach().double().cpu()
    return float((got.detach().double().cpu() - want).abs().max()) / max(1.0, float(want.abs().max()))


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def ints(*shape, seed, lo, hi, step=1):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(lo, hi + 1, shape, generator=g) * step).float()


def dev4(t):
    return t.to(DEV).contiguous(memory_format=CL)


def packed_with_transform(w, r):
    """(forward, input-gradient) packing of one weight by the step-level packing launch, transform included."""
    plan = ops._PackPlan([(w, r)], w.device)
    plan.run()
    ops.invalidate_packs()
    return plan.slices[0]


def fwd(x, pf, bias, r, B, H, W, select):
    """64 -> 64 r^2 conv of x (B, 64, H, W), stored through PixelShuffle(r) into a NaN-filled (B, 64, rH, rW) map."""
    y = torch.full((B, 64, r * H, r * W), float("nan"), device=DEV).contiguous(memory_format=CL)
    ops.conv_c64(x, hip.view_plain(H, W, 64), pf, bias, (r * r, 1), y, hip.view_shuffle(H, W, r), B, H, W, 64, 64 * r * r,
                 select=select)
    return y


def dgrad(dy, pd, r, B, H, W, select, alpha=1.0):
    """64 r^2 -> 64 input gradient of dy (B, 64, rH, rW), read through the shuffle view, into a NaN-filled (B, 64, H, W) map."""
    dx = torch.full((B, 64, H, W), float("nan"), device=DEV).contiguous(memory_format=CL)
    ops.conv_c64(dy, hip.view_shuffle(H, W, r), pd, None, (1, 64), dx, hip.view_plain(H, W, 64), B, H, W, 64 * r * r, 64,
                 alpha=alpha, select=select)
    return dx


def ref_fwd(x, w, b, r):
    return F.pixel_shuffle(F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=1), r)


def ref_dgrad(dy, w, r, alpha=1.0):
    return alpha * F.conv_transpose2d(F.pixel_unshuffle(dy.double(), r), w.double(), padding=1)


class env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop(self.name, None)
        else:
            os.environ[self.name] = self.prev


# ------------------------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("r", [2, 3])
def test_packing_matches_the_restatement(r):
    rr = r * r
    w = rnd(64 * rr, 64, 3, 3, seed=1, scale=0.05).to(DEV)
    w1 = rnd(64, 64, 3, 3, seed=2, scale=0.05).to(DEV)
    plan = ops._PackPlan([(w1, 1), (w, r), (w1, 1)], w.device)
    plan.run()
    ops.invalidate_packs()
    alone = ops._PackPlan([(w1, 1)], w.device)
    alone.run()
    ops.invalidate_packs()
    direct = 64 * 64 * rr * 9
    pf, pd = plan.slices[1]
    assert pf.numel() == pd.numel() == direct + rr * ops.WINOGRAD_FLOATS and ops.WINOGRAD_FLOATS == BLOCK
    qf, qd = torch.empty(direct, device=DEV), torch.empty(direct, device=DEV)
    hip.check(hip.lib().sisr_pack_conv3x3_both(hip.ptr(w), hip.ptr(qf), hip.ptr(qd), 64 * rr, 64, r, hip.stream()), "pack_both")
    assert torch.equal(pf[:direct], qf) and torch.equal(pd[:direct], qd)
    wn = w.cpu().numpy()
    assert np.array_equal(pf[direct:].cpu().numpy(), chunked_u(wn, r, dgrad=False))
    assert np.array_equal(pd[direct:].cpu().numpy(), chunked_u(wn, r, dgrad=True))
    for k in (0, 2):  # the 64 -> 64 jobs around it: the bytes of a plan of their own
        assert torch.equal(plan.slices[k][0], alone.slices[0][0]) and torch.equal(plan.slices[k][1], alone.slices[0][1])
    w1n = w1.cpu().numpy()
    assert np.array_equal(alone.slices[0][0][64 * 64 * 9:].cpu().numpy(), chunked_u(w1n, 1, dgrad=False))
    assert np.array_equal(alone.slices[0][1][64 * 64 * 9:].cpu().numpy(), chunked_u(w1n, 1, dgrad=True))


# ----------------------------------------------------------------------------------------------------- float64 ATen
@pytest.mark.parametrize("r,B,H,W", CASES)
def test_forward_against_float64(r, B, H, W):
    rr = r * r
    x, w, b = rnd(B, 64, H, W, seed=10), rnd(64 * rr, 64, 3, 3, seed=11, scale=0.05), rnd(64 * rr, seed=12)
    xd, bd = dev4(x), b.to(DEV)
    pf, _ = packed_with_transform(w.to(DEV), r)
    for bias, bias_d in ((b, bd), (None, None)):
        want = ref_fwd(x, w, bias, r)
        yw, yd = fwd(xd, pf, bias_d, r, B, H, W, WINO), fwd(xd, pf, bias_d, r, B, H, W, DIRECT)
        ew, ed = max_rel(yw, want), max_rel(yd, want)
        print(f"forward r={r} {(B, H, W)} bias={bias is not None}: winograd {ew:.3e} direct {ed:.3e} ratio {ew / ed:.2f}")
        close(yw, want, 2e-5, 2e-6, "winograd vs float64")
        assert ew <= 3 * ed + 1e-7, (ew, ed)
        assert not torch.equal(yw, yd), "the chunked form did not engage"


@pytest.mark.parametrize("r,B,H,W", CASES)
def test_input_gradient_against_float64(r, B, H, W):
    rr = r * r
    dy, w = rnd(B, 64, r * H, r * W, seed=20), rnd(64 * rr, 64, 3, 3, seed=21, scale=0.05)
    dyd = dev4(dy)
    _, pd = packed_with_transform(w.to(DEV), r)
    want = ref_dgrad(dy, w, r, 0.3)
    gw, gd = dgrad(dyd, pd, r, B, H, W, WINO, alpha=0.3), dgrad(dyd, pd, r, B, H, W, DIRECT, alpha=0.3)
    ew, ed = max_rel(gw, want), max_rel(gd, want)
    print(f"dgrad r={r} {(B, H, W)}: winograd {ew:.3e} direct {ed:.3e} ratio {ew / ed:.2f}")
    assert ew <= 3 * ed + 1e-7, (ew, ed)
    assert not torch.equal(gw, gd), "the chunked form did not engage"


# ------------------------------------------------------------------------------------------------------ exact data
@pytest.mark.parametrize("r,B,H,W", [(2, 3, 37, 70), (3, 1, 13, 9)])
def test_exact_on_dyadic_data(r, B, H, W):
    """Small integer maps, weights that are multiples of 4: every Winograd intermediate is an exact fp32 integer, so both
    launches equal float64 bit for bit."""
    rr = r * r
    x = ints(B, 64, H, W, seed=30, lo=-3, hi=3)
    dy = ints(B, 64, r * H, r * W, seed=31, lo=-3, hi=3)
    w = ints(64 * rr, 64, 3, 3, seed=32, lo=-2, hi=2, step=4)
    b = ints(64 * rr, seed=33, lo=-5, hi=5)
    pf, pd = packed_with_transform(w.to(DEV), r)
    y = fwd(dev4(x), pf, b.to(DEV), r, B, H, W, WINO)
    assert torch.equal(y.double().cpu(), ref_fwd(x, w, b, r))
    dx = dgrad(dev4(dy), pd, r, B, H, W, WINO, alpha=0.5)
    assert torch.equal(dx.double().cpu(), ref_dgrad(dy, w, r, 0.5))


def _one_hot_set(r):
    """(o, i, tap): every chunk q = o % r^2, both 32-channel halves of o // r^2 and of i, all nine taps."""
    rr = r * r
    return [((7, 45)[t % 2] * rr + t % rr, (3, 60)[(t // 2) % 2], t) for t in range(9)]


@pytest.mark.parametrize("r", [2, 3])
def test_one_hot_weights(r):
    """One nonzero weight (o, i, tap): the forward output is input channel i shifted by the tap at exactly the shuffled position
    of channel o, the input gradient is the un-shuffled dy channel o shifted the other way in channel i; zero elsewhere."""
    rr = r * r
    B, H, W = 1, 13, 37
    x = ints(B, 64, H, W, seed=40, lo=0, hi=1)
    dy = ints(B, 64, r * H, r * W, seed=41, lo=0, hi=1)
    xd, dyd = dev4(x), dev4(dy)
    xp = F.pad(x, (1, 1, 1, 1))
    dyu = F.pad(F.pixel_unshuffle(dy, r), (1, 1, 1, 1))
    halves = set()
    for o, i, t in _one_hot_set(r):
        kh, kw = divmod(t, 3)
        n, q = divmod(o, rr)
        halves.add((q, n >= 32, i >= 32))
        w = torch.zeros(64 * rr, 64, 3, 3)
        w[o, i, kh, kw] = 1.0
        pf, pd = packed_with_transform(w.to(DEV), r)
        want = torch.zeros(B, 64, r * H, r * W)
        want[:, n, q // r::r, q % r::r] = xp[:, i, kh:kh + H, kw:kw + W]
        assert torch.equal(fwd(xd, pf, None, r, B, H, W, WINO).cpu(), want), (o, i, t)
        want = torch.zeros(B, 64, H, W)
        want[:, i] = dyu[:, o, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W]
        assert torch.equal(dgrad(dyd, pd, r, B, H, W, WINO).cpu(), want), (o, i, t)
    assert {q for q, _, _ in halves} == set(range(rr))
    assert {h for _, h, _ in halves} == {False, True} == {h for _, _, h in halves}


# ------------------------------------------------------------------------------------- selection and determinism
def test_chunked_form_is_deterministic():
    r, B, H, W = 2, 3, 37, 70
    w, b = rnd(256, 64, 3, 3, seed=50, scale=0.05).to(DEV), rnd(256, seed=51).to(DEV)
    pf, pd = packed_with_transform(w, r)
    x, dy = dev4(rnd(B, 64, H, W, seed=52)), dev4(rnd(B, 64, r * H, r * W, seed=53))
    assert torch.equal(fwd(x, pf, b, r, B, H, W, WINO), fwd(x, pf, b, r, B, H, W, WINO))
    assert torch.equal(dgrad(dy, pd, r, B, H, W, WINO), dgrad(dy, pd, r, B, H, W, WINO))


@pytest.mark.parametrize("B,H,W", [(3, 192, 256), (2, 256, 256)])
def test_selection_rule(B, H, W):
    """Default select on a transform-carrying packing: the direct bits at <= 8 x 128^2 output pixels per launch, the chunked
    form's above; SISR_CONV_WINOGRAD=0 gives the direct bits; a packing without the transform never selects the form."""
    r = 2
    w, b = rnd(256, 64, 3, 3, seed=60, scale=0.05).to(DEV), rnd(256, seed=61).to(DEV)
    pf, pd = packed_with_transform(w, r)
    qf, qd = ops.pack_pair(w, r)
    x, dy = dev4(rnd(B, 64, H, W, seed=62)), dev4(rnd(B, 64, r * H, r * W, seed=63))
    above = B * H * W > 8 * 128 * 128
    runs = ((lambda pk, s: fwd(x, pk, b, r, B, H, W, s), pf, qf), (lambda pk, s: dgrad(dy, pk, r, B, H, W, s, alpha=0.3), pd, qd))
    for run, pk, plain in runs:
        y0, y7, yw = run(pk, 0), run(pk, DIRECT), run(pk, WINO)
        assert not torch.equal(yw, y7)
        assert torch.equal(y0, yw if above else y7)
        with env("SISR_CONV_WINOGRAD", "0"):
            assert torch.equal(run(pk, 0), y7)
        assert torch.equal(run(plain, 0), y7)


def test_other_channel_counts_are_refused():
    """Select 11 / 12 name the transform behind the packing: only 64 -> 64, 64 -> 64 r^2 and 64 r^2 -> 64 carry one."""
    B, H, W = 1, 8, 32
    for cin, cout in ((64, 128), (128, 64), (64, 512), (128, 128), (256, 256)):
        x = dev4(rnd(B, cin, H, W, seed=80))
        pk = torch.zeros(cin * cout * 9 + (cin // 64) * (cout // 64) * ops.WINOGRAD_FLOATS, device=DEV)
        y = torch.full((B, cout, H, W), float("nan"), device=DEV).contiguous(memory_format=CL)
        for sel in (ops.SELECT_WINOGRAD, WINO):
            with pytest.raises(RuntimeError):
                ops.conv_c64(x, hip.view_plain(H, W, cin), pk, None, (1, 64), y, hip.view_plain(H, W, cout), B, H, W, cin, cout,
                             select=sel)
        torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------- module level
def test_conv3x3_shuffle_under_autograd():
    """ops.conv3x3(x, w, b, shuffle=2) at (3, 192, 256) on the step-level packing: y, dx, dw and db against float64 autograd,
    the Winograd run at most 3 x as far from it as the direct run (+ 1e-7), y also inside the forward's tolerance."""
    r, B, H, W = 2, 3, 192, 256
    x, w, b = rnd(B, 64, H, W, seed=70), rnd(256, 64, 3, 3, seed=71, scale=0.05), rnd(256, seed=72)
    cot = rnd(B, 64, r * H, r * W, seed=73)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    ref = F.pixel_shuffle(F.conv2d(x64, w64, b64, padding=1), r)
    want = (ref.detach(),) + torch.autograd.grad(ref, (x64, w64, b64), cot.double())
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    plan = ops._PackPlan([(wd, r)], wd.device)
    got = {}
    try:
        for wino in ("1", "0"):
            with env("SISR_CONV_WINOGRAD", wino):
                plan.run()
                y = ops.conv3x3(xd, wd, bd, shuffle=r)
                got[wino] = (y.detach(),) + torch.autograd.grad(y, (xd, wd, bd), cot.to(DEV))
    finally:
        ops.invalidate_packs()
    assert not torch.equal(got["1"][0], got["0"][0]) and not torch.equal(got["1"][1], got["0"][1]), "the chunked form did not engage"
    close(got["1"][0], want[0], 2e-5, 2e-6, "y")
    for name, gw, gd, wt in zip(("y", "dx", "dw", "db"), got["1"], got["0"], want):
        ew, ed = max_rel(gw, wt), max_rel(gd, wt)
        print(f"conv3x3 shuffle=2 {name}: winograd {ew:.3e} direct {ed:.3e}")
        assert ew <= 3 * ed + 1e-7, (name, ew, ed)
