"""The float64 references of tests/_glue.py against independent float64 statements of the same operations (no GPU).

tests/test_glue_gpu.py compares the Adam, SFTMD glue, layout and quantiser kernels with these references; here each is
checked against another formulation: torch.optim.Adam(foreach=False) in float64, float64 autograd of the four-conv SFT
layer / of torch.clamp / of F.pixel_shuffle, the oracle's BatchBlur, and tensor.to(torch.bfloat16).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _exact as X
import _glue as R
from oracle import degrade_oracle as DO


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def close(got, want, what="", rel=1e-12):
    got, want = got.detach().double(), want.detach().double().reshape(got.shape)
    tol = rel * max(float(want.abs().max()), 1.0)
    assert float((got - want).abs().max()) <= tol, f"{what}: max |diff| {float((got - want).abs().max())}"


# ----------------------------------------------------------------------------- Adam
def test_adam_reference_follows_torch_adam_over_three_steps_with_a_skipped_parameter():
    """three parameters, three steps, parameter 1 without a gradient in step 2 (torch counts its steps separately):
    parameters and both moments <= 1e-12 relative"""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    ps = [torch.nn.Parameter(rnd(n, seed=10 + n)) for n in (7, 33, 5)]
    opt = torch.optim.Adam(ps, lr=lr, betas=(b1, b2), eps=eps, foreach=False)
    mine = [dict(p=p.detach().clone(), m=torch.zeros_like(p), v=torch.zeros_like(p), t=0) for p in ps]
    for step in range(3):
        for k, p in enumerate(ps):
            if k == 1 and step == 1:
                p.grad = None
                continue
            p.grad = rnd(*p.shape, seed=100 * step + k, scale=10.0 ** (k - 2))
            s = mine[k]
            s["t"] += 1
            out = R.adam_ref(s["p"], p.grad, s["m"], s["v"], **R.adam_scalars(lr, b1, b2, eps, s["t"], rounded=False))
            mag = R.adam_ref(s["p"], p.grad, s["m"], s["v"], **R.adam_scalars(lr, b1, b2, eps, s["t"], rounded=False), A=True)
            assert all(bool((mag[n] >= out[n].abs()).all()) for n in "mvp")
            s.update(out)
        opt.step()
    for k, p in enumerate(ps):
        st = opt.state[p]
        assert int(st["step"]) == mine[k]["t"] == (2 if k == 1 else 3)
        for got, want, what in ((mine[k]["p"], p, "p"), (mine[k]["m"], st["exp_avg"], "m"), (mine[k]["v"], st["exp_avg_sq"], "v")):
            assert float(((got - want.detach()).abs() / want.detach().abs().clamp_min(1e-300)).max()) <= 1e-12, (k, what)


def test_adam_grad_scale_scales_the_gradient():
    p, g, m, v = (rnd(19, seed=s) for s in (1, 2, 3, 4))
    v = v.abs()
    sc = R.adam_scalars(1e-4, 0.9, 0.999, 1e-8, 5, rounded=False)
    a = R.adam_ref(p, g, m, v, **{**sc, "grad_scale": 0.5})
    b = R.adam_ref(p, g * 0.5, m, v, **sc)
    for n in "mvp":
        assert torch.equal(a[n], b[n])
    assert R.f32(0.1) == float(np.float32(0.1)) and R.adam_scalars(1e-4, 0.9, 0.999, 1e-8, 1)["omb2"] == float(np.float32(1 - 0.999))


# ----------------------------------------------------------------------------- SFT composition and combine
def sft_params(M, seed):
    return [rnd(*s, seed=seed + i, scale=0.2) for i, s in enumerate(R.SFT_PARAM_SHAPES(M))]


@pytest.mark.parametrize("M", [0, 1, 16, 17, 33, 64])
def test_sft_compose_reference_is_the_four_conv_layer(M):
    """two convs with the merged weights == the four convs of StandardSft on cat(x, maps); split is the inverse and reads
    nothing outside the real blocks"""
    prm = sft_params(M, 20 + M)
    mw1, mb1, aw1, ab1, mw2, mb2, aw2, ab2 = prm
    WA, bA, WB, bB = merged = R.sft_compose_ref(prm, M)
    cat = rnd(2, 64 + M, 5, 6, seed=3)
    cat128 = F.pad(cat, (0, 0, 0, 0, 0, 64 - M))
    t = F.leaky_relu(F.conv2d(cat128, WA, bA, padding=1), 0.2)
    y2 = F.conv2d(t, WB, bB, padding=1)
    mul = F.conv2d(F.leaky_relu(F.conv2d(cat, mw1, mb1, padding=1), 0.2), mw2, mb2, padding=1)
    add = F.conv2d(F.leaky_relu(F.conv2d(cat, aw1, ab1, padding=1), 0.2), aw2, ab2, padding=1)
    close(y2[:, :64], mul, "mul branch")
    close(y2[:, 64:], add, "add branch")
    za, zb = R.sft_structural(M)
    assert bool((WA[za] == 0).all()) and bool((WB[zb] == 0).all()) and not bool(torch.signbit(WA[za]).any())
    assert int((~za).sum()) == 2 * mw1.numel() and int((~zb).sum()) == 2 * mw2.numel()
    poisoned = (torch.where(za, torch.full_like(WA, float("nan")), WA), bA, torch.where(zb, torch.full_like(WB, float("nan")), WB), bB)
    for got, want in zip(R.sft_split_ref(poisoned, M), prm):
        assert torch.equal(got, want)


@pytest.mark.parametrize("relu", [False, True])
def test_sft_combine_references_follow_autograd(relu):
    npix = 37
    x, y2, dout = rnd(npix, 64, seed=1), rnd(npix, 128, seed=2, scale=3.0), rnd(npix, 64, seed=3)
    y2[3, 64:] = -(x[3] * torch.sigmoid(y2[3, :64]))  # pre == 0 or its rounding residue
    xr, yr = x.clone().requires_grad_(True), y2.clone().requires_grad_(True)
    pre = xr * torch.sigmoid(yr[:, :64]) + yr[:, 64:]
    out = F.relu(pre) if relu else pre
    out.backward(dout)
    f = R.sft_combine_fwd_ref(x, y2, relu)
    close(f["out"], out, "out")
    b = R.sft_combine_bwd_ref(dout, x, y2, relu)
    close(b["dx"], xr.grad, "dx")
    close(b["dm"], yr.grad[:, :64], "dm")
    close(b["da"], yr.grad[:, 64:], "da")
    mag = R.sft_combine_bwd_ref(dout, x, y2, relu, A=True)
    assert all(bool((mag[n] >= b[n].abs()).all()) for n in ("dx", "dm", "da"))
    assert bool((R.sft_combine_fwd_ref(x, y2, relu, A=True)["out"] >= f["out"].abs()).all())
    z = torch.zeros(1, 64, dtype=torch.float64)
    assert bool((R.sft_combine_bwd_ref(z + 1, z, torch.zeros(1, 128, dtype=torch.float64), True)["da"] == 0).all())  # pre == 0


def test_map64_and_clamp_references_follow_torch():
    a, b = rnd(23, 64, seed=4), rnd(23, 64, seed=5)
    a[0, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0], dtype=torch.float64)
    a32, b32 = a.float().double(), b.float().double()
    ar = a32.clone().requires_grad_(True)
    assert torch.equal(R.map64_ref(0, a32), a32) and torch.equal(R.map64_ref(1, a32, b32), a32 + b32)
    assert torch.equal(R.map64_ref(4, a32, b32), a32 * b32) and torch.equal(R.map64_ref(7, a32, b32[:, 0]), a32 * b32[:, :1])
    close(R.map64_ref(2, a32), F.leaky_relu(a32, X.SLOPE32), "leaky", rel=2.0 ** -24)
    F.leaky_relu(ar, X.SLOPE32).backward(b32)
    close(R.map64_ref(3, a32, b32), ar.grad, "leaky backward", rel=2.0 ** -24)
    assert torch.equal(R.map64_ref(5, a32), F.relu(a32))
    ar.grad = None
    F.relu(ar).backward(b32)
    assert torch.equal(R.map64_ref(6, a32, b32), ar.grad)
    assert bool((R.map64_ref(6, a32, b32)[0, :2] == 0).all()) and bool((R.map64_ref(3, a32, b32)[0, :2].abs() < b32[0, :2].abs()).all())
    v = torch.tensor([-1.0, -0.0, 0.0, 2.0 ** -149, 0.5, 1 - 2.0 ** -24, 1.0, 1 + 2.0 ** -23, 2.0], dtype=torch.float64)
    vr = v.clone().requires_grad_(True)
    g = rnd(9, seed=6)
    torch.clamp(vr, 0.0, 1.0).backward(g)
    assert torch.equal(R.clamp01_ref(v), torch.clamp(v, 0.0, 1.0)) and torch.equal(R.clamp01_bwd_ref(v, g), vr.grad)
    assert R.clamp01_bwd_ref(v, g).ne(0).tolist() == [False, True, True, True, True, True, True, False, False]


# ----------------------------------------------------------------------------- layout
@pytest.mark.parametrize("C,r,Cp", [(1, 1, 4), (3, 2, 12), (3, 2, 64), (1, 3, 12), (3, 4, 64)])
def test_shuffle_references_follow_pixel_shuffle_and_its_autograd(C, r, Cp):
    B, H, W = 2, 5, 7
    y = rnd(B, H, W, Cp, seed=7).requires_grad_(True)
    want = F.pixel_shuffle(y.permute(0, 3, 1, 2)[:, :C * r * r], r)
    close(R.shuffle_rgb_ref(y.detach(), C, r), want, "shuffle")
    g = rnd(*want.shape, seed=8)
    want.backward(g)
    assert torch.equal(R.shuffle_rgb_adjoint_ref(g, C, r, Cp), y.grad)
    assert bool((R.shuffle_rgb_adjoint_ref(g, C, r, Cp)[..., C * r * r:] == 0).all())
    x = rnd(B, H, W, C * r * r, seed=9)
    out = R.pixel_shuffle_cl_ref(x, C, r)
    for b, h, w, c, dy, dx in ((0, 0, 0, 0, 0, 0), (1, 4, 6, C - 1, r - 1, r - 1), (1, 2, 3, 0, r - 1, 0)):
        assert out[b, r * h + dy, r * w + dx, c] == x[b, h, w, c * r * r + dy * r + dx]
    assert torch.equal(R.pixel_unshuffle_cl_ref(out, C, r), x)


def test_pad_references_are_plain_indexing():
    x = rnd(2, 13, 5, 7, seed=10)
    y = R.nchw_to_nhwc_pad_ref(x, 64)
    assert y.shape == (2, 5, 7, 64) and bool((y[..., 13:] == 0).all())
    for b, c, h, w in ((0, 0, 0, 0), (1, 12, 4, 6), (1, 5, 2, 3)):
        assert y[b, h, w, c] == x[b, c, h, w]
    w = rnd(5, 7, 9, seed=11)
    wp = R.pad_oihw_ref(w, 8, 12)
    assert wp.shape == (8, 12, 9) and float(wp.abs().sum()) == float(w.abs().sum()) and torch.equal(wp, F.pad(w, (0, 0, 0, 5, 0, 3)))
    assert torch.equal(R.crop_oihw_ref(wp, 5, 7), w)


# ----------------------------------------------------------------------------- bf16 rounding
def test_bf16_reference_is_round_to_nearest_even_on_every_pattern():
    x = R.bf16_patterns()
    assert x.numel() == 5 * 65536
    bits, isnan = R.bf16_rne_ref(x)
    assert torch.equal(isnan, x.isnan())
    torch_bits = R.bf16_bits(x.to(torch.bfloat16))
    assert torch.equal(bits[~isnan], torch_bits[~isnan])
    assert bool(R.bf16_is_nan(bits[isnan]).all()) and bool(R.bf16_is_nan(torch_bits[isnan]).all())
    assert torch.equal(bits[isnan] >> 15, R.f32_bits(x)[isnan] >> 31)
    fin = ~isnan
    assert torch.equal(R.bf16_bits(X.bf16_of(x[fin].double())), bits[fin])

    def one(pattern):
        return int(R.bf16_rne_ref(torch.tensor([pattern], dtype=torch.int64).to(torch.int32).view(torch.float32))[0])
    assert one(0x3F808000) == 0x3F80 and one(0x3F818000) == 0x3F82  # ties to even, both directions
    assert one(0x3F807FFF) == 0x3F80 and one(0x3F808001) == 0x3F81
    assert one(0x3FFF8000) == 0x4000  # carry into the exponent
    assert one(0x7F7F8000) == 0x7F80 and one(0x7F7F7FFF) == 0x7F7F  # the largest finite values round to infinity
    assert one(0x7F800000) == 0x7F80 and one(0x00008000) == 0x0000 and one(0x00018000) == 0x0002


# ----------------------------------------------------------------------------- blur and quantisers
@pytest.mark.parametrize("H,W,l", [(11, 11, 21), (33, 40, 21), (9, 12, 8), (5, 5, 8), (1, 1, 1), (20, 17, 15)])
def test_blur_reference_follows_the_oracle_batch_blur(H, W, l):
    x, k = rnd(3, H, W, seed=H + l).abs(), rnd(l, l, seed=l).abs()
    k = k / k.sum()
    close(R.blur_ref(x, k), DO.batch_blur(x[None], k)[0], f"blur {H}x{W} l={l}")
    hot = torch.zeros(l, l, dtype=torch.float64)
    hot[0, l - 1] = 1.0  # a one-hot kernel is a shifted copy of the reflected image
    assert torch.equal(R.blur_ref(x, hot), DO.batch_blur(x[None], hot)[0])
    assert bool((R.blur_mag(x, -k) >= R.blur_ref(x, -k).abs()).all())


def test_quantiser_references_truncate_as_fp32_does():
    v = (torch.arange(0, 257, dtype=torch.float64) / 256).float()
    assert torch.equal(R.quant_ref(v), v.mul(255).byte())
    k = (torch.arange(0, 256, dtype=torch.float32) / 255)
    near = torch.cat([k, torch.nextafter(k, torch.ones(())), torch.nextafter(k, -torch.ones(()))]).clamp(0, 1)
    assert torch.equal(R.quant_ref(near), near.mul(255).byte())
    g = torch.Generator().manual_seed(3)
    blur, noise = torch.rand(4099, generator=g), torch.randn(4099, generator=g)
    sigma = R.f32(0.0731)
    got, v = R.noise_quant_ref(blur, noise, sigma)
    want = (noise * torch.tensor(sigma, dtype=torch.float32) + blur).clamp(0, 1)
    assert torch.equal(v.float(), want) and torch.equal(got, want.mul(255).byte())
    in64 = X.fp32_round(X.fp32_round(noise.double() * sigma) + blur.double()).clamp(0, 1)  # no double rounding on this data
    assert torch.equal(in64, v)
