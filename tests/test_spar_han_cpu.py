"""The SPARNet norm / activation / geometry references and the LAM / CSAM references (tests/_spar_han.py) on their own, no
GPU: each hand-written forward and backward formula equals float64 autograd of its PyTorch or oracle counterpart
(nn.BatchNorm2d, nn.GroupNorm, nn.InstanceNorm2d, F.normalize, nn.PReLU, nn.SELU, F.pad(mode='reflect') /
F.interpolate(mode='nearest'), O.lam_module, O.csam_module), the ties at exactly 0 (and below F.normalize's eps) included,
and the |.| (A) form of every backward bounds its value form."""
import pytest
import torch
import torch.nn.functional as F

import _exact as X
import _spar_han as S
from oracle import sisr_oracle as O


def close(got, want, what="", rel=1e-12):
    got, want = got.detach().double(), want.detach().double().reshape(got.shape)
    tol = rel * max(float(want.abs().max()), 1.0)
    assert float((got - want).abs().max()) <= tol, f"{what}: max |diff| {float((got - want).abs().max())}"


def bounded_by(v, mag, what=""):
    assert bool((v.abs() <= mag + 1e-12 * (1 + mag)).all()), f"|{what}| exceeds its A-form magnitude"


def leaf(t):
    return t.double().clone().requires_grad_(True)


def cl(t):
    """NCHW -> [B * H * W][C]"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def nchw(t, B, H, W):
    return t.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def randn(shape, seed, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale + shift


# ----------------------------------------------------------------------------- batch norm + LeakyReLU
@pytest.mark.parametrize("B,C,H,W,slope", [(2, 5, 3, 4, 0.2), (1, 3, 1, 7, 0.0), (3, 4, 2, 2, 1.0), (2, 6, 5, 1, 0.5)])
def test_batch_norm_reference_equals_autograd(B, C, H, W, slope):
    x = leaf(randn((B, C, H, W), 1, 1.5, 0.3))
    bn = torch.nn.BatchNorm2d(C, momentum=0.125).double()
    with torch.no_grad():
        bn.weight.copy_(randn(C, 2, 0.5, 1.0))
        bn.bias.copy_(randn(C, 3, 0.3))
        bn.running_mean.copy_(randn(C, 4))
        bn.running_var.copy_(randn(C, 5).abs() + 0.5)
    rm0, rv0 = bn.running_mean.clone(), bn.running_var.clone()
    y = F.leaky_relu(bn(x), slope)
    ref = S.bn_fwd_ref(cl(x), bn.weight, bn.bias, bn.eps, slope, rm0, rv0, 0.125)
    close(ref["y"], cl(y), "y")
    close(ref["rm"], bn.running_mean, "running mean")
    close(ref["rv"], bn.running_var, "running var (unbiased n / (n - 1))")
    dy = randn((B, C, H, W), 6)
    gx, gg, gb = torch.autograd.grad(y, [x, bn.weight, bn.bias], dy)
    got = S.bn_bwd_ref(cl(x), cl(dy), bn.weight, bn.bias, ref["mean"], ref["invstd"], slope)
    close(got["dx"], cl(gx), "dx")
    close(got["dgamma"], gg, "dgamma")
    close(got["dbeta"], gb, "dbeta")
    mag = S.bn_bwd_ref(cl(x), cl(dy), bn.weight, bn.bias, ref["mean"], ref["invstd"], slope, A=True)
    for k in ("dx", "dgamma", "dbeta"):
        bounded_by(got[k], mag[k], k)
    bn.eval()
    ye = F.leaky_relu(bn(x.detach()), slope)
    close(S.bn_fwd_ref(cl(x), bn.weight, bn.bias, bn.eps, slope, bn.running_mean, bn.running_var, training=False)["y"],
          cl(ye), "eval y")


@pytest.mark.parametrize("slope", [0.0, 0.2, 1.0])
def test_batch_norm_leaky_tie_at_zero(slope):
    """z exactly 0 takes the negative branch (slope), as PyTorch's LeakyReLU' does"""
    x = leaf(torch.tensor([[-1.0], [1.0], [0.0], [0.0]]).view(4, 1, 1, 1))  # mean 0, z = 0 at the last two pixels
    bn = torch.nn.BatchNorm2d(1).double()
    y = F.leaky_relu(bn(x), slope)
    dy = torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64).view(4, 1, 1, 1)
    (gx,) = torch.autograd.grad(y, [x], dy)
    ref = S.bn_fwd_ref(cl(x), bn.weight, bn.bias, bn.eps, slope)
    assert bool((ref["z"][2:] == 0).all())
    got = S.bn_bwd_ref(cl(x), cl(dy), bn.weight, bn.bias, ref["mean"], ref["invstd"], slope)
    assert torch.equal(got["dz"][:, 0], torch.tensor([slope, 2.0, 3 * slope, 4 * slope], dtype=torch.float64))
    close(got["dx"], cl(gx), "dx at the tie")


# ----------------------------------------------------------------------------- group / instance norm
@pytest.mark.parametrize("B,C,H,W,cg", [(2, 8, 3, 5, 1), (3, 8, 2, 4, 2), (1, 16, 5, 3, 4), (2, 6, 1, 1, 2)])
def test_group_norm_reference_equals_autograd(B, C, H, W, cg):
    x = leaf(randn((B, C, H, W), 7, 2.0, 0.5))
    mod = (torch.nn.InstanceNorm2d(C, affine=True) if cg == 1 else torch.nn.GroupNorm(C // cg, C)).double()
    with torch.no_grad():
        mod.weight.copy_(randn(C, 8, 0.5, 1.0))
        mod.bias.copy_(randn(C, 9, 0.3))
    y = mod(x)
    xs = x.permute(0, 2, 3, 1).reshape(B, H * W, C)
    ref = S.gn_fwd_ref(xs, mod.weight, mod.bias, cg, mod.eps)
    close(ref["y"], y.permute(0, 2, 3, 1).reshape(B, H * W, C), "y")
    dy = randn((B, C, H, W), 10)
    gx, gg, gb = torch.autograd.grad(y, [x, mod.weight, mod.bias], dy)
    dys = dy.permute(0, 2, 3, 1).reshape(B, H * W, C)
    got = S.gn_bwd_ref(xs, dys, mod.weight, ref["mean"], ref["invstd"], cg)
    close(got["dx"], gx.permute(0, 2, 3, 1).reshape(B, H * W, C), "dx")
    close(got["dgamma_b"].sum(0), gg, "dgamma (sum of the per-sample partials)")
    close(got["dbeta_b"].sum(0), gb, "dbeta")
    mag = S.gn_bwd_ref(xs, dys, mod.weight, ref["mean"], ref["invstd"], cg, A=True)
    for k in ("dx", "dgamma_b", "dbeta_b"):
        bounded_by(got[k], mag[k], k)


# ----------------------------------------------------------------------------- pixel norm
def test_pixel_norm_reference_equals_autograd_with_zero_and_tiny_pixels():
    x = randn((2, 8, 3, 3), 11)
    x[0, :, 0, 0] = 0.0          # all-zero pixel: y = 0, dx = dy / eps
    x[1, :, 2, 1] = 1e-14        # norm 2.8e-14 < eps: y = x / eps, dx = dy / eps
    x[1, :, 0, 2] = 0.0
    x[1, 3, 0, 2] = 1e-13        # one channel below eps
    x = leaf(x)
    y = F.normalize(x, p=2, dim=1)
    ref = S.pn_fwd_ref(cl(x))
    close(ref["y"], cl(y), "y")
    dy = randn((2, 8, 3, 3), 12)
    (gx,) = torch.autograd.grad(y, [x], dy)
    got = S.pn_bwd_ref(cl(x), cl(dy))
    close(got, cl(gx), "dx", rel=1e-12 / S.PN_EPS)  # dx / eps reaches 1e12 here: relative agreement
    assert torch.equal(got[0], cl(dy)[0] / S.PN_EPS) and float(ref["norm"][0]) == 0.0
    bounded_by(got, S.pn_bwd_ref(cl(x), cl(dy), A=True), "dx")


# ----------------------------------------------------------------------------- PReLU / SELU
def test_prelu_reference_equals_autograd_with_ties():
    x = randn((2, 6, 3, 4), 13)
    x[0, :, 0, 0] = 0.0
    x = leaf(x)
    mod = torch.nn.PReLU(6).double()
    with torch.no_grad():
        mod.weight.copy_(randn(6, 14, 0.3, 0.2))
    y = mod(x)
    close(S.prelu_ref(cl(x), mod.weight), cl(y), "y")
    dy = randn((2, 6, 3, 4), 15)
    gx, ga = torch.autograd.grad(y, [x, mod.weight], dy)
    got = S.prelu_bwd_ref(cl(x), cl(dy), mod.weight)
    close(got["dx"], cl(gx), "dx (x = 0: the slope branch)")
    close(got["da"], ga, "dslope = sum dy min(x, 0)")
    assert bool((got["dyx"][cl(x.detach()) > 0] == 0).all())


def test_selu_reference_equals_autograd_with_ties():
    x = randn((2, 5, 3, 3), 16, 2.0)
    x[0, :, 0, 0] = 0.0
    x[1, :, 1, 1] = torch.tensor([-1e-6, -1e-3, 1e-6, -30.0, -1e-30], dtype=torch.float64)
    x = leaf(x)
    y = torch.nn.SELU()(x)
    close(S.selu_ref(cl(x)), cl(y), "y")
    bounded_by(S.selu_ref(cl(x)), S.selu_ref(cl(x), A=True), "y")
    dy = randn((2, 5, 3, 3), 17)
    (gx,) = torch.autograd.grad(y, [x], dy)
    close(S.selu_bwd_ref(cl(x), cl(dy)), cl(gx), "dx (x = 0: the exponential branch)")
    # the small-|x| values the fp32 kernel is pinned at: relative agreement with torch's own expm1 form
    v = torch.tensor([-1e-6, -1e-3], dtype=torch.float64)
    assert torch.allclose(S.selu_ref(v.view(1, 2)).view(2), torch.selu(v), rtol=1e-15, atol=0)


# ----------------------------------------------------------------------------- attention products
@pytest.mark.parametrize("identity", [False, True])
def test_spar_combine_reference_equals_autograd(identity):
    B, C, H, W = 2, 8, 3, 4
    x, lg = leaf(randn((B, C, H, W), 18)), leaf(randn((B, 4, H, W), 19, 2.0))
    idn = leaf(randn((B, C, H, W), 20)) if identity else None
    y = x * torch.sigmoid(lg[:, :1]) + (idn if identity else 0)
    ref = S.spar_combine_ref(cl(x), cl(lg)[:, 0], cl(idn) if identity else None)
    close(ref["y"], cl(y), "y")
    dy = randn((B, C, H, W), 21)
    gx, gl = torch.autograd.grad(y, [x, lg], dy)
    got = S.spar_combine_bwd_ref(cl(dy), cl(x), ref["a"])
    close(got["dx"], cl(gx), "dx")
    close(got["dlogit"], cl(gl)[:, 0], "dlogit channel 0")
    assert float(gl[:, 1:].abs().max()) == 0.0
    mag = S.spar_combine_bwd_ref(cl(dy), cl(x), ref["a"], A=True)
    for k in ("dx", "dlogit"):
        bounded_by(got[k], mag[k], k)


def test_spar3d_reference_equals_autograd():
    x, lg, idn = leaf(randn((2, 8, 3, 3), 22)), leaf(randn((2, 8, 3, 3), 23, 3.0)), leaf(randn((2, 8, 3, 3), 24))
    y = x * torch.sigmoid(lg) + idn
    close(S.spar3d_ref(cl(x), cl(lg), cl(idn))["y"], cl(y), "y")
    dy = randn((2, 8, 3, 3), 25)
    gx, gl = torch.autograd.grad(y, [x, lg], dy)
    got = S.spar3d_bwd_ref(cl(dy), cl(x), cl(lg))
    close(got["dx"], cl(gx), "dx")
    close(got["dlogits"], cl(gl), "dlogits")
    mag = S.spar3d_bwd_ref(cl(dy), cl(x), cl(lg), A=True)
    for k in ("dx", "dlogits"):
        bounded_by(got[k], mag[k], k)


# ----------------------------------------------------------------------------- geometry
def nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("H,W,up", [(2, 2, 1), (2, 3, 2), (5, 7, 1), (4, 3, 2), (9, 2, 2)])
def test_pad_reflect_up_reference_and_adjoint_equal_autograd(H, W, up):
    x = leaf(randn((2, 4, H, W), 26))
    t = F.interpolate(x, scale_factor=up, mode="nearest") if up > 1 else x
    y = F.pad(t, (1, 1, 1, 1), mode="reflect")
    assert torch.equal(S.pad_reflect_up_ref(nhwc(x), up), nhwc(y).detach())
    dy = X.ints(y.shape, 27).double()
    (gx,) = torch.autograd.grad(y, [x], dy)
    assert torch.equal(S.pad_reflect_up_adj(nhwc(dy), H, W, up), nhwc(gx))


@pytest.mark.parametrize("Hf,Wf,stride", [(3, 3, 1), (7, 8, 2), (8, 7, 2), (6, 5, 1), (3, 4, 2)])
def test_crop_stride_reference_and_adjoint_equal_strided_conv_geometry(Hf, Wf, stride):
    """the stride-s conv over the padded map equals the stride-1 'same' conv's interior every s-th pixel: crop_stride takes
    exactly the pixels Conv2d(stride=s, no padding) centres on"""
    src = leaf(randn((2, 4, Hf, Wf), 28))
    y = src[:, :, 1:Hf - 1, 1:Wf - 1][:, :, ::stride, ::stride]
    got = S.crop_stride_ref(nhwc(src), stride)
    conv_out = F.conv2d(src.detach(), torch.ones(1, 4, 3, 3, dtype=torch.float64), stride=stride).shape[2:]
    assert got.shape[1:3] == ((Hf - 3) // stride + 1, (Wf - 3) // stride + 1) == tuple(y.shape[2:]) == tuple(conv_out)
    assert torch.equal(got, nhwc(y).detach())
    dy = X.ints(y.shape, 29).double()
    (gs,) = torch.autograd.grad(y, [src], dy)
    assert torch.equal(S.crop_stride_adj(nhwc(dy), Hf, Wf, stride), nhwc(gs))


@pytest.mark.parametrize("H,W,up", [(1, 1, 2), (3, 5, 3), (2, 2, 4), (4, 3, 1)])
def test_nearest_up_reference_and_adjoint_equal_autograd(H, W, up):
    x = leaf(randn((2, 4, H, W), 30))
    y = F.interpolate(x, scale_factor=up, mode="nearest")
    assert torch.equal(S.nearest_up_ref(nhwc(x), up), nhwc(y).detach())
    dy = X.ints(y.shape, 31).double()
    (gx,) = torch.autograd.grad(y, [x], dy)
    assert torch.equal(S.nearest_up_adj(nhwc(dy), up), nhwc(gx))


# ----------------------------------------------------------------------------- LAM / CSAM
@pytest.mark.parametrize("B,N,C,H,W", [(2, 3, 4, 2, 3), (1, 11, 8, 2, 2), (3, 2, 4, 1, 5)])
def test_lam_reference_equals_oracle_autograd(B, N, C, H, W):
    x = leaf(randn((B, N, C, H, W), 32, 0.4))
    gamma = leaf(torch.tensor([0.7]))
    y = O.lam_module({"k.gamma": gamma}, "k", x).view(B, N, C, H, W)
    ref = S.lam_fwd_ref(x.view(B, N, -1), gamma)
    close(ref["y"], y.view(B, N, -1), "y")
    dy = randn((B, N, C, H, W), 33)
    gx, gg = torch.autograd.grad(y, [x, gamma], dy)
    got = S.lam_bwd_ref(x.view(B, N, -1), ref["A"], gamma, dy.view(B, N, -1))
    close(got["dx"], gx.view(B, N, -1), "dx")
    close(got["dgamma"], gg, "dgamma")
    mag = S.lam_bwd_ref(x.view(B, N, -1), ref["A"], gamma, dy.view(B, N, -1), A=True)
    for k in ("dx", "G", "dE", "dgamma"):
        bounded_by(got[k], mag[k], k)


@pytest.mark.parametrize("B,H,W", [(2, 3, 4), (1, 1, 5), (2, 4, 1), (1, 1, 1)])
def test_csam_reference_equals_oracle_autograd(B, H, W):
    C = 6
    x = leaf(randn((B, C, H, W), 34))
    w, b, g = leaf(randn((1, 1, 3, 3, 3), 35, 0.5)), leaf(torch.tensor([0.3])), leaf(torch.tensor([0.8]))
    y = O.csam_module({"k.conv.weight": w, "k.conv.bias": b, "k.gamma": g}, "k", x)
    ref = S.csam_fwd_ref(nhwc(x), w, b, g)
    close(ref["y"], nhwc(y), "y")
    dy = randn((B, C, H, W), 36)
    gx, gw, gb, gg = torch.autograd.grad(y, [x, w, b, g], dy)
    got = S.csam_bwd_ref(nhwc(x), w, b, g, nhwc(dy))
    close(got["dx"], nhwc(gx), "dx")
    close(got["dw"], gw.view(27), "dw27 ([dc][dh][dw])")
    close(got["dbias"], gb, "dbias")
    close(got["dgamma"], gg, "dgamma")
    mag = S.csam_bwd_ref(nhwc(x), w, b, g, nhwc(dy), A=True)
    for k in ("dx", "dw", "dbias", "dgamma", "dz"):
        bounded_by(got[k], mag[k], k)
