"""The float64 references of tests/_san.py against float64 autograd of the oracle and of PyTorch (no GPU).

tests/test_san_kernels_gpu.py compares the SAN kernels with these references; here each is checked against an independent
statement of the same operation: the oracle's _CovPool / _SqrtmNS autograd Functions (iterations 2, 3 and 5, the saved
iterates included), torch.softmax attention, F.max_pool2d's backward on windows with 2-, 3- and 4-way ties and +0 / -0,
and the oracle's whole non-local block per attention domain, forward and every gradient.
"""
import pytest
import torch
import torch.nn.functional as F

import _san as S
from oracle import sisr_oracle as O

TOL = dict(rtol=1e-11, atol=1e-12)


def rnd(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def same(a, b, what, **kw):
    torch.testing.assert_close(a, b, **(kw or TOL), msg=lambda m: f"{what}: {m}")


@pytest.mark.parametrize("B,H,W", [(2, 3, 3), (1, 13, 9), (3, 8, 8)])
def test_covpool_and_its_backward_follow_the_oracle(B, H, W):
    x = (rnd(B, 64, H, W, seed=1) + 0.7).requires_grad_(True)
    cov = O._CovPool.apply(x)
    rows = x.detach().permute(0, 2, 3, 1).reshape(B, H * W, 64)
    mean = rows.mean(1)
    same(S.covpool_ref(rows, mean), cov.detach(), "covpool")
    same(S.covpool_sum_ref(rows, mean) / (H * W), cov.detach(), "covpool sum")
    assert bool((S.covpool_ref(rows, mean, A=True) >= S.covpool_ref(rows, mean).abs()).all())
    G, dy, gate = rnd(B, 64, 64, seed=2), rnd(B, H * W, 64, seed=3), rnd(B, 64, seed=4)
    (gx,) = torch.autograd.grad((cov * G).sum(), x)
    want = gx.permute(0, 2, 3, 1).reshape(B, H * W, 64) + dy * gate[:, None, :]
    got = S.soca_bwd_apply_ref(dy, gate, rows, mean, G + G.transpose(1, 2))
    same(got, want, "soca_bwd_apply")
    assert bool((S.soca_bwd_apply_ref(dy, gate, rows, mean, G + G.transpose(1, 2), A=True) >= got.abs()).all())


class _Ctx:
    def save_for_backward(self, *t):
        self.saved = t


@pytest.mark.parametrize("iters", [2, 3, 5])
@pytest.mark.parametrize("r", [None, 2, 8])
def test_sqrtm_forward_backward_and_saved_iterates_follow_the_oracle(iters, r):
    B = 2
    x = S.correlated_maps(B, 13 * 9, r, 0.03, seed=5).double()
    cov = S.covpool_ref(x, x.mean(1))
    ctx = _Ctx()
    out = O._SqrtmNS.forward(ctx, cov, iters)
    _, _, last, tr, ys, zs = ctx.saved
    f = S.sqrtm_fwd_ref(cov, iters)
    assert f["Y"].shape == (B, iters - 1, 64, 64) and f["Z"].shape == (B, iters - 1, 64, 64)
    same(f["trace"], tr, "trace")
    same(f["Y"], ys, "Y_i")
    same(f["Z"], zs, "Z_i")
    same(f["last"], last, "last")
    same(f["pooled"], out.mean(dim=1), "pooled")
    covg = cov.clone().requires_grad_(True)
    cot = rnd(B, 64, seed=6)
    (g,) = torch.autograd.grad((O._SqrtmNS.apply(covg, iters).mean(dim=1) * cot).sum(), covg)
    want = g + g.transpose(1, 2)
    same(S.sqrtm_bwd_ref(cov, iters, cot), want, "G + G^T", rtol=1e-9, atol=1e-9 * float(want.abs().max()))


def test_sqrtm_reference_in_fp32_is_the_same_formula():
    """dt=float32 evaluates the same steps in fp32: close to float64, not equal to it"""
    x = S.correlated_maps(1, 400, None, 0, seed=7)
    cov = S.covpool_ref(x, x.mean(1)).float()
    a, b = S.sqrtm_fwd_ref(cov, 5), S.sqrtm_fwd_ref(cov, 5, dt=torch.float32)
    assert b["pooled"].dtype == torch.float32
    err = float((b["pooled"].double() - a["pooled"]).abs().max() / a["pooled"].abs().max())
    assert 0 < err < 1e-4, err


@pytest.mark.parametrize("nb,nq,nk,scale", [(2, 30, 6, 1.0), (1, 7, 1, 1.0), (1, 40, 77, 4.0)])
def test_attention_follows_torch_softmax(nb, nq, nk, scale):
    th, ph, g = (rnd(nb, nq, 8, seed=8, scale=scale).requires_grad_(True), rnd(nb, nk, 8, seed=9).requires_grad_(True),
                 rnd(nb, nk, 8, seed=10).requires_grad_(True))
    dy = rnd(nb, nq, 8, seed=11)
    s = th @ ph.transpose(1, 2)
    y = torch.softmax(s, dim=-1) @ g
    gth, gph, gg = torch.autograd.grad((y * dy).sum(), (th, ph, g))
    f, b = S.attn_fwd_ref(th, ph, g), S.attn_bwd_ref(th, ph, g, dy)
    same(f["y"], y.detach(), "y")
    same(f["lse"], torch.logsumexp(s.detach(), -1), "lse")
    same(b["dtheta"], gth, "dtheta", rtol=1e-9, atol=1e-11)
    same(b["dphi"], gph, "dphi", rtol=1e-9, atol=1e-11)
    same(b["dg"], gg, "dg")
    same(b["dsum"], (dy * y.detach()).sum(-1), "dsum")


# B, H, W, y0, x0, hq, wq, nqy, nqx
DOMAINS = [(2, 5, 7, 0, 0, 5, 7, 1, 1), (1, 6, 8, 0, 0, 3, 4, 2, 2), (2, 5, 7, 2, 3, 3, 4, 1, 1), (1, 5, 7, 0, 3, 2, 4, 1, 1),
           (1, 2, 2, 0, 0, 2, 2, 1, 1)]


def test_domain_pixels_enumerates_rectangles_in_b_iy_ix_order():
    pix = S.domain_pixels((2, 6, 8, 0, 0, 3, 4, 2, 2))
    assert pix.shape == (8, 3, 4)
    assert pix[0, 0, 0] == 0 and pix[1, 0, 0] == 4 and pix[2, 0, 0] == 3 * 8 and pix[4, 0, 0] == 48 and pix[3, 2, 3] == 47
    assert sorted(pix.reshape(-1).tolist()) == list(range(96))


@pytest.mark.parametrize("dom", DOMAINS)
def test_tie_routing_follows_max_pool2d_backward(dom):
    B, H, W, y0, x0, hq, wq, nqy, nqx = dom
    npix = B * H * W
    proj = S.tie_values((npix, 24), seed=12).double()
    if hq * wq >= 12:
        counts, mixed = S.tie_census(proj, dom)
        assert all(c > 0 for c in counts) and mixed > 0, (counts, mixed)
    pix = S.domain_pixels(dom)
    nd, nk = pix.shape[0], (hq // 2) * (wq // 2)
    v = proj[pix.reshape(-1)].view(nd, hq, wq, 24)[..., 8:].permute(0, 3, 1, 2).clone().requires_grad_(True)
    pooled = F.max_pool2d(v, 2)
    f = S.split_pool_fwd_ref(proj, dom)
    want = pooled.detach().permute(0, 2, 3, 1).reshape(nd, nk, 16)
    assert torch.equal(f["phi"], want[..., :8]) and torch.equal(f["g"], want[..., 8:])
    assert torch.equal(f["theta"], proj[pix.reshape(-1)].view(nd, hq * wq, 24)[..., :8])
    dth, dph, dg = rnd(nd, hq * wq, 8, seed=13), rnd(nd, nk, 8, seed=14), rnd(nd, nk, 8, seed=15)
    cot = torch.cat([dph, dg], -1).view(nd, hq // 2, wq // 2, 16).permute(0, 3, 1, 2)
    (gv,) = torch.autograd.grad((pooled * cot).sum(), v)
    got = S.split_pool_bwd_ref(proj, dth, dph, dg, dom, npix)
    inside = torch.zeros(npix, dtype=torch.bool)
    inside[pix.reshape(-1)] = True
    assert bool(torch.isnan(got[~inside]).all()) and not bool(torch.isnan(got[inside]).any())
    assert torch.equal(got[pix.reshape(-1)][:, 8:].view(nd, hq, wq, 16), gv.permute(0, 2, 3, 1))
    assert torch.equal(got[pix.reshape(-1)][:, :8].view(nd, hq * wq, 8), dth)


@pytest.mark.parametrize("dom", DOMAINS)
def test_the_kernel_chain_composes_to_the_oracle_block_per_domain(dom):
    """project -> split / pool -> attention -> output and every backward step, against O.nonlocal_block on each rectangle"""
    B, H, W, y0, x0, hq, wq, nqy, nqx = dom
    npix = B * H * W
    sd = {"b.theta.weight": rnd(8, 64, 1, 1, seed=20, scale=0.3), "b.theta.bias": rnd(8, seed=21),
          "b.phi.0.weight": rnd(8, 64, 1, 1, seed=22, scale=0.3), "b.phi.0.bias": rnd(8, seed=23),
          "b.g.0.weight": rnd(8, 64, 1, 1, seed=24, scale=0.3), "b.g.0.bias": rnd(8, seed=25),
          "b.W.weight": rnd(64, 8, 1, 1, seed=26, scale=0.3), "b.W.bias": rnd(64, seed=27)}
    sd = {k: v.requires_grad_(True) for k, v in sd.items()}
    x = rnd(B, 64, H, W, seed=28).requires_grad_(True)
    cot = rnd(B, 64, H, W, seed=29)
    loss, zs = 0.0, {}
    for b in range(B):
        for iy in range(nqy):
            for ix in range(nqx):
                ys, xs = slice(y0 + iy * hq, y0 + (iy + 1) * hq), slice(x0 + ix * wq, x0 + (ix + 1) * wq)
                z = O.nonlocal_block(sd, "b", x[b:b + 1, :, ys, xs])
                zs[(b, iy, ix)] = z.detach()
                loss = loss + (z * cot[b:b + 1, :, ys, xs]).sum()
    keys = list(sd)
    grads = dict(zip(["x"] + keys, torch.autograd.grad(loss, [x] + [sd[k] for k in keys])))
    rows = lambda t: t.detach().permute(0, 2, 3, 1).reshape(npix, -1)  # noqa: E731
    w = {k: sd[k].detach().reshape(sd[k].shape[0], -1) if k.endswith("weight") else sd[k].detach() for k in keys}
    xr, dz = rows(x), rows(cot)
    pw = (w["b.theta.weight"], w["b.phi.0.weight"], w["b.g.0.weight"])
    proj = S.project_fwd_ref(xr, pw[0], w["b.theta.bias"], pw[1], w["b.phi.0.bias"], pw[2], w["b.g.0.bias"])
    sp = S.split_pool_fwd_ref(proj, dom)
    at = S.attn_fwd_ref(sp["theta"], sp["phi"], sp["g"])
    z = S.output_fwd_ref(at["y"], xr, w["b.W.weight"], w["b.W.bias"], dom)
    pix = S.domain_pixels(dom)
    inside = torch.zeros(npix, dtype=torch.bool)
    inside[pix.reshape(-1)] = True
    assert bool(torch.isnan(z[~inside]).all())
    for (b, iy, ix), zd in zs.items():
        same(z[pix[(b * nqy + iy) * nqx + ix].reshape(-1)], zd[0].permute(1, 2, 0).reshape(-1, 64), "z")
    ob = S.output_bwd_ref(dz, at["y"], w["b.W.weight"], dom)
    ab = S.attn_bwd_ref(sp["theta"], sp["phi"], sp["g"], ob["dy"])
    dproj = S.split_pool_bwd_ref(proj, ab["dtheta"], ab["dphi"], ab["dg"], dom, npix, fill=0.0)
    dzin = torch.where(inside[:, None], dz, torch.zeros_like(dz))
    loose = dict(rtol=1e-9, atol=1e-11)
    same(S.project_dgrad_ref(dproj, dzin, *pw), rows(grads["x"]), "dx", **loose)
    wg = S.project_wgrad_ref(xr, dproj)
    for i, name in enumerate(("theta", "phi.0", "g.0")):
        same(wg["dW"][8 * i:8 * i + 8], grads[f"b.{name}.weight"].reshape(8, 64), name + " dW", **loose)
        same(wg["db"][8 * i:8 * i + 8], grads[f"b.{name}.bias"], name + " db", **loose)
    same(ob["dW"], grads["b.W.weight"].reshape(64, 8), "W dW", **loose)
    same(ob["db"], grads["b.W.bias"], "W db", **loose)
    for A_ref, ref in ((S.output_fwd_ref(at["y"], xr, w["b.W.weight"], w["b.W.bias"], dom, A=True)[inside], z[inside].abs()),
                       (S.output_bwd_ref(dz, at["y"], w["b.W.weight"], dom, A=True)["dW"], ob["dW"].abs())):
        assert bool((A_ref >= ref).all())
