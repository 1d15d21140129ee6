"""Winograd F(2x2,3x3) form of the fp32 64-channel weight gradient (wgrad3x3_c64_w4_kernel): exact dyadic data against
float64 bit for bit, random data against float64 beside the direct form, determinism, the selection rule and the switches,
and whole-net checks (full-depth RCAN losses, reduced RCAN / QRCAN against the float64 oracle)."""
import contextlib
import os

import pytest
import torch
import torch.nn.functional as F

import _exact as X
import sisr_amd

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
hip = sisr_amd.hip
DEV = "cuda:0"
CL = torch.channels_last
NAN = float("nan")
THRESHOLD = 8 * 128 * 128  # pixels per launch above which the Winograd form is selected


@contextlib.contextmanager
def env(**kv):
    prev = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        yield
    finally:
        for k, v in prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


WINO = dict(SISR_WGRAD_WINOGRAD=None, SISR_CONV_WINOGRAD=None)
DIRECT = dict(SISR_WGRAD_WINOGRAD="0", SISR_CONV_WINOGRAD=None)


def dev4(t):
    return t.to(DEV, torch.float32).contiguous(memory_format=CL)


def dd(t):
    return t.to(DEV, torch.float64)


def run(x, dy, B, H, W, cin=64, cout=64, bias=True, switches=WINO, **kw):
    dw = torch.full((cout, cin, 3, 3), NAN, device=DEV)
    db = torch.full((cout,), NAN, device=DEV) if bias else None
    with env(**switches):
        ops.wgrad_c64(x, hip.view_plain(H, W, cin), dy, hip.view_plain(H, W, cout), dw, db, B, H, W, cin, cout, **kw)
    torch.cuda.synchronize()
    return dw, db


# the kernel's transforms (tests/test_winograd_wgrad_cpu.py pins them against the direct weight gradient)
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
AS = torch.tensor([[1, 0], [1, 1], [1, -1], [0, 1]], dtype=torch.float64)
GS = torch.tensor([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, -1]], dtype=torch.float64)


def winograd_wgrad_budget(x, dyp):
    """the Winograd contraction on absolute values: sum_blocks |M| |V| per transform point, then the fold with |G|, in
    units of the fold's granule (granule(x) granule(dY') / 4); it bounds every partial sum the kernel forms"""
    B, C, H, W = x.shape
    Hb, Wb = (H + 1) // 2, (W + 1) // 2
    bt, a_s, gs = (m.to(x.device).abs() for m in (BT, AS, GS))
    dU = 0
    for b0 in range(0, B, 4):
        xs, ys = x[b0:b0 + 4].abs(), dyp[b0:b0 + 4].abs()
        d = F.pad(xs, (1, 2 * Wb + 1 - W, 1, 2 * Hb + 1 - H)).unfold(2, 4, 2).unfold(3, 4, 2)
        y = F.pad(ys, (0, 2 * Wb - W, 0, 2 * Hb - H)).unfold(2, 2, 2).unfold(3, 2, 2)
        V = torch.einsum("rk,bchwkl,sl->rsbhwc", bt, d, bt).reshape(16, -1, C)
        M = torch.einsum("ri,bohwij,sj->rsbhwo", a_s, y, a_s).reshape(16, -1, y.shape[1])
        dU = dU + torch.bmm(M.transpose(1, 2), V)
    mag = torch.einsum("ra,rsoc,sb->ocab", gs, dU.view(4, 4, *dU.shape[1:]), gs)
    return X.assert_budget(mag, X.granule(x) * X.granule(dyp) / 4, "Winograd weight gradient")


def exact_ref(x, dy, sc=None, sh=None, alpha=1.0):
    dyp = dd(dy)
    if sc is not None:
        dyp = dyp * dd(sc).view(*sc.shape, 1, 1) + dd(sh).view(*sh.shape, 1, 1)
    X.wgrad_budget(dd(x), dyp)
    winograd_wgrad_budget(dd(x), dyp)
    return alpha * X.wgrad_ref(dd(x), dyp), alpha * dyp.sum(dim=(0, 2, 3))


@pytest.mark.parametrize("B,H,W,cout", [(9, 128, 128, 64), (32, 128, 128, 64), (40, 37, 129, 64), (9, 131, 127, 64),
                                        (9, 128, 128, 256)])
def test_exact_against_float64(B, H, W, cout):
    """x in {-1, 0, 1} (3/4 zeros), dY in {-1, 0, 1}: plain with the bias gradient, then (but at B = 32, over the exact-data
    budget) dy_scale + dy_shift (halves) + alpha, bit-equal to float64; ragged / odd sizes above the threshold and a
    multi-pair grid (cout = 256)"""
    assert B * H * W > THRESHOLD
    x = X.ints((B, 64, H, W), 600 + B, lo=-1, hi=1, zeros=0.75)
    dy = X.ints((B, cout, H, W), 601 + W, lo=-1, hi=1)
    xd, dyd = dev4(x), dev4(dy)
    dw, db = run(xd, dyd, B, H, W, cout=cout)
    dw_ref, db_ref = exact_ref(x, dy)
    X.assert_exact(dw, dw_ref, "plain dw")
    X.assert_exact(db, db_ref, "plain db")
    if B == 32:
        return
    sc, sh = X.scales((B, cout), 602), X.ints((B, cout), 603) / 2
    dw, db = run(xd, dyd, B, H, W, cout=cout, alpha=X.ALPHA, dy_scale=sc.to(DEV), dy_shift=sh.to(DEV))
    dw_ref, db_ref = exact_ref(x, dy, sc, sh, X.ALPHA)
    X.assert_exact(dw, dw_ref, "affine dw")
    X.assert_exact(db, db_ref, "affine db")


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("B,H,W", [(9, 128, 128), (32, 128, 128), (40, 37, 129)])
def test_random_against_float64_and_the_direct_form(B, H, W):
    """random data: within the direct kernel's tolerance of float64 and at most 3x the direct form's max error; two runs
    give the same bits; the bias gradient within the same tolerance"""
    x, dy = rnd(B, 64, H, W, seed=610), rnd(B, 64, H, W, seed=611)
    sc, sh = rnd(B, 64, seed=612).abs() + 0.5, rnd(B, 64, seed=613)
    xd, dyd = dev4(x), dev4(dy)
    kw = dict(dy_scale=sc.to(DEV), dy_shift=sh.to(DEV), alpha=0.7)
    dyp = dd(dy) * dd(sc).view(B, 64, 1, 1) + dd(sh).view(B, 64, 1, 1)
    want, want_b = 0.7 * X.wgrad_ref(dd(x), dyp), 0.7 * dyp.sum(dim=(0, 2, 3))
    dw_w, db_w = run(xd, dyd, B, H, W, **kw)
    dw_w2, db_w2 = run(xd, dyd, B, H, W, **kw)
    dw_d, db_d = run(xd, dyd, B, H, W, switches=DIRECT, **kw)
    assert torch.equal(dw_w, dw_w2) and torch.equal(db_w, db_w2), "two runs differ"
    assert not torch.equal(dw_w, dw_d), "the Winograd form did not engage"
    scale = float(want.abs().max())
    err_w = float((dw_w.double() - want).abs().max()) / scale
    err_d = float((dw_d.double() - want).abs().max()) / scale
    print(f"max |err| / max |dw|: winograd {err_w:.3e}, direct {err_d:.3e}")
    assert err_d < 1e-5 and err_w < 1e-5
    assert err_w <= 3 * err_d
    # the bias sums run over 4-row instead of 8-row tiles: another summation order, the same accuracy
    err_b = float((db_w.double() - want_b).abs().max()) / float(want_b.abs().max())
    assert err_b < 1e-5


@pytest.mark.parametrize("B,switches", [(8, WINO), (9, dict(SISR_WGRAD_WINOGRAD="0", SISR_CONV_WINOGRAD=None)),
                                        (9, dict(SISR_WGRAD_WINOGRAD=None, SISR_CONV_WINOGRAD="0"))])
def test_selection_rule_and_switches(B, switches):
    """at <= 8 x 128^2 pixels, and with either switch at 0 above it, the result is the direct dense kernel's, bit for bit"""
    H = W = 128
    x, dy = dev4(rnd(B, 64, H, W, seed=620)), dev4(rnd(B, 64, H, W, seed=621))
    dw, db = run(x, dy, B, H, W, switches=switches)
    with env(SISR_CONV_WINOGRAD="0"):
        dw_d, db_d = run(x, dy, B, H, W, switches=dict(SISR_WGRAD_WINOGRAD="0"))
    assert torch.equal(dw, dw_d) and torch.equal(db, db_d)
    if B * H * W > THRESHOLD:
        dw_w, _ = run(x, dy, B, H, W)
        assert not torch.equal(dw_w, dw_d), "the Winograd form did not engage"


def test_full_depth_training_loss_matches_the_direct_weight_gradient():
    """RCAN x4 at full depth, 16 tiles of 128 x 128, three training steps: the losses with the Winograd weight gradient
    match SISR_WGRAD_WINOGRAD=0 to 1e-5 relative"""
    g = torch.Generator().manual_seed(8)
    x = torch.rand(16, 3, 128, 128, generator=g).to(DEV)
    y = torch.rand(16, 3, 512, 512, generator=g).to(DEV)
    losses = {}
    for wino in ("1", "0"):
        with env(SISR_WGRAD_WINOGRAD=wino):
            torch.manual_seed(8)
            h = sisr_amd.available_models["rcan"](device=DEV, model_save_dir="/tmp", eval_mode=False, scale=4, lr=1e-4)
            losses[wino] = [float(h.train_step(x, y)[0]) for _ in range(3)]
            del h
    assert losses["1"] != losses["0"], "the Winograd weight gradient did not engage"
    for a, b in zip(losses["1"], losses["0"]):
        assert abs(a - b) <= 1e-5 * abs(b), (losses["1"], losses["0"])


def _net_grads(net, x, md, cot, wgrad_wino):
    net.zero_grad(set_to_none=True)
    with env(SISR_WGRAD_WINOGRAD=None if wgrad_wino else "0"):
        out = net(x, md) if md is not None else net(x)
        out.backward(cot)
        torch.cuda.synchronize()
    return {k: p.grad.detach().double().cpu() for k, p in net.named_parameters()}


@pytest.mark.parametrize("meta", [False, True])
def test_reduced_depth_net_against_the_float64_oracle(meta):
    """RCAN / QRCAN, 2 groups x 3 blocks, 18 x 128 x 64 LR maps (above the threshold): the parameter gradients' root-sum-square
    distance to the float64 oracle with the Winograd weight gradient is at most 2x that of the direct weight gradient and of
    the reference's fp32 arithmetic (the aggregate, as test_winograd_gpu.py argues)"""
    from oracle import sisr_oracle as O
    A = sisr_amd.architectures
    torch.manual_seed(8)
    kw = dict(n_resblocks=3, n_resgroups=2, n_feats=64, scale=2)
    net = A.QRCAN(style="standard", num_metadata=10, include_q_layer=True, **kw) if meta else A.RCAN(**kw)
    B, H, W = 18, 128, 64
    x = rnd(B, 3, H, W, seed=90) * 0.5
    md = rnd(B, 10, 1, 1, seed=91) * 0.3 if meta else None

    def oracle(dt):
        sd = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in net.state_dict().items()}
        if meta:
            r = O.qrcan(sd, x.to(dt), md.to(dt), n_resgroups=2, n_resblocks=3, scale=2, style="standard", include_q_layer=True)
        else:
            r = O.rcan(sd, x.to(dt), n_resgroups=2, n_resblocks=3, scale=2)
        r.backward(rnd(*r.shape, seed=92).to(dt))
        return {k: v.grad.double() for k, v in sd.items()}

    g_ref, g_32 = oracle(torch.float64), oracle(torch.float32)
    cot = rnd(B, 3, 2 * H, 2 * W, seed=92)
    net.to(DEV)
    xd, mdd = x.to(DEV), (md.to(DEV) if meta else None)
    g_w = _net_grads(net, xd, mdd, cot.to(DEV), True)
    g_d = _net_grads(net, xd, mdd, cot.to(DEV), False)
    tot = {"w": 0.0, "d": 0.0, "r": 0.0}
    for k in g_w:
        want = g_ref[k]
        for n, g in (("w", g_w[k]), ("d", g_d[k]), ("r", g_32[k])):
            tot[n] += float((g - want).norm()) ** 2
    tot = {n: v ** 0.5 for n, v in tot.items()}
    print(f"gradients, root-sum-square |err| vs f64: winograd wgrad {tot['w']:.3e}, direct {tot['d']:.3e}, "
          f"reference fp32 {tot['r']:.3e}")
    assert any(not torch.equal(g_w[k], g_d[k]) for k in g_w), "the Winograd weight gradient did not engage"
    assert tot["w"] <= 2 * tot["d"] and tot["w"] <= 2 * tot["r"]
