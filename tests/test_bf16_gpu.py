"""bf16 matrix-core mode (ops.set_precision('bf16')) on a real MI355X (pytest -m gpu).

The reference has no reduced-precision mode, so there is no reference vector for it: PARITY UNPINNED against the
reference.  What is pinned: (1) the kernels against the oracle's restatement of the mode (operands of every
64-channel-multiple conv contraction rounded to bf16, exact products, fp32 accumulation -- oracle.CONV_PRECISION =
'bf16'), to fp32 summation-order tolerance; (2) the distance from the fp32 result, reported and bounded loosely.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sisr_amd
from oracle import sisr_oracle as O
from test_hip_gpu import DEV, close, rnd
from test_init_parity import set5

pytestmark = pytest.mark.gpu
A = sisr_amd.architectures
ops = sisr_amd.ops
hip = sisr_amd.hip


@pytest.fixture(autouse=True)
def bf16_mode():
    ops.set_precision("bf16")
    O.CONV_PRECISION = "bf16"
    yield
    ops.set_precision("fp32")
    O.CONV_PRECISION = "fp32"


def r16(t):
    return t.to(torch.bfloat16).to(torch.float32)


@pytest.mark.parametrize("B,H,W", [(2, 16, 16), (1, 13, 9), (1, 57, 86), (2, 4, 32), (1, 128, 128)])
def test_conv64_bf16_fwd_bwd(B, H, W):
    m = A.default_conv(64, 64, 3)
    x = rnd(B, 64, H, W, seed=1)
    cot = rnd(B, 64, H, W, seed=2)
    sd = {"c." + k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    ref = O.conv(sd, "c", xo)
    ref.backward(cot)
    m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = ops.conv3x3(xd, m.weight, m.bias)
    close(out, ref, 2e-5, 2e-6, "bf16 conv out")
    out.backward(cot.to(DEV))
    close(xd.grad, xo.grad, 2e-5, 2e-6, "bf16 conv dx")
    close(m.weight.grad, sd["c.weight"].grad, 1e-4, 1e-5, "bf16 conv dw")
    close(m.bias.grad, sd["c.bias"].grad, 1e-4, 1e-5, "bf16 conv db")
    # and it really is the bf16 contraction, not fp32: the fp32 result differs at the 1e-3 level
    with torch.no_grad():
        exact = F.conv2d(x, m.weight.cpu(), m.bias.cpu(), padding=1)
    assert float((out.detach().cpu() - exact).abs().max()) > 1e-4


def test_multichunk_and_shuffle_bf16():
    """128 -> 64 (two input chunks) and 64 -> 256 + PixelShuffle(2) through the bf16 kernels."""
    for cin, cout, shuffle in ((128, 64, 1), (64, 256, 2)):
        m = A.default_conv(cin, cout, 3)
        x = rnd(2, cin, 9, 37, seed=3)
        sd = {"c." + k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
        xo = x.clone().requires_grad_(True)
        ref = O.conv(sd, "c", xo)
        if shuffle > 1:
            ref = F.pixel_shuffle(ref, shuffle)
        cot = rnd(*ref.shape, seed=4)
        ref.backward(cot)
        m.to(DEV)
        xd = x.to(DEV).requires_grad_(True)
        out = ops.conv3x3(xd, m.weight, m.bias, shuffle=shuffle)
        close(out, ref, 2e-5, 2e-6, f"{cin}->{cout} out")
        out.backward(cot.to(DEV))
        close(xd.grad, xo.grad, 3e-5, 3e-6, f"{cin}->{cout} dx")
        close(m.weight.grad, sd["c.weight"].grad, 1e-4, 1e-5, f"{cin}->{cout} dw")
        close(m.bias.grad, sd["c.bias"].grad, 1e-4, 1e-5, f"{cin}->{cout} db")


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def test_conv_options_bf16():
    """Every prologue / epilogue option of the bf16 conv kernel against the rounding restatement."""
    B, H, W = 2, 11, 37
    x, w, b = rnd(B, 64, H, W, seed=5), rnd(64, 64, 3, 3, seed=6, scale=0.05), rnd(64, seed=7)
    res, mask = rnd(B, 64, H, W, seed=8), rnd(B, 64, H, W, seed=9)
    sc, sh, osc = rnd(B, 64, seed=10).abs() + 0.5, rnd(B, 64, seed=11), rnd(B, 64, seed=12)
    cl = torch.channels_last
    d = lambda t: t.to(DEV).contiguous(memory_format=cl) if t.dim() == 4 else t.to(DEV).contiguous()  # noqa: E731
    xd, bd, resd, maskd, scd, shd, oscd = map(d, (x, b, res, mask, sc, sh, osc))
    wd = w.to(DEV).contiguous()  # OIHW
    v = hip.view_plain(H, W, 64)
    pk = ops.pack_weight(wd, "fwd")
    assert pk.dtype == torch.bfloat16

    def run(**kw):
        y = torch.empty(B, 64, H, W, device=DEV).contiguous(memory_format=cl)
        ops.conv_c64(xd, v, pk, kw.pop("bias", None), (1, 64), y, v, B, H, W, 64, 64, **kw)
        return y

    base = lambda xin: F.conv2d(r16(xin), r16(w), None, padding=1)  # noqa: E731
    gap = torch.empty(B, ops.gap_parts(H, W), 64, device=DEV)
    y = run(bias=bd, relu=True, gap=gap)
    want = F.relu(base(x) + b.view(1, 64, 1, 1))
    close(y, want, 2e-5, 2e-6, "relu + bias")
    close(gap.sum(dim=1), want.sum(dim=(2, 3)), 1e-4, 1e-5, "gap partials")
    close(run(res=resd, alpha=0.3), 0.3 * base(x) + res, 2e-5, 2e-6, "residual + alpha")
    close(run(mask=maskd), base(x) * (mask > 0), 2e-5, 2e-6, "mask")
    xa = x * sc.view(B, 64, 1, 1) + sh.view(B, 64, 1, 1)
    close(run(mask=maskd, in_scale=scd, in_shift=shd), base(xa) * (mask > 0), 2e-5, 2e-6, "affine + mask")
    close(run(in_scale=scd, res=resd), base(x * sc.view(B, 64, 1, 1)) + res, 2e-5, 2e-6, "scale + residual")
    close(run(out_scale=oscd), base(x) * osc.view(B, 64, 1, 1), 2e-5, 2e-6, "out scale")


@pytest.mark.parametrize("B,H,W", [(8, 128, 128), (5, 126, 150), (33, 64, 64)])
def test_persistent_conv_is_bit_identical_to_per_tile_conv(B, H, W):
    """Grids of >= 1024 tiles run the persistent double-buffered bf16 kernel; it must reproduce the one-workgroup-
    per-tile kernel bit for bit (same fragment order), for every prologue / epilogue it serves."""
    cl = torch.channels_last
    dev4 = lambda t: t.to(DEV).contiguous(memory_format=cl)  # noqa: E731
    x, res, mask, skip, dot = (dev4(rnd(B, 64, H, W, seed=80 + i)) for i in range(5))
    w, b = rnd(64, 64, 3, 3, seed=86, scale=0.05).to(DEV), rnd(64, seed=87).to(DEV)
    sc, sh = (rnd(B, 64, seed=88).abs() + 0.5).to(DEV), rnd(B, 64, seed=89).to(DEV)
    v = hip.view_plain(H, W, 64)
    pk = ops.pack_weight(w, "fwd")
    cases = [dict(bias=b, relu=True, gap=True), dict(res=res, alpha=0.3), dict(mask=mask), dict(mask=mask, res=res),
             dict(mask=mask, in_scale=sc, in_shift=sh), dict(in_scale=sc, res=res), dict(in_scale=sc),
             dict(mask=mask, in_scale=sc, in_shift=sh, res=res),
             dict(bias=b, relu=True, in_scale=sc, gate_add=skip, gate_out=True),
             dict(in_scale=sc, gate_add=skip, gate_out=True, res=res), dict(gap=True, dot=dot),
             dict(gap=True, dot=dot, res=res)]
    outs = {}
    for persist in (1, 0):  # per-call kernel selection: select = 0 persistent tile loop, 1 per-tile kernel
        for i, kw in enumerate(cases):
            kw = dict(kw)
            y = torch.full((B, 64, H, W), float("nan"), device=DEV).contiguous(memory_format=cl)
            gap = torch.full((B, ops.gap_parts(H, W), 64), float("nan"), device=DEV) if kw.pop("gap", False) else None
            go = torch.full((B, 64, H, W), float("nan"), device=DEV).contiguous(memory_format=cl) \
                if kw.pop("gate_out", False) else None
            ops.conv_c64(x, v, pk, kw.pop("bias", None), (1, 64), y, v, B, H, W, 64, 64, gap=gap, gate_out=go,
                         select=0 if persist else 1, **kw)
            outs[(persist, i)] = (y, gap, go)
    for i in range(len(cases)):
        for a, bb, what in zip(outs[(1, i)], outs[(0, i)], ("output", "gap / dot partials", "gate_out")):
            if a is not None:
                assert not torch.isnan(a).any(), f"case {i}: {what} has unwritten elements"
                assert torch.equal(a, bb), f"case {i}: {what} differs between the two kernels"


@pytest.mark.parametrize("B,H,W", [(1, 13, 9), (2, 16, 40), (1, 57, 86), (1, 128, 128)])
def test_conv_gate_and_dot_hooks_bf16(B, H, W):
    """GATE prologue (input = t*g + skip built in fp32, written out, then rounded) and DOT epilogue of the bf16 conv."""
    cl = torch.channels_last
    dev4 = lambda t: t.to(DEV).contiguous(memory_format=cl)  # noqa: E731
    t, skip, res, dot = (rnd(B, 64, H, W, seed=60 + i) for i in range(4))
    g = rnd(B, 64, seed=64).abs() + 0.25
    w, b = rnd(64, 64, 3, 3, seed=65, scale=0.05), rnd(64, seed=66)
    td, skd, resd, dotd, gd, wd, bd = dev4(t), dev4(skip), dev4(res), dev4(dot), g.to(DEV), w.to(DEV), b.to(DEV)
    v = hip.view_plain(H, W, 64)
    pk = ops.pack_weight(wd, "fwd")
    u = t * g.view(B, 64, 1, 1) + skip
    conv16 = lambda xin, bias: F.conv2d(r16(xin), r16(w), bias, padding=1)  # noqa: E731
    for kw, want in ((dict(relu=True), F.relu(conv16(u, b))), (dict(res=resd), conv16(u, b) + res)):
        y = torch.full((B, 64, H, W), float("nan"), device=DEV).contiguous(memory_format=cl)
        uo = torch.full((B, 64, H, W), float("nan"), device=DEV).contiguous(memory_format=cl)
        ops.conv_c64(td, v, pk, bd, (1, 64), y, v, B, H, W, 64, 64, in_scale=gd, gate_add=skd, gate_out=uo, **kw)
        close(uo, u, 1e-6, 1e-6, "gate_out")
        # u itself may differ by an fp32 ulp (fused multiply-add), which can flip a bf16 rounding: compare via rms
        assert rms(y.cpu() - want) < 2e-4 * rms(want), kw
    for kw, want in ((dict(), conv16(t, None)), (dict(res=resd), conv16(t, None) + res)):
        y = torch.empty(B, 64, H, W, device=DEV).contiguous(memory_format=cl)
        gap = torch.full((B, ops.gap_parts(H, W), 64), float("nan"), device=DEV)
        ops.conv_c64(td, v, pk, None, (1, 64), y, v, B, H, W, 64, 64, gap=gap, dot=dotd, **kw)
        close(y, want, 2e-5, 2e-6, "dot conv output")
        close(gap.sum(dim=1), (want * dot).sum(dim=(2, 3)), 2e-4, 2e-5, "dot partials")


@pytest.mark.parametrize("kind", ["rcab", "resblock", "paramresblock"])
def test_fused_block_bf16_vs_oracle_restatement(kind):
    """Two chained convs per direction: still comparable element-wise (one rounding layer of amplification)."""
    torch.manual_seed(8)
    relu = torch.nn.ReLU(True)
    x, md = rnd(2, 64, 12, 40, seed=13), rnd(2, 10, 1, 1, seed=14, scale=0.3)
    if kind == "rcab":
        m = A.RCAB(A.default_conv, 64, 3, 16, act=relu)
        fn = lambda sd, xx: O.rcab(sd, "b", xx)  # noqa: E731
    elif kind == "resblock":
        m = A.ResBlock(A.default_conv, 64, 3, act=relu, res_scale=0.1)
        fn = lambda sd, xx: O.res_block(sd, "b", xx, 0.1)  # noqa: E731
    else:
        m = A.ParamResBlock(A.default_conv, 64, 10, 3, act=relu, res_scale=0.1)
        fn = lambda sd, xx: O.param_res_block(sd, "b", xx, md, 0.1, False)  # noqa: E731
    sd = {"b." + k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    ref = fn(sd, xo)
    cot = rnd(*ref.shape, seed=15)
    ref.backward(cot)
    m.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out = m((xd, md.to(DEV)))[0] if kind == "paramresblock" else m(xd)
    out.backward(cot.to(DEV))

    def near(got, want, what):
        e, n = rms(got.detach().cpu() - want.detach()), rms(want.detach())
        assert e < 2e-4 * n + 1e-7, (kind, what, e, n)

    near(out, ref, "out")
    near(xd.grad, xo.grad, "dx")
    for k, p in m.named_parameters():
        near(p.grad, sd["b." + k].grad, k)


def _net_vs_oracle(net, name, cfg, x, md=None):
    """Deep nets cannot be compared tightly in this mode.  An activation that differs by one fp32 ulp between the
    GPU's and the CPU's summation order can round to the neighbouring bf16 value at the next conv's input (a 2^-8
    relative step); a perturbation d << ulp therefore leaves a rounding layer with rms sqrt(d * ulp) >> d, and after
    four or five convs two fp32-noise-apart evaluations have decorrelated to the bf16 noise floor itself.  What a
    whole net can show is that the HIP result is no further from the bf16 restatement than the restatement is from
    fp32 (same noise floor, no systematic error); exactness is established per kernel and per block above."""
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    ref = O.forward(name, sd, x.clone(), md, **cfg)
    cot = rnd(*ref.shape, seed=31)
    ref.backward(cot)
    O.CONV_PRECISION = "fp32"
    sd32 = {k: v.detach().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    ref32 = O.forward(name, sd32, x.clone(), md, **cfg)
    ref32.backward(cot)
    O.CONV_PRECISION = "bf16"
    net.to(DEV)
    out = net(x.to(DEV), md.to(DEV)) if md is not None else net(x.to(DEV))
    out.backward(cot.to(DEV))
    o = out.detach().cpu()
    gap, err = rms(ref.detach() - ref32.detach()), rms(o - ref.detach())
    print(f"{name}: rms(bf16 oracle - fp32 oracle) = {gap:.3e}, rms(HIP bf16 - bf16 oracle) = {err:.3e}")
    assert gap > 0 and err < 1.5 * gap, (gap, err)
    worst, tot_g, tot_e = 0.0, 0.0, 0.0
    for k, p in net.named_parameters():
        g16, g32 = sd[k].grad, sd32[k].grad
        gg, ee = rms(g16 - g32), rms(p.grad.cpu() - g16)
        tot_g += gg * gg * g16.numel()
        tot_e += ee * ee * g16.numel()
        if g16.numel() >= 64:  # single scalars (gammas, biases of 3) are one random draw each: judged in aggregate
            assert ee <= 2.5 * gg + 1e-5 * (1 + rms(g16)), (k, gg, ee)
            worst = max(worst, ee / (gg + 1e-30))
    print(f"{name}: grads: total err / total gap = {(tot_e / tot_g) ** 0.5:.3f}, worst tensor {worst:.3f}")
    assert tot_e < 2.25 * tot_g
    return o


def test_rcan_reduced_bf16_vs_oracle_restatement():
    torch.manual_seed(8)
    net = A.RCAN(n_resblocks=2, n_resgroups=2, n_feats=64, scale=4)
    _net_vs_oracle(net, "rcan", dict(n_resgroups=2, n_resblocks=2, scale=4), rnd(2, 3, 20, 36, seed=30, scale=0.5))


def test_qrcan_and_han_reduced_bf16_vs_oracle_restatement():
    torch.manual_seed(8)
    net = A.QRCAN(n_resblocks=2, n_resgroups=2, n_feats=64, scale=4, style="standard", num_metadata=10,
                  include_q_layer=True)
    _net_vs_oracle(net, "qrcan", dict(n_resgroups=2, n_resblocks=2, scale=4, style="standard", include_q_layer=True),
                   rnd(2, 3, 12, 34, seed=33, scale=0.5), rnd(2, 10, 1, 1, seed=34, scale=0.3))
    torch.manual_seed(8)
    net = sisr_amd.han.HAN(n_resgroups=10, n_resblocks=1, n_feats=64, scale=4)
    with torch.no_grad():
        net.la.gamma.fill_(0.37)
        net.csa.gamma.fill_(0.37)
    _net_vs_oracle(net, "han", dict(n_resgroups=10, n_resblocks=1, scale=4), rnd(1, 3, 16, 20, seed=35, scale=0.5))


def test_han_full_depth_bf16_set5_psnr_close_to_fp32():
    """BASELINE config 'HAN x4 bf16': full-depth HAN on Set5 in bf16 mode vs the fp32 HIP path (same weights)."""
    torch.manual_seed(8)
    h = sisr_amd.handlers.available_models["han"](device=0, model_save_dir="/tmp", eval_mode=True, scale=4)
    rows = []
    for im, x, y, md in set5():
        ops.set_precision("bf16")
        o16, _, _ = h.run_eval(x, y, request_loss=False)
        ops.set_precision("fp32")
        o32, _, _ = h.run_eval(x, y, request_loss=False)
        p16 = sisr_amd.metrics.y_psnr(o16[0].numpy(), y[0].numpy())
        p32 = sisr_amd.metrics.y_psnr(o32[0].numpy(), y[0].numpy())
        rows.append((im, p16, p32, float((o16 - o32).abs().max())))
    print("HAN bf16 vs fp32 Set5 (image, psnr16, psnr32, max abs diff):", rows)
    for im, p16, p32, d in rows:
        assert abs(p16 - p32) < 0.05, rows
        assert d > 0, "bf16 mode produced the fp32 result bit for bit: the switch did nothing"


def test_training_step_bf16_runs_and_tracks_fp32():
    """Ten RCAN training steps in each mode from the same init / data: losses stay within 2 % of each other."""
    losses = {}
    for mode in ("fp32", "bf16"):
        ops.set_precision(mode)
        torch.manual_seed(8)
        h = sisr_amd.handlers.available_models["rcan"](device=0, model_save_dir="/tmp", eval_mode=False, scale=4, lr=1e-4)
        g = torch.Generator().manual_seed(9)
        ls = []
        for _ in range(10):
            x, y = torch.rand(4, 3, 32, 32, generator=g), torch.rand(4, 3, 128, 128, generator=g)
            loss, _ = h.run_train(x, y)
            ls.append(float(loss))
        losses[mode] = ls
    print("loss trajectories:", losses)
    for a, b in zip(losses["fp32"], losses["bf16"]):
        assert np.isfinite(b) and abs(a - b) < 0.02 * abs(a) + 1e-3, losses
