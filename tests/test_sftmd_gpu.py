"""SFTMD on the HIP kernels vs the reference's own vectors (pytest -m gpu; fixtures: tools/make_fixtures_sftmd.py) and, for
the new kernels one by one, vs the oracle's formulation of the same op."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sisr_amd
from sisr_amd import hip, ops
from conftest import golden_json, load_golden
from test_init_parity import set5
from test_oracle_sftmd import PARAMS, VARIANTS, reduced_net, variant_inputs, variant_net

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(ops.PRECISION != "fp32", reason="SFTMD runs on the fp32 kernels only (SISR_PRECISION is set)")]


def build(eval_mode=True, **extra):
    torch.manual_seed(8)
    return sisr_amd.available_models["sftmd"](device=0, model_save_dir="/tmp", eval_mode=eval_mode, scale=4, **PARAMS, **extra)


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("shape", [(1, 7, 9), (2, 16, 33), (1, 40, 70), (1, 3, 100), (2, 264, 530)])
def test_conv9_forward_and_gradients(shape):
    """9x9 64 -> 3 conv + clamp (ref: SFTMD.conv_output, :159): ragged sizes smaller and larger than the 9-tap window and
    the kernels' tiles (24 / 32 / 64 columns, 8 rows); the last one has more tiles than the persistent grids have workgroups."""
    B, H, W = shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 64, H, W, generator=g)
    w = (torch.randn(3, 64, 9, 9, generator=g) * 0.02).requires_grad_(True)
    b = (torch.randn(3, generator=g) * 0.1 + 0.4).requires_grad_(True)
    cot = torch.randn(B, 3, H, W, generator=g)
    xr = x.clone().requires_grad_(True)
    want = torch.clamp(F.conv2d(F.leaky_relu(xr, 0.2), w, b, padding=4), 0, 1)
    want.backward(cot)
    xa = F.leaky_relu(x, 0.2).cuda().contiguous(memory_format=torch.channels_last)
    L, dev = hip.lib(), xa.device
    wc, bc = w.detach().cuda(), b.detach().cuda()
    pre = torch.empty(B, 3, H, W, device=dev)
    hip.check(L.sisr_conv9_fwd(hip.ptr(xa), hip.ptr(wc), hip.ptr(bc), hip.ptr(pre), B, H, W, hip.stream()), "conv9")
    out = torch.empty_like(pre)
    hip.check(L.sisr_clamp01(hip.ptr(pre), None, hip.ptr(out), pre.numel(), 0, hip.stream()), "clamp")
    np.testing.assert_allclose(out.cpu().numpy(), want.detach().numpy(), rtol=1e-5, atol=1e-5)  # 5184-term fp32 sums, |pre| ~ 1
    dpre = torch.empty_like(pre)
    hip.check(L.sisr_clamp01(hip.ptr(pre), hip.ptr(cot.cuda()), hip.ptr(dpre), pre.numel(), 1, hip.stream()), "clamp bwd")
    dx = torch.empty(B, 64, H, W, device=dev).contiguous(memory_format=torch.channels_last)
    hip.check(L.sisr_conv9_dgrad(hip.ptr(dpre), hip.ptr(wc), hip.ptr(xa), hip.ptr(dx), B, H, W, hip.stream()), "conv9 dgrad")
    assert rel(dx, xr.grad) < 3e-6
    dw, db = torch.empty_like(wc), torch.empty(3, device=dev)
    nbytes = L.sisr_conv9_wgrad_workspace_bytes(B, H, W)
    ws = hip.workspace(dev, nbytes)
    hip.check(L.sisr_conv9_wgrad(hip.ptr(xa), hip.ptr(dpre), hip.ptr(dw), hip.ptr(db), hip.ptr(ws), nbytes, B, H, W,
                                 hip.stream()), "conv9 wgrad")
    assert rel(dw, w.grad) < 1e-5 and rel(db, b.grad) < 1e-5


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M", [1, 10, 64])
def test_sft_layer_matches_the_four_conv_formulation(relu, M):
    """Merged / block-diagonal MFMA convs + combine kernel vs StandardSft as the reference writes it (:46-56)."""
    g = torch.Generator().manual_seed(5 + M)
    B, H, W = 2, 10, 37
    mod = sisr_amd.sftmd.StandardSft(nf=64, para=M)
    x = torch.randn(B, 64, H, W, generator=g)
    md = torch.rand(B, M, H, W, generator=g)
    cot = torch.randn(B, 64, H, W, generator=g)
    xr = x.clone().requires_grad_(True)
    cat = torch.cat((xr, md), 1)
    mul = torch.sigmoid(mod.mul_conv2(F.leaky_relu(mod.mul_conv1(cat), 0.2)))
    add = mod.add_conv2(F.leaky_relu(mod.add_conv1(cat), 0.2))
    want = xr * mul + add
    want = F.relu(want) if relu else want
    want.backward(cot)
    ref_g = {k: p.grad.clone() for k, p in mod.named_parameters()}
    mod.zero_grad()
    mod.cuda()
    xg = x.cuda().requires_grad_(True)
    out = ops.sft_layer(xg, ops.nchw_to_nhwc_pad(md.cuda(), 64), mod, relu)
    assert rel(out, want) < 2e-6
    out.backward(cot.cuda())
    assert rel(xg.grad, xr.grad) < 5e-6
    for k, p in mod.named_parameters():
        assert rel(p.grad, ref_g[k]) < 5e-6, k


@pytest.mark.parametrize("shape", [(2, 10, 37), (4, 64, 64), (1, 7, 33)])
def test_sparse_select_codes_equal_the_dense_kernel(shape):
    """`select` 8 / 9 skip structural zeros of the merged SFT weights: the remaining products are accumulated in the dense
    kernel's order, so the outputs are bit-identical; the masked weight gradient (other K-slice split) agrees to rounding.
    Small and large grids."""
    B, H, W = shape
    g = torch.Generator().manual_seed(11)
    cl = torch.channels_last
    # 64 -> 128 block-diagonal
    wb = torch.zeros(128, 64, 3, 3)
    wb[:64, :32] = torch.randn(64, 32, 3, 3, generator=g) * 0.1
    wb[64:, 32:] = torch.randn(64, 32, 3, 3, generator=g) * 0.1
    wb, bias = wb.cuda(), (torch.randn(128, generator=g) * 0.1).cuda()
    t = torch.randn(B, 64, H, W, generator=g).cuda().contiguous(memory_format=cl)
    pf, _ = ops.pack_pair(wb)
    outs = []
    for sel in (0, ops.SPARSE_BLOCK_DIAGONAL):
        y = torch.empty(B, 128, H, W, device="cuda").contiguous(memory_format=cl)
        ops.conv_c64(t, hip.view_plain(H, W, 64), pf, bias, (1, 64), y, hip.view_plain(H, W, 128), B, H, W, 64, 128, select=sel)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    # 128 -> 64, input channels >= 80 zero, LeakyReLU epilogue
    wa = torch.zeros(64, 128, 3, 3)
    wa[:, :80] = torch.randn(64, 80, 3, 3, generator=g) * 0.1
    wa = wa.cuda()
    cat = torch.randn(B, 128, H, W, generator=g).cuda().contiguous(memory_format=cl)
    pa, _ = ops.pack_pair(wa)
    outs = []
    for sel in (0, ops.SPARSE_SECOND_CHUNK):
        y = torch.empty(B, 64, H, W, device="cuda").contiguous(memory_format=cl)
        ops.conv_c64(cat, hip.view_plain(H, W, 128), pa, None, (1, 64), y, hip.view_plain(H, W, 64), B, H, W, 128, 64,
                     relu=ops.LEAKY, select=sel)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    # 128 -> 64, the transpose of the block-diagonal form (B's input gradient): LeakyReLU' mask epilogue
    _, pdb = ops.pack_pair(wb)
    dy2g = torch.randn(B, 128, H, W, generator=g).cuda().contiguous(memory_format=cl)
    outs = []
    for sel in (0, ops.SPARSE_HALVES):
        y = torch.empty(B, 64, H, W, device="cuda").contiguous(memory_format=cl)
        ops.conv_c64(dy2g, hip.view_plain(H, W, 128), pdb, None, (1, 64), y, hip.view_plain(H, W, 64), B, H, W, 128, 64, mask=t,
                     relu=ops.LEAKY_MASK, select=sel)
        outs.append(y)
    assert torch.equal(outs[0], outs[1])
    # masked weight gradients vs the full ones on the blocks that are read back
    dy2 = torch.randn(B, 128, H, W, generator=g).cuda().contiguous(memory_format=cl)
    full, part = torch.empty(128, 64, 3, 3, device="cuda"), torch.full((128, 64, 3, 3), float("nan"), device="cuda")
    bf, bp = torch.empty(128, device="cuda"), torch.empty(128, device="cuda")
    ops.wgrad_c64(t, hip.view_plain(H, W, 64), dy2, hip.view_plain(H, W, 128), full, bf, B, H, W, 64, 128)
    ops.wgrad_c64(t, hip.view_plain(H, W, 64), dy2, hip.view_plain(H, W, 128), part, bp, B, H, W, 64, 128, active_units=0xC3)
    assert rel(part[:64, :32], full[:64, :32]) < 1e-6 and rel(part[64:, 32:], full[64:, 32:]) < 1e-6 and rel(bp, bf) < 1e-6
    assert torch.isnan(part[:64, 32:]).all() and torch.isnan(part[64:, :32]).all()  # skipped blocks are not written
    dt = torch.randn(B, 64, H, W, generator=g).cuda().contiguous(memory_format=cl)
    full, part = torch.empty(64, 128, 3, 3, device="cuda"), torch.full((64, 128, 3, 3), float("nan"), device="cuda")
    bf, bp = torch.empty(64, device="cuda"), torch.empty(64, device="cuda")
    ops.wgrad_c64(cat, hip.view_plain(H, W, 128), dt, hip.view_plain(H, W, 64), full, bf, B, H, W, 128, 64)
    ops.wgrad_c64(cat, hip.view_plain(H, W, 128), dt, hip.view_plain(H, W, 64), part, bp, B, H, W, 128, 64, active_units=0x3F)
    assert rel(part[:, :96], full[:, :96]) < 1e-6 and rel(bp, bf) < 1e-6 and torch.isnan(part[:, 96:]).all()


def test_sparse_select_codes_refuse_other_shapes():
    x = torch.zeros(1, 64, 8, 32, device="cuda").contiguous(memory_format=torch.channels_last)
    pf, _ = ops.pack_pair(torch.zeros(64, 64, 3, 3, device="cuda"))
    for sel in (ops.SPARSE_BLOCK_DIAGONAL, ops.SPARSE_SECOND_CHUNK, ops.SPARSE_HALVES):
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.conv_c64(x, hip.view_plain(8, 32, 64), pf, None, (1, 64), torch.empty_like(x), hip.view_plain(8, 32, 64), 1, 8, 32,
                         64, 64, select=sel)


def test_leaky_codes_are_refused_off_the_fp32_kernels():
    x = torch.zeros(1, 64, 8, 32, device="cuda").contiguous(memory_format=torch.channels_last)
    w = torch.zeros(64, 64, 3, 3, device="cuda")
    prev = ops.PRECISION
    try:
        ops.set_precision("bf16")
        pf, _ = ops.pack_pair(w)
        with pytest.raises(RuntimeError, match="unsupported"):
            ops.conv_c64(x, hip.view_plain(8, 32, 64), pf, None, (1, 64), torch.empty_like(x), hip.view_plain(8, 32, 64), 1, 8, 32,
                         64, 64, relu=ops.LEAKY)
        with pytest.raises(NotImplementedError):
            ops.sftmd_forward(None, x, x)
    finally:
        ops.set_precision(prev)


def test_f1_reduced_net_output_and_gradients():
    a, meta = load_golden("f1_sftmd_reduced")
    net = reduced_net().to("cuda:0")
    out = net(torch.from_numpy(a["in0"]).cuda(), torch.from_numpy(a["in1"]).cuda())
    np.testing.assert_allclose(out.detach().cpu().numpy(), a["out"], rtol=2e-4, atol=2e-5)
    out.backward(torch.from_numpy(a["cot"]).cuda())
    for k, p in net.named_parameters():
        gn = float(a["pgn/" + k])
        assert abs(float(p.grad.double().norm()) / gn - 1) < 1e-4, k
        np.testing.assert_allclose(p.grad.reshape(-1)[:32].cpu().numpy(), a["pg32/" + k], rtol=2e-3,
                                   atol=5e-5 * gn / np.sqrt(p.numel()) + 1e-9, err_msg=k)


@pytest.mark.parametrize("scale", [2, 3])
def test_other_scales_vs_oracle(scale):
    """x2 / x3: one conv -> PixelShuffle(scale) -> LeakyReLU stage (ref: :148-156), 256 / 576 shuffled channels.  The reference
    fixtures are x4; here the oracle (pinned at x4 by F1-F3) is the yardstick, in float64."""
    from oracle import sisr_oracle as O
    torch.manual_seed(8)
    net = sisr_amd.sftmd.SFTMD(in_nc=3, num_features=64, num_blocks=2, scale=scale, input_para=10)
    g = torch.Generator().manual_seed(40 + scale)
    x, maps = torch.rand(2, 3, 11, 13, generator=g), torch.rand(2, 10, 1, 1, generator=g).expand(2, 10, 11, 13).contiguous()
    cot = torch.randn(2, 3, 11 * scale, 13 * scale, generator=g)
    sd = {k: v.detach().double().requires_grad_(True) for k, v in net.state_dict().items()}
    want = O.sftmd(sd, x.double(), maps.double(), num_blocks=2, scale=scale)
    want.backward(cot.double())
    net.to("cuda:0")
    out = net(x.cuda(), maps.cuda())
    np.testing.assert_allclose(out.detach().cpu().numpy(), want.detach().float().numpy(), rtol=2e-4, atol=2e-5)
    out.backward(cot.cuda())
    for k, p in net.named_parameters():
        assert rel(p.grad, sd[k].grad) < 5e-5, k


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_f4_non_default_options_vs_reference(name):
    """SFT_type 'concat' / 'weak' / 'none', mask_para, repeats, q_injection with 2 and 3 FC layers (fixture f4: the reference's
    output and per-parameter gradient norms / leading values on reduced x2 nets).

    'weak1': its input is the one of 100 candidates whose closest LeakyReLU pre-activation lies furthest from zero (4.2e-6;
    tools/make_fixtures_sftmd.py) -- with round 2's input one of 59 904 lay 2.3e-7 from the kink, the MFMA conv's summation
    order landed on the other side of it than the reference's, and that single mask bit moved every upstream gradient by
    2e-3.  Same tolerance as the other variants now."""
    tol = 2e-4
    a = np.load(f"{sisr_amd.__path__[0]}/../tests/golden/f4_sftmd_variants.npz")
    net, kw, vector = variant_net(name)
    net.to("cuda:0")
    x, md = variant_inputs(a, name, vector)
    out = net(x.cuda(), md.cuda())
    np.testing.assert_allclose(out.detach().cpu().numpy(), a[f"{name}/out"], rtol=2e-4, atol=2e-5)
    out.backward(torch.from_numpy(a[f"{name}/cot"]).cuda())
    named = dict(net.named_parameters())
    keys = [k[len(name) + 5:] for k in a.files if k.startswith(name + "/pgn/")]
    assert sorted(keys) == sorted(k for k, p in named.items() if p.grad is not None)
    for k in keys:
        gn = float(a[f"{name}/pgn/{k}"])
        assert abs(float(named[k].grad.double().norm()) - gn) <= tol * gn + 1e-10, k
        np.testing.assert_allclose(named[k].grad.reshape(-1)[:8].cpu().numpy(), a[f"{name}/pg8/{k}"], rtol=25 * tol,
                                   atol=25 * tol * gn / np.sqrt(named[k].numel()) + 1e-9, err_msg=k)


def test_f2_set5_forward_psnr_parity_with_reference():
    ref = golden_json("f_sftmd")["full_depth"]["images"]
    crops = np.load(f"{sisr_amd.__path__[0]}/../tests/golden/f2_sftmd_crops.npz")
    h = build()
    for im, x, y, md in set5():
        if im not in ref:
            continue
        out, loss, _ = h.run_eval(x, y, request_loss=True, metadata=md, metadata_keys=[("blur_kernel",)] * 10)
        o = out[0].numpy()
        assert abs(sisr_amd.metrics.y_psnr(o, y[0].numpy()) - ref[im]["y_psnr"]) < 1e-3, im
        assert abs(float(loss) - ref[im]["l1"]) < 1e-5
        hh, ww = o.shape[1:]
        np.testing.assert_allclose(o[:, hh // 2 - 16:hh // 2 + 16, ww // 2 - 16:ww // 2 + 16], crops[im], rtol=1e-3, atol=1e-4)


def test_f3_run_train_trajectory_matches_reference():
    ref = golden_json("f_sftmd")["train_steps"]
    h = build(eval_mode=False, lr=1e-4, scheduler=ref["scheduler"], scheduler_params=ref["scheduler_params"])
    g = torch.Generator().manual_seed(77)
    for step in ref["steps"]:
        x, y = torch.rand(2, 3, 16, 16, generator=g), torch.rand(2, 3, 64, 64, generator=g)
        md = torch.rand(2, 10, generator=g, dtype=torch.float64) * 0.4
        assert abs(h.get_learning_rate() - step["lr_before"]) < 1e-12
        loss, out = h.run_train(x, y, metadata=md, metadata_keys=[("blur_kernel", "blur_kernel")] * 10)
        gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in h.net.parameters())))
        assert abs(float(loss) - step["loss"]) < 5e-6 and abs(gn / step["grad_norm"] - 1) < 2e-4
        assert abs(float(out.mean()) - step["out_mean"]) < 5e-5 and abs(h.get_learning_rate() - step["lr_after"]) < 1e-12
    psum = float(sum(v.double().sum() for v in h.net.state_dict().values()))
    assert abs(psum - ref["final_param_sum"]) < 5e-2


def test_handler_concat_strategy_and_da_injection():
    """ref: SFTMD_variants/handlers.py:7-22.  concat_strategy: the handler concatenates the metadata maps to the RGB batch
    (QModel.channel_concat_logic) and conv1 takes 3 + M channels; da_injection: the network ignores the flag (its constructor
    swallows it), the handler switches the metadata to per-sample vectors."""
    g = torch.Generator().manual_seed(4)
    x, y = torch.rand(2, 3, 16, 20, generator=g), torch.rand(2, 3, 32, 40, generator=g)
    md = torch.rand(2, 10, generator=g, dtype=torch.float64) * 0.4
    keys = [("blur_kernel",) * 2] * 10
    torch.manual_seed(8)
    h = sisr_amd.available_models["sftmd"](device=0, model_save_dir="/tmp", eval_mode=False, scale=2, lr=1e-4,
                                           metadata=["blur_kernel"], num_blocks=2, concat_strategy=True)
    assert h.channel_concat and tuple(h.net.conv1.weight.shape) == (64, 13, 3, 3) and not h.vector_metadata
    w0 = h.net.conv1.weight.detach().clone()
    for _ in range(3):
        loss = float(h.run_train(x, y, metadata=md, metadata_keys=keys)[0])
    assert np.isfinite(loss)
    g = h.net.conv1.weight.grad
    assert g is not None and float(g[:, :3].abs().sum()) > 0 and float(g[:, 3:].abs().sum()) > 0  # RGB and map channels learn
    assert float((h.net.conv1.weight.detach() - w0)[:, 3:].abs().max()) > 0
    out, _, _ = h.run_eval(x, metadata=md, metadata_keys=keys)
    assert tuple(out.shape) == (2, 3, 32, 40)
    torch.manual_seed(8)
    h = sisr_amd.available_models["sftmd"](device=0, model_save_dir="/tmp", eval_mode=False, scale=2, lr=1e-3,
                                           metadata=["blur_kernel"], num_blocks=2, da_injection=True, SFT_type="none")
    assert h.vector_metadata and not h.channel_concat
    ch = h.generate_channels(x, md, keys)
    assert tuple(ch.shape) == (2, 10, 1, 1)
