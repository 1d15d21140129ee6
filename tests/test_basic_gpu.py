"""SRCNN / VDSR on the HIP kernels (pytest -m gpu): the kernels of csrc/basic.hip against float64 on exact data, then the
networks and handlers against the reference's own vectors (fixtures: tools/make_fixtures_basic.py).

Kernel level: every operand is a small dyadic rational (tests/_exact.py), so after `assert_budget` every comparison is exact.
Model level: tolerances are those of tests/test_srmd_gpu.py for the same kinds of quantity."""
import numpy as np
import pytest
import torch

import _basic as R
import _exact as E
import sisr_amd
from conftest import golden_json, load_golden

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
DEV = "cuda:0"
CL = torch.channels_last
WIDTHS = [(64, 32), (32, 64), (64, 64), (32, 32), (48, 48)]  # (cin, cout); 48: zero-padded to 64 on both sides


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _f64(t):
    return t.detach().to(DEV).double().requires_grad_(True)


def _wgrad_budget(x, dy, k, what):
    E.wgrad_budget(x.to(DEV), dy.to(DEV), padding=k // 2, k=k, what=what)


# ----------------------------------------------------------------------------- Y -> features
@pytest.mark.parametrize("hw", R.SIZES)
@pytest.mark.parametrize("K", [3, 5, 9])
@pytest.mark.parametrize("cout, bias, relu", [(64, True, True), (32, False, True), (48, True, False), (64, False, False)])
def test_y2f_forward_and_weight_gradient_exact(hw, K, cout, bias, relu):
    H, W = hw
    cp = R.pad_width(cout)
    x, w = E.ints((R.B, 1, H, W), 11), E.weights((cout, 1, K, K), 12)
    b = E.biases(cout, 13) if bias else None
    cot = E.ints((R.B, cp, H, W), 14)  # cotangent on the padded channels too: it must not reach any gradient
    E.conv_budget(x.to(DEV), w.to(DEV), extras=(b,), padding=K // 2, what="y2f")
    wl, bl = _leaf(w), (_leaf(b) if bias else None)
    y = ops.conv_y2f(x.to(DEV), wl, bl, relu=relu)
    assert y.shape == (R.B, cp, H, W) and y.is_contiguous(memory_format=CL)
    w64, b64 = _f64(w), (_f64(b) if bias else None)
    ref = R.conv_act(x.to(DEV), w64, b64, relu)
    E.assert_exact(y[:, :cout], ref.detach(), "y2f output")
    assert not y[:, cout:].any(), "padded channels must be written as zero"
    _wgrad_budget(x, cot[:, :cout], K, "y2f weight gradient")
    y.backward(cot.to(DEV))
    ref.backward(cot[:, :cout].to(DEV).double())
    E.assert_exact(wl.grad, w64.grad, "y2f dw")
    if bias:
        E.assert_exact(bl.grad, b64.grad, "y2f db")
    first = wl.grad.clone()
    wl.grad = None
    ops.conv_y2f(x.to(DEV), wl, bl, relu=relu).backward(cot.to(DEV))
    assert torch.equal(first, wl.grad), "the weight gradient must be bit-identical run to run"


@pytest.mark.parametrize("hw", R.SIZES)
@pytest.mark.parametrize("K", [3, 5, 9])
def test_y2f_flipped_taps_and_mask_is_the_input_gradient_of_f2y(hw, K):
    """the raw entry point with flip_taps and a mask: conv of dy with the flipped weight, zero where the masking map <= 0"""
    H, W = hw
    hip, L = sisr_amd.hip, sisr_amd.hip.lib()
    cin, cp = 48, 64
    dy, w = E.ints((R.B, 1, H, W), 21), E.weights((1, cin, K, K), 22)
    m = R.to_map(E.ints((R.B, cp, H, W), 23, -1, 1), cp, DEV)
    E.conv_budget(dy.to(DEV), w.transpose(0, 1).to(DEV), padding=K // 2, what="y2f(flip)")
    out = torch.full((R.B, cp, H, W), float("nan"), device=DEV).contiguous(memory_format=CL)
    dyd, wd = dy.to(DEV), w.to(DEV)  # named: a temporary inside the call expression is released before the launch
    hip.check(L.sisr_convk_y2f(hip.ptr(dyd), hip.ptr(wd), None, hip.ptr(m), hip.ptr(out), R.B, H, W, K, cin, cp, 0, 1,
                               hip.stream()), "sisr_convk_y2f")
    ref = E.dgrad_ref(dyd, wd) * E.relu_mask(m[:, :cin])
    E.assert_exact(out[:, :cin], ref, "masked input gradient")
    assert not out[:, cin:].any()


# ----------------------------------------------------------------------------- features -> Y
@pytest.mark.parametrize("hw", R.SIZES)
@pytest.mark.parametrize("K", [3, 5, 9])
@pytest.mark.parametrize("cin, bias, residual", [(64, True, True), (32, False, False), (48, True, False), (64, False, True)])
def test_f2y_forward_and_gradients_exact(hw, K, cin, bias, residual):
    H, W = hw
    cp = R.pad_width(cin)
    x, w = E.ints((R.B, cin, H, W), 31), E.weights((1, cin, K, K), 32)
    b = E.biases(1, 33) if bias else None
    res = E.ints((R.B, 1, H, W), 34) if residual else None
    cot = E.ints((R.B, 1, H, W), 35)
    E.conv_budget(x.to(DEV), w.to(DEV), extras=(b, res), padding=K // 2, what="f2y")
    xl, wl = R.to_map(x, cp, DEV).requires_grad_(True), _leaf(w)
    bl, rl = (_leaf(b) if bias else None), (_leaf(res) if residual else None)
    y = ops.conv_f2y(xl, wl, bl, rl)
    x64, w64 = _f64(x), _f64(w)
    b64, r64 = (_f64(b) if bias else None), (_f64(res) if residual else None)
    ref = R.conv_act(x64, w64, b64, False, r64)
    E.assert_exact(y, ref.detach(), "f2y output")
    E.conv_budget(cot.to(DEV), w.transpose(0, 1).to(DEV), padding=K // 2, what="f2y input gradient")
    _wgrad_budget(x, cot, K, "f2y weight gradient")
    y.backward(cot.to(DEV))
    ref.backward(cot.to(DEV).double())
    E.assert_exact(xl.grad[:, :cin], x64.grad, "f2y dx")
    assert not xl.grad[:, cin:].any()
    E.assert_exact(wl.grad, w64.grad, "f2y dw")
    if bias:
        E.assert_exact(bl.grad, b64.grad, "f2y db")
    if residual:
        E.assert_exact(rl.grad, r64.grad, "f2y dresidual")
    first = (wl.grad.clone(), xl.grad.clone())
    wl.grad = xl.grad = None
    ops.conv_f2y(xl, wl, bl, rl).backward(cot.to(DEV))
    assert torch.equal(first[0], wl.grad) and torch.equal(first[1], xl.grad)


# ----------------------------------------------------------------------------- K x K on the matrix cores
def _kxk_case(H, W, K, cin, cout, bias, relu):
    cip, cop = R.pad_width(cin), R.pad_width(cout)
    x, w = E.ints((R.B, cin, H, W), 41, zeros=0.25), E.weights((cout, cin, K, K), 42)
    b = E.biases(cout, 43) if bias else None
    cot = E.ints((R.B, cop, H, W), 44)
    E.conv_budget(x.to(DEV), w.to(DEV), extras=(b,), padding=K // 2, what="kxk")
    xl, wl, bl = R.to_map(x, cip, DEV).requires_grad_(True), _leaf(w), (_leaf(b) if bias else None)
    y = ops.conv_kxk(xl, wl, bl, relu=relu)
    assert y.shape == (R.B, cop, H, W) and y.is_contiguous(memory_format=CL)
    x64, w64, b64 = _f64(x), _f64(w), (_f64(b) if bias else None)
    ref = R.conv_act(x64, w64, b64, relu)
    E.assert_exact(y[:, :cout], ref.detach(), "kxk output")
    assert not y[:, cout:].any(), "padded channels must be written as zero"
    E.conv_budget(cot[:, :cout].to(DEV), w.transpose(0, 1).to(DEV), padding=K // 2, what="kxk input gradient")
    _wgrad_budget(x, cot[:, :cout], K, "kxk weight gradient")
    y.backward(cot.to(DEV))
    ref.backward(cot[:, :cout].to(DEV).double())
    E.assert_exact(xl.grad[:, :cin], x64.grad, "kxk dx")
    assert not xl.grad[:, cin:].any()
    E.assert_exact(wl.grad, w64.grad, "kxk dw")
    if bias:
        E.assert_exact(bl.grad, b64.grad, "kxk db")
    first = (wl.grad.clone(), xl.grad.clone(), bl.grad.clone() if bias else None)
    wl.grad = xl.grad = None
    if bias:
        bl.grad = None
    ops.conv_kxk(xl, wl, bl, relu=relu).backward(cot.to(DEV))
    assert torch.equal(first[0], wl.grad) and torch.equal(first[1], xl.grad), "gradients must be bit-identical run to run"
    assert not bias or torch.equal(first[2], bl.grad)


@pytest.mark.parametrize("hw", R.SIZES)
@pytest.mark.parametrize("K", [1, 3, 5, 9])
@pytest.mark.parametrize("cin, cout", WIDTHS)
def test_kxk_mfma_forward_and_gradients_exact(hw, K, cin, cout):
    _kxk_case(hw[0], hw[1], K, cin, cout, bias=True, relu=True)


@pytest.mark.parametrize("bias, relu", [(False, False), (True, False), (False, True)])
def test_kxk_mfma_options(bias, relu):
    _kxk_case(9, 21, 5, 64, 32, bias, relu)
    _kxk_case(37, 70, 3, 48, 48, bias, relu)


@pytest.mark.parametrize("hw", R.SIZES)
def test_kxk_mfma_output_mask_epilogue(hw):
    """the raw entry point with the backward mask of the sisr_conv3x3_c64 convention: zero where the masking map <= 0"""
    H, W = hw
    hip = sisr_amd.hip
    x, w = E.ints((R.B, 64, H, W), 51), E.weights((32, 64, 5, 5), 52)
    m = R.to_map(E.ints((R.B, 32, H, W), 53, -1, 1), 32, DEV)
    E.conv_budget(x.to(DEV), w.to(DEV), padding=2, what="kxk")
    pf, _ = ops.pack_convk(w.to(DEV), need_dgrad=False)
    out = torch.full((R.B, 32, H, W), float("nan"), device=DEV).contiguous(memory_format=CL)
    ops.convk_mfma(R.to_map(x, 64, DEV), pf, None, 0, out, R.B, H, W, 5, 64, 32, mask=m)
    E.assert_exact(out, E.conv_ref(x.to(DEV), w.to(DEV)) * E.relu_mask(m), "masked conv")


# ----------------------------------------------------------------------------- MSE
def test_mse_loss_exact_at_a_power_of_two_and_close_at_a_ragged_size():
    a, b = E.ints((4, 1, 16, 16), 61) / 4, E.ints((4, 1, 16, 16), 62) / 4  # n = 1024: the division is exact
    al = _leaf(a)
    loss = ops.mse_loss(al, b.to(DEV))
    want, grad = R.mse_ref(a, b)
    E.assert_budget((a.double() - b.double()).pow(2).sum(), 1 / 16, "mse")
    E.assert_exact(loss, want, "mse loss")
    loss.backward()
    E.assert_exact(al.grad, grad, "mse gradient")
    g = torch.Generator().manual_seed(63)
    a, b = torch.rand(2, 1, 13, 22, generator=g), torch.rand(2, 1, 13, 22, generator=g)  # n = 572: the tail of the last block
    al = _leaf(a)
    loss = ops.mse_loss(al, b.to(DEV))
    want, grad = R.mse_ref(a, b)
    np.testing.assert_allclose(float(loss.detach()), float(want), rtol=1e-6)
    loss.backward()
    np.testing.assert_allclose(al.grad.cpu().double().numpy(), grad.detach().numpy(), rtol=1e-6, atol=1e-12)
    again = ops.mse_loss(a.to(DEV), b.to(DEV))
    assert torch.equal(again, loss.detach())


# ----------------------------------------------------------------------------- models
@pytest.mark.parametrize("name, cls", [("b1_srcnn", "SRCNN"), ("b1_vdsr_reduced", "VDSR")])
def test_b1_output_and_gradients(name, cls):
    """stored distance of the fixture from float64: output 9e-8 (max abs), gradients 8e-7 (relative norm); the tolerances
    of tests/test_srmd_gpu.py (2e-4 / 2e-5 on outputs, 5e-5 per gradient) are kept as they are"""
    a, meta = load_golden(name)
    cfg = {k: meta[k] for k in ("kernel_pattern", "channel_pattern") if k in meta}
    net = getattr(sisr_amd.basic, cls)(**cfg)
    net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in a.items() if k.startswith("sd/")}, strict=True)
    net.to(DEV)
    out = net(torch.from_numpy(a["in0"]).to(DEV))
    np.testing.assert_allclose(out.detach().cpu().numpy(), a["out"], rtol=2e-4, atol=2e-5)
    out.backward(torch.from_numpy(a["cot"]).to(DEV))
    for k, p in net.named_parameters():
        want = a["pg/" + k]
        err = np.linalg.norm(p.grad.cpu().numpy().ravel() - want.ravel()) / (np.linalg.norm(want.ravel()) + 1e-30)
        assert err < 5e-5, (k, err)


def _handler(name, eval_mode=True, **extra):
    torch.manual_seed(8)
    return sisr_amd.available_models[name](device=0, model_save_dir="/tmp", eval_mode=eval_mode, **extra)


@pytest.fixture(scope="module")
def set5_ycbcr():
    return R.set5_interp()


@pytest.mark.parametrize("name", ["srcnn", "vdsr"])
def test_b2_set5_y_psnr_parity_with_reference(name, set5_ycbcr):
    ref = golden_json("b_basic")["full_depth"][name]["images"]
    crops = np.load(f"{sisr_amd.__path__[0]}/../tests/golden/b2_{name}_crops.npz")
    h = _handler(name)
    for im, x, y in set5_ycbcr:
        out, loss, _ = h.run_eval(x[:, :1], y[:, :1], request_loss=True)
        o = out[0].numpy()
        assert abs(R.psnr(np.clip(o[0], 0, 1), y[0, 0].numpy()) - ref[im]["y_psnr"]) < 1e-3, im
        assert abs(float(loss) - ref[im]["mse"]) < 5e-6, im
        hh, ww = o.shape[1:]
        np.testing.assert_allclose(o[:, hh // 2 - 16:hh // 2 + 16, ww // 2 - 16:ww // 2 + 16], crops[im], rtol=1e-3, atol=1e-4)


def test_b2_model_interface_y_channel_branch(set5_ycbcr, tmp_path):
    """net_run_and_process on a Y-channel model: Y through the net, the input's Cb / Cr re-attached, back to RGB"""
    params = {"name": "vdsr", "internal_params": {"scale": 4, "kernel_pattern": [3] * 4, "channel_pattern": [1, 64, 64, 64, 1]}}
    torch.manual_seed(8)
    mi = sisr_amd.ModelInterface(str(tmp_path), "exp", gpu="single", sp_gpu=0, mode="train", new_params=params)
    im, x, y = set5_ycbcr[1]
    rgb, ycc, loss, _ = mi.net_run_and_process(lr=x, hr=y, request_loss=True)
    out, loss2, _ = mi.model.run_eval(x[:, :1], y[:, :1], request_loss=True)
    want = torch.cat([out, x[:, 1:]], 1).numpy()
    np.testing.assert_array_equal(ycc, np.clip(want, 0, 1))
    np.testing.assert_array_equal(rgb[0], sisr_amd.metrics.ycbcr_to_rgb_jpg(np.clip(want[0], 0, 1)))
    assert float(loss) == float(loss2)
    res = mi.net_run_process_and_measure(lr=x, hr=y, metrics=("SSIM",), request_loss=True)
    np.testing.assert_array_equal(res[1], ycc)
    host = sisr_amd.metrics.ssim(ycc[0, 0], np.clip(y[0, 0].numpy(), 0, 1), max_value=1)
    assert abs(res[4]["SSIM"][0] - host) < 1e-9  # the device kernel follows the host float64 form to 1e-12 (tests/test_ssim_gpu.py)


@pytest.mark.parametrize("name", ["srcnn", "vdsr"])
def test_b3_run_train_trajectory_matches_reference(name):
    ref = golden_json("b_basic")["train_steps"][name]
    h = _handler(name, eval_mode=False, lr=1e-4)
    g = torch.Generator().manual_seed(83)
    for step in ref["steps"]:
        x, y = torch.rand(2, 1, 24, 24, generator=g), torch.rand(2, 1, 24, 24, generator=g)
        loss, out = h.run_train(x, y)
        gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in h.net.parameters())))
        assert abs(float(loss) - step["loss"]) < 5e-6 and abs(gn / step["grad_norm"] - 1) < 1e-4, (float(loss), gn, step)
        assert abs(float(out.mean()) - step["out_mean"]) < 5e-5 and abs(h.get_learning_rate() - step["lr"]) < 1e-12
    psum = float(sum(v.double().sum() for v in h.net.state_dict().values()))
    assert abs(psum - ref["final_param_sum"]) < 5e-2


def test_vdsr_step_under_graph_capture_equals_eager():
    """BaseModel.use_graph: forward + MSE + backward of VDSR replayed from a hipGraph gives the eager trajectory"""
    runs = {}
    for mode in (False, True):
        h = _handler("vdsr", eval_mode=False, lr=1e-4, kernel_pattern=[3] * 5, channel_pattern=[1, 64, 64, 64, 64, 1])
        h.use_graph = mode
        g = torch.Generator().manual_seed(5)
        ls = []
        for _ in range(3):
            x, y = torch.rand(2, 1, 24, 40, generator=g), torch.rand(2, 1, 24, 40, generator=g)
            loss, out = h.train_step(x, y)
            ls.append((float(loss), float(out.double().sum())))
        runs[mode] = (ls, [p.detach().clone() for p in h.net.parameters()])
    for (la, oa), (lb, ob) in zip(runs[False][0], runs[True][0]):
        assert abs(la - lb) <= 1e-7 * abs(la) and abs(oa - ob) <= 1e-6 * abs(oa)
    for pa, pb in zip(runs[False][1], runs[True][1]):
        torch.testing.assert_close(pa, pb, rtol=1e-5, atol=1e-7)


def test_b4_train_sisr_on_hip_matches_the_reference_run(tmp_path):
    """the reference's own one-epoch srcnn run on Set5 (fixture b4: three batches of 32 x 32 Y crops, validation on the five
    YCbCr images) through train_sisr on the HIP kernels: losses to 5e-6, Y-PSNR to 1e-3 dB"""
    import os
    ref = golden_json("b4_train_sisr")["srcnn"]["summary"]
    cfg = R.b4_config(tmp_path)
    cfg["training"]["gpu"] = "single"
    cfg["training"]["sp_gpu"] = 0
    total = sisr_amd.cli.train_sisr(cfg)
    print({k: list(total[k]) for k in ("train-loss", "val-loss", "val-PSNR")}, ref)
    np.testing.assert_allclose(total["train-loss"], ref["train-loss"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(total["val-loss"], ref["val-loss"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(total["val-PSNR"], ref["val-PSNR"], rtol=0, atol=1e-3)
    np.testing.assert_allclose(total["learning-rate"], ref["learning-rate"], rtol=0, atol=1e-12)
    assert os.path.isfile(os.path.join(str(tmp_path), cfg["experiment"], "result_outputs", "summary.csv"))
    assert os.path.isfile(os.path.join(str(tmp_path), cfg["experiment"], "saved_models", "train_model_0"))


def test_bias_gradient_with_a_frozen_weight():
    """a trainable bias beside a frozen weight still gets its gradient (both come from one launch), the weight none"""
    H, W = 9, 21
    x = R.to_map(E.ints((R.B, 64, H, W), 71), 64, DEV)
    cases = [(ops.conv_f2y, E.weights((1, 64, 5, 5), 72), E.biases(1, 73), E.ints((R.B, 1, H, W), 74), {}),
             (ops.conv_kxk, E.weights((32, 64, 5, 5), 75), E.biases(32, 76), E.ints((R.B, 32, H, W), 77), {"relu": True})]
    for op, w, b, cot, kw in cases:
        grads = []
        for frozen in (False, True):
            wl, bl = w.to(DEV).requires_grad_(not frozen), _leaf(b)
            op(x, wl, bl, **kw).backward(cot.to(DEV))
            assert (wl.grad is None) == frozen
            grads.append(bl.grad)
        assert torch.equal(grads[0], grads[1])
