"""SRCNN / VDSR (basic.py): registry, seed-8 weights, handler attributes, the Y-channel data path and the float64
restatement against the reference's own vectors (CPU; fixtures: tools/make_fixtures_basic.py)."""
import os

import numpy as np
import pytest
import torch

import _basic as R
import sisr_amd
from conftest import GOLDEN, golden_json, load_golden
from test_init_parity import digest

CPU = torch.device("cpu")


def build(name, eval_mode=True, **extra):
    torch.manual_seed(8)
    return sisr_amd.available_models[name](device=CPU, model_save_dir="/tmp", eval_mode=eval_mode, **extra)


def test_registry_lists_both_models():
    assert sisr_amd.available_models["srcnn"] is sisr_amd.basic.SRCNNHandler
    assert sisr_amd.available_models["vdsr"] is sisr_amd.basic.VDSRHandler
    assert sisr_amd.basic.SRCNNHandler in sisr_amd.handlers.HANDLERS


@pytest.mark.parametrize("name", ["srcnn", "vdsr"])
def test_b2_seed8_keys_and_digest_match_the_reference(name):
    ref = golden_json("b_basic")["full_depth"][name]
    h = build(name)
    sd = h.net.state_dict()
    assert list(sd) == ref["keys"] and len(sd) == ref["n_tensors"]
    assert int(sum(p.numel() for p in h.net.parameters())) == ref["n_params"]
    assert digest(sd) == ref["sha256"], "initial weights differ from the reference's for seed 8"


def test_handler_attributes():
    ref = golden_json("b_basic")
    for name, clip in (("srcnn", None), ("vdsr", 0.1)):
        h = build(name, eval_mode=False)
        assert h.model_name == name and h.colorspace == "ycbcr" == ref["full_depth"][name]["colorspace"]
        assert h.im_input == "interp" == ref["full_depth"][name]["im_input"]
        assert h.grad_clip == clip == ref["train_steps"][name]["grad_clip"]
        assert isinstance(h.criterion, sisr_amd.basic.MSELoss) and h.get_learning_rate() == 1e-4
    assert build("vdsr").net.depth == 20 and build("srcnn").net.depth == 3
    assert build("vdsr", grad_clip=0).grad_clip is None
    h = build("vdsr", kernel_pattern=[3, 5, 3], channel_pattern=[1, 16, 48, 1])
    assert [tuple(m.weight.shape) for m in h.net.layer_dict.values()] == [(16, 1, 3, 3), (48, 16, 5, 5), (1, 48, 3, 3)]


def test_layer_routing():
    """ends -> the Y kernels; runs of 3 x 3 64 -> 64 -> conv_chain; every other inner layer -> the K x K MFMA kernel"""
    plan = build("vdsr").net.plan()
    assert [(k, len(ls)) for k, ls in plan] == [("chain", 18)]
    assert [(k, len(ls)) for k, ls in build("srcnn").net.plan()] == [("kxk", 1)]
    net = sisr_amd.basic.SRCNN(kernel_pattern=[3, 3, 3, 5, 3, 3, 3], channel_pattern=[1, 64, 64, 64, 64, 64, 32, 1])
    assert [(k, len(ls)) for k, ls in net.plan()] == [("chain", 2), ("kxk", 1), ("chain", 1), ("kxk", 1)]


@pytest.mark.parametrize("kwargs, limit", [
    (dict(padding=0), "same"),
    (dict(kernel_pattern=[11, 5, 5]), "up to 9"),
    (dict(kernel_pattern=[4, 5, 5]), "odd"),
    (dict(channel_pattern=[3, 64, 32, 1]), "one channel"),
    (dict(channel_pattern=[1, 64, 32, 3]), "one channel"),
    (dict(channel_pattern=[1, 128, 32, 1]), "1 to 64"),
    (dict(kernel_pattern=[9, 5], channel_pattern=[1, 64, 32, 1]), "one more entry"),
])
def test_unsupported_patterns_are_refused_by_name(kwargs, limit):
    for cls in (sisr_amd.basic.SRCNN, sisr_amd.basic.VDSR):
        with pytest.raises(NotImplementedError, match=limit):
            cls(**kwargs)


def test_cpu_tensors_are_refused():
    ops = sisr_amd.ops
    x, f = torch.zeros(1, 1, 8, 8), torch.zeros(1, 64, 8, 8).contiguous(memory_format=torch.channels_last)
    match = "no CPU fallback|HIP device"
    with pytest.raises(RuntimeError, match=match):
        ops.conv_y2f(x, torch.zeros(64, 1, 9, 9), torch.zeros(64), relu=True)
    with pytest.raises(RuntimeError, match=match):
        ops.conv_f2y(f, torch.zeros(1, 64, 5, 5), torch.zeros(1))
    with pytest.raises(RuntimeError, match=match):
        ops.conv_kxk(f, torch.zeros(32, 64, 5, 5), torch.zeros(32), relu=True)
    with pytest.raises(RuntimeError, match=match):
        ops.mse_loss(x, x)
    with pytest.raises(RuntimeError, match=match):
        build("srcnn").net(x)


def test_new_entry_points_refuse_bad_arguments_before_any_device_call():
    import ctypes as C
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    ARG, UNSUPPORTED = -1, -4
    assert L.sisr_convk_y2f(None, a, a, None, a, 1, 8, 8, 3, 64, 64, 1, 0, None) == ARG
    assert L.sisr_convk_y2f(a, a, a, None, a, 1, 8, 8, 4, 64, 64, 1, 0, None) == UNSUPPORTED      # even kernel
    assert L.sisr_convk_y2f(a, a, a, None, a, 1, 8, 8, 11, 64, 64, 1, 0, None) == UNSUPPORTED     # kernel above 9
    assert L.sisr_convk_y2f(a, a, a, None, a, 1, 8, 8, 3, 65, 64, 1, 0, None) == UNSUPPORTED      # wider than the map
    assert L.sisr_convk_y2f(a, a, a, None, a, 1, 8, 8, 3, 48, 48, 1, 0, None) == UNSUPPORTED      # map not 32 / 64 wide
    assert L.sisr_convk_f2y(a, a, a, None, a, 0, 8, 8, 3, 64, 64, None) == ARG
    assert L.sisr_convk_f2y(a, a, a, None, a, 1, 8, 8, 3, 33, 32, None) == UNSUPPORTED
    assert L.sisr_corrk_y_workspace_bytes(1, 8, 8, 4, 64) == 0
    assert L.sisr_corrk_y_workspace_bytes(2, 9, 21, 5, 64) == 4 * 2 * 2 * 26 * 64                   # 4 tiles x (25 taps + bias) x 64
    assert L.sisr_corrk_y(a, a, None, a, a, 1, 8, 8, 3, 64, 64, 0, 1, a, 16, None) == ARG           # workspace too small
    assert L.sisr_corrk_y(a, a, None, a, None, 1, 8, 8, 3, 64, 64, 0, 1, a, 1 << 20, None) == ARG   # db_mode without db
    assert L.sisr_pack_convk(a, a, a, 5, 32, 65, 32, 64, None) == UNSUPPORTED
    assert L.sisr_convk_mfma(a, None, a, a, 32, None, a, 1, 8, 8, 5, 48, 32, 1, None) == UNSUPPORTED
    assert L.sisr_convk_mfma(a, None, None, a, 32, None, a, 1, 8, 8, 5, 64, 32, 1, None) == ARG
    assert L.sisr_wgradk_mfma_workspace_bytes(1, 8, 8, 5, 64, 48) == 0
    assert L.sisr_wgradk_mfma(a, a, None, a, a, 1, 8, 8, 5, 32, 64, 32, 64, a, 16, None) == ARG     # workspace too small
    assert L.sisr_mse_loss_workspace_bytes() == 2048
    assert L.sisr_mse_loss(a, a, 0, a, None, a, None) == ARG


def test_ycbcr_inverse_round_trips_and_equals_the_reference_formula():
    M = sisr_amd.metrics
    rgb = np.random.default_rng(3).random((3, 17, 23))
    ycc = M.rgb_to_ycbcr_jpg(rgb)
    assert np.abs(M.ycbcr_to_rgb_jpg(ycc) - rgb).max() < 1e-6
    bias = 128. * (1 / 255)  # ref: sr_tools/image_manipulation.py:100-105
    want = np.array([ycc[0] + 1.402 * ycc[2] - 1.402 * bias,
                     ycc[0] - 0.344136 * ycc[1] - 0.714136 * ycc[2] + (0.714136 + 0.344136) * bias,
                     ycc[0] + 1.772 * ycc[1] - 1.772 * bias])
    np.testing.assert_array_equal(M.ycbcr_to_rgb_jpg(ycc), want)
    batch = torch.from_numpy(np.stack([ycc, ycc * 1.5 - 0.2]).astype(np.float32))  # the second one leaves [0, 1]: clipped first
    got = sisr_amd.ModelInterface.colorspace_convert(batch, colorspace="ycbcr")
    np.testing.assert_array_equal(got[1], M.ycbcr_to_rgb_jpg(np.clip(batch[1].numpy(), 0, 1)))
    torch_ycc = sisr_amd.data.rgb_to_ycbcr(torch.from_numpy(rgb).float(), y_only=False)
    np.testing.assert_array_equal(torch_ycc.numpy(), R.jpg_ycbcr(torch.from_numpy(rgb).float()).numpy())


def test_dataset_shapes_in_ycbcr():
    d = os.path.join(GOLDEN, "set5")
    kw = dict(lr_dir=os.path.join(d, "hr"), hr_dir=os.path.join(d, "hr"), split="all", scale=4, input="interp",
              colorspace="ycbcr")
    train = sisr_amd.data.SuperResImages(**kw)[0]  # y_only defaults to True, as a training split gets it
    ev = sisr_amd.data.SuperResImages(y_only=False, **kw)[0]
    h, w = ev["hr"].shape[1:]
    assert train["lr"].shape == (1, h, w) == train["hr"].shape and ev["lr"].shape == (3, h, w)
    np.testing.assert_array_equal(train["lr"][0].numpy(), ev["lr"][0].numpy())
    rgb = sisr_amd.data.SuperResImages(**dict(kw, colorspace="rgb"))[0]["lr"]
    np.testing.assert_array_equal(ev["lr"].numpy(), R.jpg_ycbcr(rgb).numpy())
    sets = {"a": {"name": "set5", "lr": kw["lr_dir"], "hr": kw["hr_dir"], "cutoff": 5}}
    tr, va = sisr_amd.data.sisr_data_setup(sets, sets, batch_size=1, dataloader_threads=0, scale=4, input="interp",
                                           colorspace="ycbcr")
    assert tr.dataset[0]["lr"].shape[0] == 1 and va.dataset[0]["lr"].shape[0] == 3  # ref: training/data_setup.py:75
    with pytest.raises(NotImplementedError):
        sisr_amd.data.SuperResImages(**dict(kw, colorspace="lab"))


@pytest.mark.parametrize("name, residual", [("b1_srcnn", False), ("b1_vdsr_reduced", True)])
def test_b1_float64_restatement_reproduces_the_reference(name, residual):
    a, meta = load_golden(name)
    sd = {k[3:]: torch.from_numpy(v).double().requires_grad_(True) for k, v in a.items() if k.startswith("sd/")}
    out = R.net_ref(sd, torch.from_numpy(a["in0"]), residual)
    np.testing.assert_allclose(out.detach().numpy(), a["out"], rtol=1e-5, atol=1e-6)
    out.backward(torch.from_numpy(a["cot"]).double())
    for k, v in sd.items():
        want = a["pg/" + k]
        err = np.linalg.norm(v.grad.numpy().ravel() - want.ravel()) / np.linalg.norm(want.ravel())
        assert err < 4 * max(meta["grad_rel_err"][k], 1e-7), (k, err)  # the stored distance is from this very evaluation
    assert meta["out_err_max"] < 1e-6


def test_png_ycbcr_equals_the_reference_formula():
    """conv_type other than 'jpg': the studio-range BT.601 form (ref: sr_tools/image_manipulation.py:78-87)"""
    img = torch.rand(3, 9, 11, generator=torch.Generator().manual_seed(4))
    got = sisr_amd.data.rgb_to_ycbcr(img, y_only=False, im_type="png")
    y = 16. * (1 / 255) + (65.481 * img[0, :, :] + 128.553 * img[1, :, :] + 24.966 * img[2, :, :]) / 255.
    cb = 128. * (1 / 255) + (-37.797 * img[0, :, :] - 74.203 * img[1, :, :] + 112.0 * img[2, :, :]) / 255.
    cr = 128. * (1 / 255) + (112.0 * img[0, :, :] - 93.786 * img[1, :, :] - 18.214 * img[2, :, :]) / 255.
    np.testing.assert_array_equal(got.numpy(), torch.stack([y, cb, cr], 0).numpy())
    only = sisr_amd.data.rgb_to_ycbcr(img, y_only=True, im_type="png")
    assert only.shape == (1, 9, 11) and torch.equal(only[0], y)
    d = os.path.join(GOLDEN, "set5", "hr")
    kw = dict(lr_dir=d, hr_dir=d, split="all", scale=1, input="interp")
    rgb = sisr_amd.data.SuperResImages(**kw)[0]["lr"]
    png = sisr_amd.data.SuperResImages(colorspace="ycbcr", conv_type="png", y_only=False, **kw)[0]["lr"]
    np.testing.assert_array_equal(png.numpy(), sisr_amd.data.rgb_to_ycbcr(rgb, y_only=False, im_type="png").numpy())


def test_b4_train_loop_matches_reference_with_float32_torch_net(tmp_path, monkeypatch):
    """the reference's own one-epoch srcnn run on Set5 (fixture b4) through train_sisr, with the handler's parameters driven by
    a plain torch forward (test-only): pins everything around the kernels for a Y-channel model -- 'ycbcr' data sets with Y
    alone for training and YCbCr for validation, (B,1,H,W) batches, RNG call order, the non-RGB validation branch, Y-PSNR
    against the YCbCr reference, summary.csv"""
    ref = golden_json("b4_train_sisr")["srcnn"]["summary"]
    cfg = R.b4_config(tmp_path)
    real_init = sisr_amd.cli.ModelInterface.__init__

    def patched(self, *a, **k):
        real_init(self, *a, **k)
        net = self.model.net
        net.forward = lambda x: R.net_ref(dict(net.state_dict(keep_vars=True)), x, False, dtype=torch.float32)
        self.model.criterion = torch.nn.MSELoss()
    monkeypatch.setattr(sisr_amd.cli.ModelInterface, "__init__", patched)
    total = sisr_amd.cli.train_sisr(cfg)
    for key in ("train-loss", "val-loss", "val-PSNR", "learning-rate"):
        np.testing.assert_allclose(total[key], ref[key], rtol=2e-5, atol=2e-6, err_msg=key)
    assert list(total["epoch"]) == [0]
    assert os.path.isfile(os.path.join(str(tmp_path), cfg["experiment"], "result_outputs", "summary.csv"))
