"""Degradation predictor, the parts that need no GPU: constructor refusals, the registry, QModel.channels_from_codes, the
argument checks of the new entry points (before any device call) and eval_sisr's metadata-list check."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _predictor as P
import sisr_amd
from conftest import GOLDEN


@pytest.mark.parametrize("kw, names", [({"num_outputs": 0}, "num_outputs"), ({"num_outputs": 65}, "num_outputs"),
                                       ({"kernel_size": 4}, "kernel_size"), ({"kernel_size": 11}, "kernel_size"),
                                       ({"num_features": 65}, "num_features"), ({"num_layers": 1}, "num_layers"),
                                       ({"in_channels": 33}, "in_channels")])
def test_constructor_refuses_what_the_kernels_cannot_run_and_names_the_limit(kw, names):
    with pytest.raises(NotImplementedError, match=names):
        sisr_amd.predictor.DegradationPredictor(**{"num_outputs": 12, **kw})


def test_limits_are_accepted_at_their_edges():
    net = sisr_amd.predictor.DegradationPredictor(in_channels=32, num_outputs=64, num_features=64, num_layers=2, kernel_size=9)
    assert list(net.state_dict()) == ["layer_dict.conv_0.weight", "layer_dict.conv_0.bias", "layer_dict.conv_1.weight",
                                      "layer_dict.conv_1.bias"]
    assert list(net.state_dict()) == list(P.Twin(32, 64, 64, 2, 9).state_dict())


def test_no_cpu_fallback():
    net = sisr_amd.predictor.DegradationPredictor(num_outputs=12, num_layers=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros(1, 3, 8, 8))


def test_registered_and_flagged():
    assert "predictor" in sisr_amd.available_models
    h = sisr_amd.available_models["predictor"](device="cpu", model_save_dir="/tmp", eval_mode=True, metadata=list(P.KEYS),
                                               num_layers=2)
    assert h.predicts_metadata is True and h.num_metadata == 12 and h.metadata == P.KEYS
    assert h.im_input == "unmodified" and h.colorspace == "rgb"
    assert isinstance(h.criterion, sisr_amd.basic.MSELoss)
    assert not hasattr(sisr_amd.available_models["qrcan"], "predicts_metadata")


def test_target_codes_follow_the_key_mask():
    h = sisr_amd.available_models["predictor"](device="cpu", model_save_dir="/tmp", eval_mode=True, metadata=list(P.KEYS),
                                               num_layers=2)
    md, keys, want = P.metadata_batch(3, 5)
    got = h.target_codes(torch.zeros(3, 3, 4, 4), md, keys)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    with pytest.raises(RuntimeError, match="Metadata needs to be specified"):
        h.target_codes(torch.zeros(3, 3, 4, 4), None, None)


@pytest.mark.parametrize("style", ["standard", "modulate"])
def test_channels_from_codes_equals_generate_channels(style):
    """the same values through the metadata route and through the code route, with and without the 'modulate' curve (which
    reads one value per image: QPI)"""
    meta = ["qpi"] if style == "modulate" else list(P.KEYS)
    h = sisr_amd.available_models["qrcan"](device="cpu", model_save_dir="/tmp", eval_mode=True, scale=4, style=style,
                                           metadata=meta, n_resgroups=1, n_resblocks=1)
    B = 3
    if style == "modulate":
        md = torch.rand(B, 1, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
        keys, codes = [tuple("qpi" for _ in range(B))], md.float()
    else:
        md, keys, codes = P.metadata_batch(B, 4)
    want = h.generate_channels(torch.zeros(B, 3, 4, 4), md, keys)
    got = h.channels_from_codes(codes)
    assert got.dtype == want.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got, want)
    assert want.shape == ((B, 64, 1, 1) if style == "modulate" else (B, 12, 1, 1))
    with pytest.raises(ValueError, match="entries per image"):
        h.channels_from_codes(torch.zeros(B, h.num_metadata + 1))


def test_new_entry_points_refuse_bad_arguments_before_any_device_call():
    """null pointers, bad K, bad widths, misaligned maps, a short workspace and a NaN slope: an error code and no launch (so
    this runs without a GPU), in the manner of test_abi's test_round4_entry_points_refuse_..."""
    hip = sisr_amd.hip
    L = hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)  # non-null stand-in: every call below fails before it is dereferenced
    a += (-a) % 16
    ARG, ALIGN, UNSUPPORTED = -1, -2, -4
    conv = lambda **k: L.sisr_convk_mfma_leaky(*_args(  # noqa: E731
        dict(x=a, in_mask=None, packed=a, bias=None, nbias=0, y=a, B=1, H=8, W=8, K=5, cin_p=64, cout_p=32, act=1, slope=0.2,
             stream=None), k))
    assert conv(x=None) == ARG and conv(packed=None) == ARG and conv(y=None) == ARG and conv(B=0) == ARG
    assert conv(slope=float("nan")) == ARG and conv(slope=float("inf")) == ARG
    assert conv(K=4) == UNSUPPORTED and conv(K=11) == UNSUPPORTED and conv(cin_p=48) == UNSUPPORTED
    assert conv(cout_p=16) == UNSUPPORTED and conv(nbias=33) == UNSUPPORTED
    assert conv(x=a + 4) == ALIGN and conv(in_mask=a + 4) == ALIGN and conv(packed=a + 8) == ALIGN
    ws = L.sisr_wgradk_mfma_workspace_bytes(1, 8, 8, 5, 64, 32)
    wgrad = lambda **k: L.sisr_wgradk_mfma_leaky(*_args(  # noqa: E731
        dict(x=a, dy=a, dymask=a, dw=a, db=None, B=1, H=8, W=8, K=5, cout=32, cin=64, cop=32, cip=64, ws=a, nb=ws, slope=0.2,
             stream=None), k))
    assert wgrad(x=None) == ARG and wgrad(dy=None) == ARG and wgrad(dymask=None) == ARG and wgrad(dw=None) == ARG
    assert wgrad(ws=None) == ARG and wgrad(nb=ws - 4) == ARG and wgrad(slope=float("nan")) == ARG and wgrad(H=0) == ARG
    assert wgrad(K=2) == UNSUPPORTED and wgrad(cop=48) == UNSUPPORTED and wgrad(cout=33) == UNSUPPORTED
    assert wgrad(cin=65) == UNSUPPORTED
    nb = L.sisr_map_mean_workspace_bytes(2, 37, 70, 32)
    assert nb == 8 * 2 * 6 * 32  # 2590 pixels in parts of 512: six float64 partials per image and channel
    assert L.sisr_map_mean_workspace_bytes(2, 37, 70, 48) == 0 and L.sisr_map_mean_workspace_bytes(0, 37, 70, 32) == 0
    mean = lambda **k: L.sisr_map_mean(*_args(  # noqa: E731
        dict(x=a, out=a, B=2, H=37, W=70, c=12, cp=32, ws=a, nb=nb, stream=None), k))
    assert mean(x=None) == ARG and mean(out=None) == ARG and mean(ws=None) == ARG and mean(nb=nb - 8) == ARG
    assert mean(c=0) == ARG and mean(W=0) == ARG
    assert mean(cp=48) == UNSUPPORTED and mean(c=33) == UNSUPPORTED
    assert mean(x=a + 4) == ALIGN and mean(ws=a + 4) == ALIGN
    bwd = lambda **k: L.sisr_map_mean_bwd(*_args(  # noqa: E731
        dict(g=a, dx=a, B=2, H=37, W=70, c=12, cp=32, stream=None), k))
    assert bwd(g=None) == ARG and bwd(dx=None) == ARG and bwd(B=0) == ARG and bwd(c=0) == ARG
    assert bwd(cp=16) == UNSUPPORTED and bwd(c=40) == UNSUPPORTED and bwd(dx=a + 4) == ALIGN


def _args(defaults, override):
    assert set(override) <= set(defaults)
    return list({**defaults, **override}.values())


def test_ops_refuse_both_activations_and_a_bad_slope():
    x, w = torch.zeros(1, 32, 4, 4), torch.zeros(8, 3, 3, 3)
    with pytest.raises(ValueError, match="relu and slope"):
        sisr_amd.ops.conv_kxk(x, w, None, relu=True, slope=0.2)
    with pytest.raises(ValueError, match="finite"):
        sisr_amd.ops.conv_kxk(x, w, None, slope=float("nan"))
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP device"):
        sisr_amd.ops.conv_kxk(x, w, None, slope=0.2)
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP device"):
        sisr_amd.ops.map_mean(x.contiguous(memory_format=torch.channels_last), 12)


def test_eval_sisr_refuses_a_model_whose_metadata_list_differs_before_any_forward(tmp_path, monkeypatch):
    """CPU models: the check needs no device and runs before an image is read or a network is run"""
    q = {"name": "qrcan", "internal_params": {"scale": 4, "style": "standard", "metadata": ["blur_kernel", "noise"],
                                              "n_resgroups": 1, "n_resblocks": 1}}
    p = {"name": "predictor", "internal_params": {"scale": 4, "metadata": ["noise", "blur_kernel"], "num_layers": 2}}
    P.save_experiment(sisr_amd, tmp_path, "q", q, gpu=False)
    P.save_experiment(sisr_amd, tmp_path, "p", p, gpu=False)

    def boom(*a, **k):
        raise AssertionError("a network ran before the metadata lists were compared")
    monkeypatch.setattr(sisr_amd.handlers.BaseModel, "run_eval", boom)
    monkeypatch.setattr(sisr_amd.cli, "SuperResImages", boom)
    set5 = os.path.join(GOLDEN, "set5")
    with pytest.raises(ValueError) as err:
        sisr_amd.cli.eval_sisr(model_and_epoch=[["q", "0"]], metadata_predictor=["p", 0], model_loc=str(tmp_path), gpu=False,
                               hr_dir=os.path.join(set5, "hr"), lr_dir=os.path.join(set5, "lr_random_blur"),
                               full_directory=True, scale=4, out_loc=str(tmp_path), results_name="ev")
    assert "['blur_kernel', 'noise']" in str(err.value) and "['noise', 'blur_kernel']" in str(err.value)
    with pytest.raises(ValueError, match="predicts no degradation code"):
        sisr_amd.cli.eval_sisr(model_and_epoch=[["q", "0"]], metadata_predictor=["q", 0], model_loc=str(tmp_path), gpu=False,
                               hr_dir=os.path.join(set5, "hr"), lr_dir=os.path.join(set5, "lr_random_blur"),
                               full_directory=True, scale=4, out_loc=str(tmp_path), results_name="ev")


def test_best_epoch_of_a_predictor_is_the_lowest_validation_loss(tmp_path):
    import pandas as pd
    p = {"name": "predictor", "internal_params": {"scale": 4, "metadata": list(P.KEYS), "num_layers": 2}}
    mi = P.save_experiment(sisr_amd, tmp_path, "p", p, gpu=False)
    for e in (1, 2):
        mi.set_epoch(e)
        mi.save()
    pd.DataFrame({"train-loss": [3., 2., 1.], "val-loss": [0.5, 0.2, 0.3], "val-MAE": [0.6, 0.4, 0.3],
                  "epoch": [0, 1, 2]}).to_csv(os.path.join(mi.logs, "summary.csv"), index=False)
    assert sisr_amd.ModelInterface(str(tmp_path), "p", mode="eval", load_epoch="best").model_epoch == 1
    assert sisr_amd.ModelInterface(str(tmp_path), "p", mode="eval", load_epoch="last").model_epoch == 2
    assert np.isfinite(mi.model.print_parameters())


def test_handlers_that_build_their_own_maps_get_the_codes_as_keyed_metadata():
    """SRMD / SFTMD make metadata maps inside run_eval: eval_sisr hands them the predicted code as the batch's metadata with
    one key per entry, and what they build from it is the code, entry by entry, over the image"""
    keys = ["blur_kernel", "noise"]
    srmd = sisr_amd.available_models["srmd"](device=torch.device("cpu"), model_save_dir="/tmp", eval_mode=True, scale=4,
                                             metadata=keys, nc=64, nb=3)
    pred = sisr_amd.available_models["predictor"](device="cpu", model_save_dir="/tmp", eval_mode=True, metadata=keys,
                                                  num_layers=2)
    codes = torch.rand(2, 11, generator=torch.Generator().manual_seed(3))
    batch = {"lr": torch.zeros(2, 3, 5, 6), "hr": torch.zeros(2, 3, 20, 24), "tag": ["a", "b"], "metadata": torch.zeros(2),
             "metadata_keys": []}
    feed = sisr_amd.cli._with_predicted_codes(srmd, pred, batch, codes)
    assert "extra_channels" not in feed and len(feed["metadata_keys"]) == 11 and feed["metadata_keys"][10] == ("noise", "noise")
    maps = srmd.generate_sft_channels(feed["lr"], feed["metadata"], feed["metadata_keys"])
    assert torch.equal(maps, codes[:, :, None, None].expand(2, 11, 5, 6))
    q = sisr_amd.available_models["qrcan"](device="cpu", model_save_dir="/tmp", eval_mode=True, scale=4, style="standard",
                                           metadata=keys, n_resgroups=1, n_resblocks=1)
    feed = sisr_amd.cli._with_predicted_codes(q, pred, batch, codes)
    assert "metadata" not in feed and torch.equal(feed["extra_channels"], codes[:, :, None, None])
    assert sisr_amd.cli._code_columns(pred) == ["blur_kernel_%d" % i for i in range(10)] + ["noise"]
