"""IKC's Corrector on the HIP kernels (pytest -m gpu).

Kernel level: the pointwise layers of up to 128 channels with a per-image bias, and their gradients, against float64 on the
exact data of tests/_exact.py (after `assert_budget` every comparison is exact).
Model level: DegradationCorrector against the float64 twin of tests/_corrector.py (a real torch.cat), with the bound and the
kink protocol of tests/test_predictor_gpu.py.
Handler level: CorrectorHandler and IKC's loop around reduced frozen models, then train_sisr and eval_sisr's `ikc` key."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _corrector as T
import _exact as E
import _predictor as P
import sisr_amd
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
DEV = "cuda:0"
CL = torch.channels_last
B = 3  # three images with three different bias rows: an image index taken from the wrong grid dimension shows


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _f64(t):
    return t.detach().double().requires_grad_(True)


def _to_map(t, cp):
    b, c, h, w = t.shape
    out = torch.zeros((b, cp, h, w), dtype=torch.float32).contiguous(memory_format=CL)
    out[:, :c] = t.float()
    return out.to(DEV)


# ----------------------------------------------------------------------------- 1. pointwise layers, exact
@pytest.mark.parametrize("hw", [(1, 1), (3, 11), (37, 70)])  # 1, 33 and 2590 pixels: one lane, one M-tile + 1, many workgroups
@pytest.mark.parametrize("cip", [32, 64, 128])
@pytest.mark.parametrize("cop", [32, 64, 128])
@pytest.mark.parametrize("with_image_bias", [False, True])
@pytest.mark.parametrize("slope", [0.5, None])
def test_pointwise_forward_and_gradients_exact(hw, cip, cop, with_image_bias, slope):
    H, W = hw
    cin, cout = cip - 3, cop - 7  # ragged real widths: the padded channels are written as zero and take no gradient
    x, w = E.ints((B, cin, H, W), 241, zeros=0.25), E.weights((cout, cin, 1, 1), 242)
    b, ib = E.biases(cout, 243), (E.ints((B, cout), 244, -8, 8) / 8 if with_image_bias else None)
    cot = E.ints((B, cop, H, W), 245)  # a cotangent on the padded channels too
    mag = F.conv2d(x.double().abs(), w.double().abs()) + b.double().abs().view(1, -1, 1, 1) + 1.0
    E.assert_budget(mag, E.granule(x) * E.granule(w), "pointwise")
    xl, wl, bl = _to_map(x, cip).requires_grad_(True), _leaf(w), _leaf(b)
    il = _leaf(ib) if with_image_bias else None
    y = ops.conv_1x1(xl, wl, bl, slope=slope, image_bias=il)
    assert y.shape == (B, cop, H, W) and y.is_contiguous(memory_format=CL)
    x64, w64, b64 = _f64(x), _f64(w), _f64(b)
    i64 = _f64(ib) if with_image_bias else None
    pre = F.conv2d(x64, w64, b64)
    if with_image_bias:
        assert len({tuple(r.tolist()) for r in ib}) == B, "test bug: the bias rows must differ"
        pre = pre + i64[:, :, None, None]
    ref = pre if slope is None else F.leaky_relu(pre, slope)
    E.assert_exact(y[:, :cout], ref.detach(), "pointwise output")
    assert not y[:, cout:].any(), "padded channels must be written as zero"
    c = cot[:, :cout]
    gc = E.granule(c) if slope is None else E.granule(c * slope, c)
    E.assert_budget(F.conv2d(c.double().abs(), w.double().abs().transpose(0, 1)), gc * E.granule(w), "pointwise dx")
    E.assert_budget(torch.einsum("bohw,bchw->oc", c.double().abs(), x.double().abs()), gc * E.granule(x), "pointwise dw")
    E.assert_budget(c.double().abs().sum(dim=(0, 2, 3)), gc, "pointwise db")
    y.backward(cot.to(DEV))
    ref.backward(c.double())
    E.assert_exact(xl.grad[:, :cin], x64.grad, "pointwise dx")
    assert not xl.grad[:, cin:].any(), "padded input channels take no gradient"
    E.assert_exact(wl.grad, w64.grad, "pointwise dw")
    E.assert_exact(bl.grad, b64.grad, "pointwise db")
    if with_image_bias:
        assert il.grad.shape == (B, cout)
        E.assert_exact(il.grad, i64.grad, "pointwise d image_bias")  # the float64 per-image sum
    first = [t.grad.clone() for t in (xl, wl, bl) + ((il,) if with_image_bias else ())]
    for t in (xl, wl, bl, il):
        if t is not None:
            t.grad = None
    ops.conv_1x1(xl, wl, bl, slope=slope, image_bias=il).backward(cot.to(DEV))
    again = [t.grad for t in (xl, wl, bl) + ((il,) if with_image_bias else ())]
    assert all(torch.equal(p, q) for p, q in zip(first, again)), "gradients must be bit-identical run to run"


def test_pointwise_gradients_read_the_mask_map_not_the_sign_of_dy():
    """raw entry points with a mask map unrelated to the output: dy_eff = m > 0 ? dy : slope * dy with m drawn on its own"""
    H, W, cin, cout, cip, cop, slope = 37, 70, 64, 128, 64, 128, 0.25
    hip, L = sisr_amd.hip, sisr_amd.hip.lib()
    x, w = E.ints((B, cin, H, W), 251), E.weights((cout, cin, 1, 1), 252)
    dy, m = E.ints((B, cout, H, W), 253), E.ints((B, cout, H, W), 254, -1, 1)
    eff = dy.double() * E.leaky_mask(m, slope)
    assert ((dy > 0) & (m <= 0)).any() and ((dy < 0) & (m > 0)).any(), "test bug: sign of dy and mask never disagree"
    E.assert_budget(torch.einsum("bohw,bchw->oc", dy.double().abs(), x.double().abs()), 0.25, "pointwise dw")
    xm, dym, mm = _to_map(x, cip), _to_map(dy, cop), _to_map(m, cop)
    wd = w.to(DEV)
    packed = torch.empty((2, cop * cip), device=DEV)
    hip.check(L.sisr_pack_conv1(hip.ptr(wd), hip.ptr(packed[0]), hip.ptr(packed[1]), cout, cin, cop, cip, hip.stream()), "pack")
    dx = torch.full((B, cip, H, W), float("nan"), device=DEV).contiguous(memory_format=CL)
    hip.check(L.sisr_conv1_mfma_leaky(hip.ptr(dym), hip.ptr(mm), hip.ptr(packed[1]), None, None, 0, hip.ptr(dx), B, H, W, cop, cip,
                                      0, slope, hip.stream()), "sisr_conv1_mfma_leaky(dgrad)")
    E.assert_exact(dx, F.conv2d(eff, w.double().transpose(0, 1)), "pointwise dgrad through a foreign mask")
    dw, db = torch.full_like(w, float("nan")).to(DEV), torch.full((cout,), float("nan"), device=DEV)
    dib = torch.full((B, cout), float("nan"), device=DEV)
    nb = L.sisr_wgrad1_mfma_workspace_bytes(B, H, W, cip, cop)
    ws = hip.workspace(torch.device(DEV), nb)
    hip.check(L.sisr_wgrad1_mfma_leaky(hip.ptr(xm), hip.ptr(dym), hip.ptr(mm), hip.ptr(dw), hip.ptr(db), hip.ptr(dib), B, H, W,
                                       cout, cin, cop, cip, hip.ptr(ws), nb, slope, hip.stream()), "sisr_wgrad1_mfma_leaky")
    E.assert_exact(dw[:, :, 0, 0], torch.einsum("bohw,bchw->oc", eff, x.double()), "pointwise wgrad through a foreign mask")
    E.assert_exact(dib, eff.sum(dim=(2, 3)), "per-image bias gradient through a foreign mask")
    E.assert_exact(db, eff.sum(dim=(0, 2, 3)), "bias gradient through a foreign mask")


# ----------------------------------------------------------------------------- 2. the network against its float64 twin
@pytest.mark.parametrize("shape", [(2, 3, 9, 21), (2, 3, 37, 70)])
@pytest.mark.parametrize("M", [1, 12])
@pytest.mark.parametrize("num_features", [64, 48])
def test_corrector_output_and_gradients_against_the_float64_twin(shape, M, num_features):
    """relative L2 distance of the output, of every parameter gradient and of the gradient of the code from float64 < 5e-5,
    the predictor test's bound, with its kink protocol: inside |z64| < KINK the reference takes the branch the HIP forward
    took, and at most two elements of a case are decided that way."""
    cfg = dict(num_codes=M, num_features=num_features)
    net = sisr_amd.corrector.DegradationCorrector(**cfg)
    sd = T.kaiming_state(net, 260 + M + num_features)
    assert list(sd) == list(T.Twin(**cfg).state_dict())
    net.load_state_dict(sd, strict=True)
    net.to(DEV)
    g = torch.Generator().manual_seed(261)
    x, codes = torch.rand(shape, generator=g), torch.rand((shape[0], M), generator=g)
    cot = torch.randn((shape[0], M), generator=g)
    cl = _leaf(codes)
    out = net(x.to(DEV), cl)
    assert out.shape == (shape[0], M)
    out.backward(cot.to(DEV))
    branches, replay = T.hip_branches(ops, net, x.to(DEV), codes.to(DEV))
    assert torch.equal(replay, out.detach()) and len(branches) == T.SITES
    ref, c64 = T.twin(sd, **cfg), _f64(codes)
    want, decided = ref(x.double(), c64, branches=branches)
    assert decided <= 2
    want.backward(cot.double())
    assert 0.005 < float(want.detach().abs().mean()) < 10, "test bug: degenerate outputs"
    worst = P.rel_l2(out, want)
    assert worst < 5e-5, ("output", worst)
    err = P.rel_l2(cl.grad, c64.grad)
    worst = max(worst, err)
    assert err < 5e-5, ("codes", err)
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        err = P.rel_l2(p.grad, q.grad)
        worst = max(worst, err)
        assert err < 5e-5, (k, err)
    print("corrector parity", shape, cfg, "largest relative L2 distance from float64: %.3g" % worst, "at-the-kink:", decided)


# ----------------------------------------------------------------------------- 3. the handler and IKC's loop
SFTMD = {"name": "sftmd", "internal_params": {"scale": 4, "metadata": ["blur_kernel"], "num_blocks": 2, "num_features": 64,
                                              "in_nc": 3}}  # the F-fixtures' configuration at two blocks; M = 10
QRCAN = {"name": "qrcan", "internal_params": {"scale": 4, "style": "standard", "include_q_layer": True, "n_resgroups": 2,
                                              "n_resblocks": 2, "metadata": list(P.KEYS)}}
PRED = {"name": "predictor", "internal_params": {"scale": 4, "metadata": list(P.KEYS), "num_layers": 3, "num_features": 32}}


def _corrector_params(sr="q", predictor="p", metadata=P.KEYS, **extra):
    ip = {"scale": 4, "lr": 1e-4, "metadata": list(metadata), "num_features": 32, "sr_model": [sr, 0], "iterations": 2}
    if predictor:
        ip["predictor"] = [predictor, 0]
    ip.update(extra)
    return {"name": "corrector", "internal_params": ip}


def _handler(tmp_path, eval_mode=False, **extra):
    torch.manual_seed(8)
    return sisr_amd.available_models["corrector"](device=0, model_save_dir=os.path.join(str(tmp_path), "c", "saved_models"),
                                                  eval_mode=eval_mode, **_corrector_params(**extra)["internal_params"])


def test_run_train_trajectory_matches_the_float64_twin_with_adam(tmp_path):
    """three batches of two iterations (six optimiser steps) around a reduced SFTMD, no predictor (the loop starts at 0.5),
    against torch.optim.Adam on the float64 twin from the same weights: each step's loss within 5e-6 and gradient norm within
    1e-4 relative, the bounds of the predictor's trajectory test.  The handler's steps are made by hand from its public calls
    (super_resolve, train_step), so every step's loss shows; run_train on a second handler must then give the same bits."""
    P.save_experiment(sisr_amd, tmp_path, "s", SFTMD, gpu=True)
    kw = dict(sr="s", predictor=None, metadata=["blur_kernel"])
    h, whole = _handler(tmp_path, **kw), _handler(tmp_path, **kw)
    sd = T.kaiming_state(h.net, 281)
    h.net.load_state_dict(sd)
    whole.net.load_state_dict(sd)
    ref = T.twin(sd, num_codes=10, num_features=32)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(282)
    for batch in range(3):
        x = torch.rand(2, 3, 16, 24, generator=g)
        md, keys, _ = P.metadata_batch(2, 283 + batch)
        target = h.target_codes(x, md, keys)
        assert target.shape == (2, 10) and torch.equal(target.cpu(), md[:, :10].float())
        code = h.initial_codes(x.to(DEV))
        assert torch.equal(code, torch.full((2, 10), 0.5, device=DEV))
        c64 = code.double().cpu()
        for it in range(2):
            sr = h.super_resolve(x.to(DEV), code)
            assert sr.shape == (2, 3, 64, 96) and sr.is_cuda
            loss, code = h.train_step(sr, target, extra_channels=code)
            gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in h.net.parameters())))
            opt.zero_grad()
            sr64 = h.super_resolve(x.to(DEV), c64.float().to(DEV)).double().cpu()
            want = c64 + ref(sr64, c64)
            wl = F.mse_loss(want, target.double().cpu())
            wl.backward()
            wn = float(torch.sqrt(sum((p.grad ** 2).sum() for p in ref.parameters())))
            print("batch", batch, "iteration", it, float(loss), float(wl), gn, wn)
            assert abs(float(loss) - float(wl)) < 5e-6 and abs(gn / wn - 1) < 1e-4, (batch, it, float(loss), float(wl), gn, wn)
            opt.step()
            c64 = want.detach()
        last, out = whole.run_train(x, torch.full((2, 3, 64, 96), float("nan")), metadata=md, metadata_keys=keys, tag=["a", "b"])
        assert out.shape == (2, 10) and not out.is_cuda and torch.equal(out, code.cpu()) and float(last) == float(loss)
    for (k, p), q, r in zip(h.net.named_parameters(), ref.parameters(), whole.net.parameters()):
        assert P.rel_l2(p, q) < 1e-5 and torch.equal(p, r), k


def test_step_under_graph_capture_equals_eager(tmp_path):
    """forward + MSE + backward of a step replayed from a hipGraph gives the eager trajectory bit for bit (the handler's
    default queue count is left alone)"""
    P.save_experiment(sisr_amd, tmp_path, "q", QRCAN, gpu=True)
    runs = {}
    for mode in (False, True):
        h = _handler(tmp_path, predictor=None)
        h.use_graph = mode
        g = torch.Generator().manual_seed(285)
        ls = []
        for step in range(2):
            x = torch.rand(2, 3, 16, 24, generator=g)
            md, keys, _ = P.metadata_batch(2, 286 + step)
            loss, out = h.run_train(x, None, metadata=md, metadata_keys=keys)
            ls.append((float(loss), out.clone()))
        runs[mode] = (ls, [p.detach().clone() for p in h.net.parameters()])
        assert bool(h._graphs) == mode
    for (la, oa), (lb, ob) in zip(runs[False][0], runs[True][0]):
        assert la == lb and torch.equal(oa, ob)
    for pa, pb in zip(runs[False][1], runs[True][1]):
        assert torch.equal(pa, pb)


def test_correct_equals_the_loop_written_out_by_hand(tmp_path):
    P.save_experiment(sisr_amd, tmp_path, "q", QRCAN, gpu=True)
    P.save_experiment(sisr_amd, tmp_path, "p", PRED, gpu=True)
    h = _handler(tmp_path, eval_mode=True)
    h.net.load_state_dict(T.kaiming_state(h.net, 291))
    x = torch.rand(2, 3, 19, 23, generator=torch.Generator().manual_seed(292))
    sr, final, history = h.correct(x, iterations=3)
    assert sr.shape == (2, 3, 76, 92) and len(history) == 4 and final is history[-1]
    with torch.no_grad():
        code = h.frozen["predictor"].model.run_eval(x, keep_on_device=True)[0]
        assert torch.equal(history[0], code)
        for it in range(3):
            code = code + h.net(h.super_resolve(x.to(DEV), code), code)
            assert torch.equal(history[it + 1], code), it
            assert not torch.equal(history[it + 1], history[it])
        assert torch.equal(sr, h.super_resolve(x.to(DEV), code))
    # codes handed in replace the predictor's; the default number of iterations is the handler's; run_eval is the loop
    start = torch.rand(2, 12, generator=torch.Generator().manual_seed(293))
    _, final2, history2 = h.correct(x, start, want_sr=False)
    assert len(history2) == 3 and torch.equal(history2[0], start.to(DEV))
    assert torch.equal(h.run_eval(x, extra_channels=start)[0], final2.cpu())


def test_sr_model_with_another_metadata_list_is_refused(tmp_path):
    P.save_experiment(sisr_amd, tmp_path, "s", SFTMD, gpu=True)
    with pytest.raises(ValueError) as err:
        _handler(tmp_path, sr="s", predictor=None)
    assert "sr_model 's' reads the metadata ['blur_kernel']" in str(err.value) and str(P.KEYS) in str(err.value)


def test_checkpoint_round_trip_through_the_model_interface(tmp_path):
    P.save_experiment(sisr_amd, tmp_path, "q", QRCAN, gpu=True)
    P.save_experiment(sisr_amd, tmp_path, "p", PRED, gpu=True)
    params = _corrector_params(lr=1e-3, ema_decay=0.5)
    torch.manual_seed(8)
    mi = sisr_amd.ModelInterface(str(tmp_path), "c", gpu="single", sp_gpu=0, mode="train", new_params=params)
    assert set(mi.model.state_dict()) == {"net." + k for k in mi.model.net.state_dict()}  # the frozen models are not its own
    g = torch.Generator().manual_seed(295)
    for _ in range(2):
        md, keys, _ = P.metadata_batch(2, 296)
        mi.train_batch(lr=torch.rand(2, 3, 16, 20, generator=g), hr=None, metadata=md, metadata_keys=keys)
    mi.save()
    sisr_amd.cli._dump_toml({"model": params}, os.path.join(mi.base_folder, "config.toml"))
    x = torch.rand(2, 3, 19, 23, generator=g)
    want, none, _ = mi.model.run_eval(x)
    with mi.model.averaged_weights():
        want_ema, _, _ = mi.model.run_eval(x)
    assert none is None and want.shape == (2, 12) and not torch.equal(want, want_ema)
    back = sisr_amd.ModelInterface(str(tmp_path), "c", gpu="single", sp_gpu=0, mode="eval", load_epoch=0)
    assert back.configuration == {"input": "unmodified", "colorspace": "rgb"}
    assert torch.equal(back.model.run_eval(x)[0], want)
    ema = sisr_amd.ModelInterface(str(tmp_path), "c", gpu="single", sp_gpu=0, mode="eval", load_epoch=0, ema=True)
    assert torch.equal(ema.model.run_eval(x)[0], want_ema)
    md, keys, target = P.metadata_batch(2, 297)
    codes, loss, _ = back.model.run_eval(x, metadata=md, metadata_keys=keys, request_loss=True, keep_on_device=True)
    assert codes.is_cuda and abs(float(loss) - float(F.mse_loss(codes.cpu().double(), target.double()))) < 1e-6


@pytest.mark.parametrize("degrade_tiles", [False, True])
def test_train_sisr_trains_the_corrector_from_online_degradations(tmp_path, monkeypatch, degrade_tiles):
    """tests/_predictor.train_config with the corrector's keys: the Set5 HR images degraded online, a reduced net around a
    reduced QRCAN and predictor; validation records val-loss and val-MAE of the final code and no image metric"""
    import pandas as pd
    real = sisr_amd.degrade.pca_matrix
    monkeypatch.setattr(sisr_amd.degrade, "pca_matrix", lambda batch=2000, k=10: real(batch=2000, k=k))
    P.save_experiment(sisr_amd, tmp_path, "q", QRCAN, gpu=True)
    P.save_experiment(sisr_amd, tmp_path, "p", PRED, gpu=True)
    cfg = P.train_config(tmp_path, experiment="corr", **({"device_tiles": True, "degrade_tiles": True} if degrade_tiles else {}))
    cfg["model"] = _corrector_params()
    cfg["training"]["num_epochs"] = 1
    before = {k: v.clone() for k, v in sisr_amd.ModelInterface(str(tmp_path), "q", gpu="single", sp_gpu=0, mode="eval",
                                                               load_epoch=0).model.net.state_dict().items()}
    total = sisr_amd.cli.train_sisr(cfg)
    summary = pd.read_csv(os.path.join(str(tmp_path), "corr", "result_outputs", "summary.csv"))
    assert {"train-loss", "val-loss", "val-MAE", "learning-rate", "epoch"} == set(summary.columns)
    assert "val-PSNR" not in total and len(total["val-loss"]) == 1
    assert np.isfinite(summary.values).all() and (summary["val-MAE"] > 0).all()
    best = sisr_amd.ModelInterface(str(tmp_path), "corr", gpu="single", sp_gpu=0, mode="eval", load_epoch="best")
    assert best.model_epoch == 0 and best.model.iterations == 2
    after = best.model.frozen["sr_model"].model.net.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before), "the SR model is frozen"


def _ikc_fixture(tmp_path, corrector_metadata=None):
    P.save_experiment(sisr_amd, tmp_path, "q", QRCAN, gpu=True)
    P.save_experiment(sisr_amd, tmp_path, "p", PRED, gpu=True)
    if corrector_metadata is not None:  # a corrector of another list, around a Q-model and a predictor of that list
        other = {"name": "qrcan", "internal_params": dict(QRCAN["internal_params"], metadata=list(corrector_metadata))}
        P.save_experiment(sisr_amd, tmp_path, "q2", other, gpu=True)
        return P.save_experiment(sisr_amd, tmp_path, "c", _corrector_params(sr="q2", predictor=None,
                                                                            metadata=corrector_metadata), gpu=True)
    return P.save_experiment(sisr_amd, tmp_path, "c", _corrector_params(), gpu=True)


def _ikc_common(tmp_path):
    return dict(model_and_epoch=[["q", "0"]], model_loc=str(tmp_path), gpu=True, hr_dir=os.path.join(GOLDEN, "set5", "hr"),
                lr_dir=P.lr_folder_without_metadata(tmp_path), full_directory=True, scale=4, out_loc=str(tmp_path),
                time_models=False)


@pytest.mark.parametrize("device_outputs", [False, True])
def test_eval_sisr_with_ikc_feeds_the_final_code_to_the_q_model(tmp_path, device_outputs):
    """rows named '~ikc', iterations + 1 code rows per image (iteration 0: the predictor's), and the final row is exactly
    what the Q-model was given: the same evaluation from a metadata file holding the final rows has the same PSNR bits"""
    import json
    import pandas as pd
    _ikc_fixture(tmp_path)
    common = dict(_ikc_common(tmp_path), device_outputs=device_outputs or None)
    df, _ = sisr_amd.cli.eval_sisr(results_name="ev_ikc", metadata_predictor=["p", 0],
                                   ikc={"corrector": ["c", 0], "iterations": 3}, save_im=True, **common)
    names = sorted(f for f in os.listdir(common["lr_dir"]) if f.endswith(".png"))
    assert set(df["Model"]) == {"q~ikc"} and sorted(df["Image_Name"]) == names and np.isfinite(df["PSNR"]).all()
    assert sorted(os.listdir(os.path.join(str(tmp_path), "ev_ikc", "q~ikc"))) == names
    codes = pd.read_csv(os.path.join(str(tmp_path), "ev_ikc", "standard_metrics", "predicted_metadata.csv"))
    cols = ["blur_kernel_%d" % i for i in range(10)] + ["noise", "jpeg_quality"]
    assert list(codes.columns) == ["Image_Name", "iteration"] + cols and len(codes) == 4 * len(names)
    for n in names:
        assert list(codes[codes["Image_Name"] == n]["iteration"]) == [0, 1, 2, 3]
    plain, _ = sisr_amd.cli.eval_sisr(results_name="ev_pred", metadata_predictor=["p", 0], **common)
    first = pd.read_csv(os.path.join(str(tmp_path), "ev_pred", "standard_metrics", "predicted_metadata.csv"))
    zero = codes[codes["iteration"] == 0].drop(columns="iteration").reset_index(drop=True)
    assert zero.equals(first) and set(plain["Model"]) == {"q"} and list(plain["PSNR"]) != list(df["PSNR"])
    vals = codes[codes["iteration"] == 3].set_index("Image_Name")
    meta = pd.DataFrame({"blur_kernel": [json.dumps([float(vals.loc[n, c]) for c in cols[:10]]) for n in names],
                         "noise": [json.dumps([float(vals.loc[n, "noise"])]) for n in names],
                         "jpeg_quality": [json.dumps([float(vals.loc[n, "jpeg_quality"])]) for n in names]}, index=names)
    meta_file = os.path.join(str(tmp_path), "from_codes.csv")
    meta.to_csv(meta_file)
    again, _ = sisr_amd.cli.eval_sisr(results_name="ev_file", metadata_file=meta_file, **common)
    assert list(again["Image_Name"]) == list(df["Image_Name"]) and list(again["PSNR"]) == list(df["PSNR"])
    both, _ = sisr_amd.cli.eval_sisr(results_name="ev_both", metadata_predictor=["p", 0], metadata_file=meta_file,
                                     ikc={"corrector": ["c", 0], "iterations": 3}, **common)
    mae = pd.read_csv(os.path.join(str(tmp_path), "ev_both", "standard_metrics", "predicted_metadata.csv"))
    assert (mae[mae["iteration"] == 3]["code_MAE"] == 0).all() and (mae[mae["iteration"] == 0]["code_MAE"] > 0).all()


def test_eval_sisr_with_ikc_and_self_ensemble(tmp_path):
    _ikc_fixture(tmp_path)
    df, _ = sisr_amd.cli.eval_sisr(results_name="ev", metadata_predictor=["p", 0], ikc={"corrector": ["c", 0]},
                                   self_ensemble=True, **_ikc_common(tmp_path))
    assert set(df["Model"]) == {"q~ikc+"} and len(df) == 5 and np.isfinite(df["PSNR"]).all()


def test_eval_sisr_refuses_ikc_without_a_predictor_or_with_another_metadata_list(tmp_path):
    _ikc_fixture(tmp_path, corrector_metadata=["blur_kernel", "jpeg_quality", "noise"])
    common = _ikc_common(tmp_path)
    with pytest.raises(ValueError, match="ikc: the loop corrects the code of metadata_predictor"):
        sisr_amd.cli.eval_sisr(results_name="ev", ikc={"corrector": ["c", 0]}, **common)
    with pytest.raises(ValueError) as err:
        sisr_amd.cli.eval_sisr(results_name="ev", metadata_predictor=["p", 0], ikc={"corrector": ["c", 0]}, **common)
    assert "['blur_kernel', 'jpeg_quality', 'noise']" in str(err.value) and str(P.KEYS) in str(err.value)
    assert not os.path.exists(os.path.join(str(tmp_path), "ev", "standard_metrics"))
