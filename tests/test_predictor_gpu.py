"""Degradation predictor on the HIP kernels (pytest -m gpu).

Kernel level: the LeakyReLU forms of the K x K MFMA conv and its gradients, and the global mean of a map, against float64 on
exact data (tests/_exact.py: after `assert_budget` every comparison is exact).  With the dyadic slopes 0.25 and 0.5 every
gradient product stays exact too; at the network's slope 0.2 the forward is one fp32 rounding (E.leaky_ref) and the gradients
are compared at model level.
Model level: DegradationPredictor and PredictorHandler against the float64 torch.nn twin of tests/_predictor.py, with the
bounds of tests/test_basic_gpu.py for the same kinds of quantity; then train_sisr and eval_sisr."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _basic as R
import _exact as E
import _predictor as P
import sisr_amd
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
DEV = "cuda:0"
CL = torch.channels_last
WIDTHS = [(64, 64), (64, 32), (32, 64), (48, 48)]  # (cin, cout); 48: zero-padded to 64 on both sides


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _f64(t):
    return t.detach().to(DEV).double().requires_grad_(True)


# ----------------------------------------------------------------------------- 1. leaky conv_kxk, dyadic slopes: all exact
def _leaky_case(H, W, K, cin, cout, slope):
    cip, cop = R.pad_width(cin), R.pad_width(cout)
    x, w = E.ints((R.B, cin, H, W), 41, zeros=0.25), E.weights((cout, cin, K, K), 42)
    b = E.biases(cout, 43)
    cot = E.ints((R.B, cop, H, W), 44)  # a cotangent on the padded channels too: it must not reach any gradient
    E.conv_budget(x.to(DEV), w.to(DEV), extras=(b,), padding=K // 2, what="leaky kxk")
    xl, wl, bl = R.to_map(x, cip, DEV).requires_grad_(True), _leaf(w), _leaf(b)
    y = ops.conv_kxk(xl, wl, bl, slope=slope)
    assert y.shape == (R.B, cop, H, W) and y.is_contiguous(memory_format=CL)
    x64, w64, b64 = _f64(x), _f64(w), _f64(b)
    pre = E.conv_ref(x64, w64, b64)
    ref = F.leaky_relu(pre, slope)
    if K == 1:  # (short contractions hit 0 often; the long ones need not)
        assert int((pre.detach() == 0).sum()) > 0, "test bug: no exact zero of the pre-activation to exercise the convention at 0"
    E.assert_exact(y[:, :cout], ref.detach(), "leaky kxk output")  # slope * v is exact: v is on the 1/8 grid, far inside 24 bits
    assert not y[:, cout:].any(), "padded channels must be written as zero"
    # the gradient kernels contract dy_eff = dy or slope * dy: budgets on the cotangent as it is (|slope| <= 1), on the granule
    # of slope * cot
    E.assert_budget(E.conv_ref(cot[:, :cout].to(DEV).abs(), w.transpose(0, 1).to(DEV).abs(), padding=K // 2),
                    E.granule(cot * slope, cot) * E.granule(w), "leaky kxk input gradient")
    _wgrad_budget(x, cot[:, :cout], slope, K)
    y.backward(cot.to(DEV))
    ref.backward(cot[:, :cout].to(DEV).double())
    E.assert_exact(xl.grad[:, :cin], x64.grad, "leaky kxk dx")
    assert not xl.grad[:, cin:].any(), "padded input channels take no gradient"
    E.assert_exact(wl.grad, w64.grad, "leaky kxk dw")
    E.assert_exact(bl.grad, b64.grad, "leaky kxk db")
    first = (wl.grad.clone(), xl.grad.clone(), bl.grad.clone())
    wl.grad = xl.grad = bl.grad = None
    ops.conv_kxk(xl, wl, bl, slope=slope).backward(cot.to(DEV))
    assert torch.equal(first[0], wl.grad) and torch.equal(first[1], xl.grad) and torch.equal(first[2], bl.grad), \
        "gradients must be bit-identical run to run"


def _wgrad_budget(x, cot, slope, K):
    """budget of dw / db with dy_eff in {cot, slope * cot}: magnitudes of cot (|slope| <= 1), granule of slope * cot"""
    mag = E.wgrad_ref(x.to(DEV).double().abs(), cot.to(DEV).double().abs(), padding=K // 2, k=K)
    gran = E.granule(x) * E.granule(cot * slope, cot)
    E.assert_budget(mag, gran, "leaky kxk weight gradient")
    E.assert_budget(cot.double().abs().sum(dim=(0, 2, 3)), E.granule(cot * slope, cot), "leaky kxk bias gradient")


@pytest.mark.parametrize("hw", R.SIZES)
@pytest.mark.parametrize("K", [1, 3, 5, 9])
@pytest.mark.parametrize("cin, cout", WIDTHS)
@pytest.mark.parametrize("slope", [0.25, 0.5])
def test_leaky_kxk_forward_and_gradients_exact(hw, K, cin, cout, slope):
    _leaky_case(hw[0], hw[1], K, cin, cout, slope)


# ----------------------------------------------------------------------------- 2. slope 0.2: the forward is one rounding
@pytest.mark.parametrize("hw", R.SIZES)
@pytest.mark.parametrize("K", [1, 3, 5, 9])
@pytest.mark.parametrize("cin, cout", WIDTHS)
def test_leaky_kxk_forward_at_slope_02_is_one_fp32_rounding(hw, K, cin, cout):
    H, W = hw
    x, w, b = E.ints((R.B, cin, H, W), 45, zeros=0.25), E.weights((cout, cin, K, K), 46), E.biases(cout, 47)
    E.conv_budget(x.to(DEV), w.to(DEV), extras=(b,), padding=K // 2, what="leaky kxk")
    y = ops.conv_kxk(R.to_map(x, R.pad_width(cin), DEV), w.to(DEV), b.to(DEV), slope=0.2)
    E.assert_exact(y[:, :cout], E.leaky_ref(E.conv_ref(x.to(DEV), w.to(DEV), b.to(DEV))), "leaky kxk output, slope 0.2f")
    assert not y[:, cout:].any()


def test_relu_and_leaky_paths_do_not_share_a_select():
    """slope = 0 through the leaky path is the multiply (-0 where v < 0); relu=True keeps fmaxf (+0): bitwise different zeros,
    equal values -- the ReLU path was not re-routed through the product"""
    x, w = E.ints((R.B, 64, 9, 21), 48), E.weights((32, 64, 3, 3), 49)
    a = ops.conv_kxk(R.to_map(x, 64, DEV), w.to(DEV), None, relu=True)
    b = ops.conv_kxk(R.to_map(x, 64, DEV), w.to(DEV), None, slope=0.0)
    assert torch.equal(a, b)  # -0 == +0
    neg = E.conv_ref(x.to(DEV), w.to(DEV)) < 0
    assert neg.any() and not torch.signbit(a[neg]).any() and torch.signbit(b[neg]).all()


# ----------------------------------------------------------------------------- 3. map_mean
@pytest.mark.parametrize("hw", [(8, 16), (32, 64)])
@pytest.mark.parametrize("cp, c", [(32, 12), (32, 32), (64, 48), (64, 12)])
def test_map_mean_exact_where_the_pixel_count_is_a_power_of_two(hw, cp, c):
    H, W = hw
    x = E.ints((R.B, cp, H, W), 51)  # padded channels hold data too: they must neither be read into the result nor get gradient
    E.assert_budget(x.double().abs().sum(dim=(2, 3)), 1.0, "map_mean")
    xl = x.contiguous(memory_format=CL).to(DEV).requires_grad_(True)
    out = ops.map_mean(xl, c)
    assert out.shape == (R.B, c) and out.is_contiguous()
    E.assert_exact(out, x[:, :c].double().mean(dim=(2, 3)), "map_mean")
    g = E.ints((R.B, c), 52)
    out.backward(g.to(DEV))
    want = (g.double() / (H * W))[:, :, None, None].expand(R.B, c, H, W)
    assert xl.grad.is_contiguous(memory_format=CL)
    E.assert_exact(xl.grad[:, :c], want, "map_mean gradient")
    assert not xl.grad[:, c:].any(), "padded channels take no gradient"
    again = ops.map_mean(xl.detach(), c)
    assert torch.equal(again, out.detach())


@pytest.mark.parametrize("hw", [(37, 70), (5, 7)])
@pytest.mark.parametrize("cp, c", [(32, 12), (64, 48), (64, 64)])
def test_map_mean_at_ragged_sizes(hw, cp, c):
    H, W = hw
    g0 = torch.Generator().manual_seed(53)
    x = torch.rand((R.B, cp, H, W), generator=g0) + 0.25
    xl = x.contiguous(memory_format=CL).to(DEV).requires_grad_(True)
    out = ops.map_mean(xl, c)
    np.testing.assert_allclose(out.detach().cpu().double().numpy(), x[:, :c].double().mean(dim=(2, 3)).numpy(), rtol=1e-6)
    g = torch.rand((R.B, c), generator=g0) - 0.5
    out.backward(g.to(DEV))
    want = E.fp32_round(g.double() / (H * W))[:, :, None, None].expand(R.B, c, H, W)  # one fp32 division per value
    E.assert_exact(xl.grad[:, :c], want, "map_mean gradient")
    assert not xl.grad[:, c:].any()
    first = xl.grad.clone()
    xl.grad = None
    again = ops.map_mean(xl, c)
    again.backward(g.to(DEV))
    assert torch.equal(again, out) and torch.equal(first, xl.grad), "a repeat must be bit-identical"


# ----------------------------------------------------------------------------- 4. the gradient kernels read the MASK map
@pytest.mark.parametrize("hw", R.SIZES)
@pytest.mark.parametrize("slope", [0.25, 0.5])
def test_leaky_dgrad_and_wgrad_read_the_mask_map_not_the_sign_of_dy(hw, slope):
    """raw entry points with a mask map unrelated to the output (as test_kxk_mfma_output_mask_epilogue does for the ReLU form):
    dy_eff = m > 0 ? dy : slope * dy with m drawn on its own"""
    H, W = hw
    K, cin, cout, cip, cop = 5, 64, 32, 64, 32
    hip, L = sisr_amd.hip, sisr_amd.hip.lib()
    x, w = E.ints((R.B, cin, H, W), 61), E.weights((cout, cin, K, K), 62)
    dy, m = E.ints((R.B, cout, H, W), 63), E.ints((R.B, cout, H, W), 64, -1, 1)
    eff = (dy.double() * E.leaky_mask(m, slope)).to(DEV)
    assert torch.equal(eff, torch.where(m > 0, dy.double(), slope * dy.double()).to(DEV))
    assert ((dy > 0) & (m <= 0)).any() and ((dy < 0) & (m > 0)).any(), "test bug: sign of dy and mask never disagree"
    E.conv_budget(eff, w.transpose(0, 1).to(DEV), padding=K // 2, what="leaky dgrad")
    _wgrad_budget(x, dy, slope, K)
    xm, dym, mm = R.to_map(x, cip, DEV), R.to_map(dy, cop, DEV), R.to_map(m, cop, DEV)
    _, pd = ops.pack_convk(w.to(DEV), need_dgrad=True)
    dx = torch.full((R.B, cip, H, W), float("nan"), device=DEV).contiguous(memory_format=CL)
    ops.convk_mfma_leaky(dym, pd, None, 0, dx, R.B, H, W, K, cop, cip, slope, in_mask=mm)
    E.assert_exact(dx, E.dgrad_ref(eff, w.to(DEV)), "leaky dgrad through a foreign mask")
    dw, db = torch.full_like(w, float("nan")).to(DEV), torch.full((cout,), float("nan"), device=DEV)
    nb = L.sisr_wgradk_mfma_workspace_bytes(R.B, H, W, K, cip, cop)
    ws = hip.workspace(torch.device(DEV), nb)
    hip.check(L.sisr_wgradk_mfma_leaky(hip.ptr(xm), hip.ptr(dym), hip.ptr(mm), hip.ptr(dw), hip.ptr(db), R.B, H, W, K, cout, cin,
                                       cop, cip, hip.ptr(ws), nb, slope, hip.stream()), "sisr_wgradk_mfma_leaky")
    E.assert_exact(dw, E.wgrad_ref(x.to(DEV), eff, padding=K // 2, k=K), "leaky wgrad through a foreign mask")
    E.assert_exact(db, eff.sum(dim=(0, 2, 3)), "leaky bias gradient through a foreign mask")


# ----------------------------------------------------------------------------- 5. the network against its float64 twin
@pytest.mark.parametrize("shape", [(2, 3, 9, 21), (2, 3, 37, 70)])
@pytest.mark.parametrize("M", [1, 12, 33])
@pytest.mark.parametrize("num_features", [64, 48])
@pytest.mark.parametrize("num_layers", [2, 6])
def test_predictor_output_and_gradients_against_the_float64_twin(shape, M, num_features, num_layers):
    """relative L2 distance of the output and of every parameter gradient from float64 < 5e-5, the per-gradient bound of
    test_basic_gpu.py::test_b1_output_and_gradients.  The reference is the float64 twin; where one of its pre-activations is
    closer to 0 than fp32 resolves (|z| < KINK = 4e-6, at most two elements of a case) its LeakyReLU derivative is the branch
    the fp32 forward took, because there the gradient is not a function of the fp32 inputs (tests/_predictor.py).  The largest
    distances measured on an MI355X, and those of the stock fp32 twin on the same GPU (tools/predictor_bench.py), are
    recorded in DESIGN.md 6w."""
    cfg = dict(num_outputs=M, num_features=num_features, num_layers=num_layers)
    net = sisr_amd.predictor.DegradationPredictor(**cfg)
    sd = P.kaiming_state(net, 70 + M + num_features + num_layers)
    assert list(sd) == list(P.Twin(**cfg).state_dict()) and all(k.startswith("layer_dict.conv_") for k in sd)
    net.load_state_dict(sd, strict=True)
    net.to(DEV)
    g = torch.Generator().manual_seed(71)
    x, cot = torch.rand(shape, generator=g), torch.randn((shape[0], M), generator=g)
    out = net(x.to(DEV))
    assert out.shape == (shape[0], M)
    out.backward(cot.to(DEV))
    with torch.no_grad():  # the branch every LeakyReLU of the HIP forward took: the same launches again, layer by layer
        t, branches = ops.nchw_to_nhwc_pad(x.to(DEV), cp=32), []
        for i in range(num_layers):
            m = net.layer_dict["conv_%d" % i]
            t = ops.conv_kxk(t, m.weight, m.bias, slope=net.slope)
            branches.append(t[:, :m.out_channels].cpu() > 0)
        assert torch.equal(ops.map_mean(t, M), out.detach())
    ref = P.twin64(sd, **cfg)  # on the host: float64 there is the reference whatever the device libraries do
    want, decided = P.twin_forward(ref, x, branches)  # (its own branches outside |z| < KINK: tests/_predictor.py)
    assert decided <= 2
    want.backward(cot.double())
    assert 0.005 < float(want.detach().abs().mean()) < 10, "test bug: degenerate outputs"
    worst = P.rel_l2(out, want)
    assert worst < 5e-5, ("output", worst)
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        err = P.rel_l2(p.grad, q.grad)
        worst = max(worst, err)
        assert err < 5e-5, (k, err)
    print("predictor parity", shape, cfg, "largest relative L2 distance from float64: %.3g" % worst, "at-the-kink:", decided)


# ----------------------------------------------------------------------------- 6. - 8. the handler
def _handler(eval_mode=False, **extra):
    torch.manual_seed(8)
    kw = dict(metadata=list(P.KEYS), lr=1e-4)
    kw.update(extra)
    return sisr_amd.available_models["predictor"](device=0, model_save_dir="/tmp", eval_mode=eval_mode, **kw)


def test_run_train_trajectory_matches_the_float64_twin_with_adam():
    """three run_train steps against torch.optim.Adam on the float64 twin from the same weights: loss within 5e-6, gradient
    norm within 1e-4 relative (the bounds of test_b3_run_train_trajectory_matches_reference).  The targets come from a
    metadata batch with a 'qpi' column the handler does not list; the HR batch is ignored."""
    h = _handler()
    sd = P.kaiming_state(h.net, 81)
    h.net.load_state_dict(sd)
    ref = P.twin64(sd, num_outputs=12)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(82)
    for step in range(3):
        x = torch.rand(2, 3, 24, 40, generator=g)
        md, keys, target = P.metadata_batch(2, 83 + step)
        loss, out = h.run_train(x, torch.full((2, 3, 96, 160), float("nan")), metadata=md, metadata_keys=keys,
                                tag=["a", "b"])
        gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in h.net.parameters())))
        opt.zero_grad()
        want = ref(x.double())
        wl = F.mse_loss(want, target.double())
        wl.backward()
        wn = float(torch.sqrt(sum((p.grad ** 2).sum() for p in ref.parameters())))
        print("step", step, float(loss), float(wl), gn, wn)
        assert out.shape == (2, 12) and not out.is_cuda
        assert abs(float(loss) - float(wl)) < 5e-6 and abs(gn / wn - 1) < 1e-4, (step, float(loss), float(wl), gn, wn)
        opt.step()
    for (k, p), q in zip(h.net.named_parameters(), ref.parameters()):
        assert P.rel_l2(p, q) < 1e-5, k  # three Adam steps of lr 1e-4 on weights of O(0.05): both moved the same way


def test_step_under_graph_capture_equals_eager():
    """forward + MSE + backward replayed from a hipGraph (map_mean and the leaky convs capture: no host synchronisation,
    workspaces from hip.workspace) gives the eager trajectory; tolerances of test_vdsr_step_under_graph_capture_equals_eager"""
    runs = {}
    for mode in (False, True):
        h = _handler(num_layers=4)
        h.use_graph = mode
        g = torch.Generator().manual_seed(5)
        ls = []
        for _ in range(3):
            x, y = torch.rand(2, 3, 24, 40, generator=g), torch.rand(2, 12, generator=g)
            loss, out = h.train_step(x, y)
            ls.append((float(loss), float(out.double().sum())))
        runs[mode] = (ls, [p.detach().clone() for p in h.net.parameters()])
    for (la, oa), (lb, ob) in zip(runs[False][0], runs[True][0]):
        assert abs(la - lb) <= 1e-7 * abs(la) and abs(oa - ob) <= 1e-6 * abs(oa)
    for pa, pb in zip(runs[False][1], runs[True][1]):
        torch.testing.assert_close(pa, pb, rtol=1e-5, atol=1e-7)


def test_checkpoint_round_trip_through_the_model_interface(tmp_path):
    params = {"name": "predictor", "internal_params": {"scale": 4, "lr": 1e-3, "metadata": list(P.KEYS), "num_layers": 3,
                                                       "num_features": 48, "kernel_size": 3, "ema_decay": 0.5}}
    torch.manual_seed(8)
    mi = sisr_amd.ModelInterface(str(tmp_path), "p", gpu="single", sp_gpu=0, mode="train", new_params=params)
    g = torch.Generator().manual_seed(91)
    for _ in range(2):
        md, keys, _ = P.metadata_batch(2, 92)
        mi.train_batch(lr=torch.rand(2, 3, 16, 20, generator=g), hr=None, metadata=md, metadata_keys=keys)
    mi.save()
    sisr_amd.cli._dump_toml({"model": params}, os.path.join(mi.base_folder, "config.toml"))
    x = torch.rand(2, 3, 19, 23, generator=g)
    want, none, _ = mi.model.run_eval(x)
    with mi.model.averaged_weights():
        want_ema, _, _ = mi.model.run_eval(x)
    assert none is None and want.shape == (2, 12) and not torch.equal(want, want_ema)
    back = sisr_amd.ModelInterface(str(tmp_path), "p", gpu="single", sp_gpu=0, mode="eval", load_epoch=0)
    assert back.configuration == {"input": "unmodified", "colorspace": "rgb"}
    assert torch.equal(back.model.run_eval(x)[0], want)
    ema = sisr_amd.ModelInterface(str(tmp_path), "p", gpu="single", sp_gpu=0, mode="eval", load_epoch=0, ema=True)
    assert torch.equal(ema.model.run_eval(x)[0], want_ema)
    md, keys, target = P.metadata_batch(2, 93)
    codes, loss, _ = back.model.run_eval(x, metadata=md, metadata_keys=keys, request_loss=True, keep_on_device=True)
    assert codes.is_cuda and abs(float(loss) - float(F.mse_loss(codes.cpu().double(), target.double()))) < 1e-6


# ----------------------------------------------------------------------------- 9. train_sisr
def _small_pca(monkeypatch):
    real = sisr_amd.degrade.pca_matrix
    monkeypatch.setattr(sisr_amd.degrade, "pca_matrix", lambda batch=2000, k=10: real(batch=2000, k=k))


@pytest.mark.parametrize("degrade_tiles", [False, True])
def test_train_sisr_trains_the_predictor_from_online_degradations(tmp_path, monkeypatch, degrade_tiles):
    """the Set5 HR images with blur + noise + JPEG drawn online, three batches of 32 x 32 LR crops per epoch, a reduced net;
    validation records val-loss and val-MAE and no image metric although the config lists PSNR.  Two epochs, so that 'best'
    has something to choose from."""
    import pandas as pd
    _small_pca(monkeypatch)
    extra = {"device_tiles": True, "degrade_tiles": True} if degrade_tiles else {}
    cfg = P.train_config(tmp_path, **extra)
    total = sisr_amd.cli.train_sisr(cfg)
    summary = pd.read_csv(os.path.join(str(tmp_path), "pred", "result_outputs", "summary.csv"))
    assert {"train-loss", "val-loss", "val-MAE", "learning-rate", "epoch"} == set(summary.columns)
    assert "val-PSNR" not in total and len(total["val-loss"]) == 2
    assert np.isfinite(summary.values).all() and (summary["val-MAE"] > 0).all()
    best = sisr_amd.ModelInterface(str(tmp_path), "pred", gpu="single", sp_gpu=0, mode="eval", load_epoch="best")
    assert best.model_epoch == int(np.argmin(total["val-loss"]))
    assert os.path.isfile(os.path.join(str(tmp_path), "pred", "saved_models", "train_model_1"))


# ----------------------------------------------------------------------------- 10. eval_sisr
def _eval_fixture(tmp_path, q_metadata=None):
    q = {"name": "qrcan", "internal_params": {"scale": 4, "style": "standard", "include_q_layer": True, "n_resgroups": 2,
                                              "n_resblocks": 2, "metadata": list(q_metadata or P.KEYS)}}
    p = {"name": "predictor", "internal_params": {"scale": 4, "metadata": list(P.KEYS), "num_layers": 3, "num_features": 32}}
    P.save_experiment(sisr_amd, tmp_path, "q", q, gpu=True)
    mi = P.save_experiment(sisr_amd, tmp_path, "p", p, gpu=True)
    return mi


@pytest.mark.parametrize("device_outputs", [False, True])
def test_eval_sisr_feeds_the_predicted_codes_to_the_q_model_unaltered(tmp_path, device_outputs):
    """no metadata file: every image gets a row.  Then the same evaluation from a degradation_metadata.csv holding the
    predicted values (repr precision) and no predictor: the PSNR column is bit-identical, so the codes reached the network
    as predicted."""
    import pandas as pd
    _eval_fixture(tmp_path)
    lr_dir = P.lr_folder_without_metadata(tmp_path)
    common = dict(model_and_epoch=[["q", "0"]], model_loc=str(tmp_path), gpu=True, hr_dir=os.path.join(GOLDEN, "set5", "hr"),
                  lr_dir=lr_dir, full_directory=True, scale=4, out_loc=str(tmp_path), time_models=False,
                  device_outputs=device_outputs or None)
    df, _ = sisr_amd.cli.eval_sisr(results_name="ev_pred", metadata_predictor=["p", 0], **common)
    names = sorted(f for f in os.listdir(lr_dir) if f.endswith(".png"))
    assert sorted(df["Image_Name"]) == names and np.isfinite(df["PSNR"]).all()
    codes = pd.read_csv(os.path.join(str(tmp_path), "ev_pred", "standard_metrics", "predicted_metadata.csv"))
    cols = ["blur_kernel_%d" % i for i in range(10)] + ["noise", "jpeg_quality"]
    assert list(codes.columns) == ["Image_Name"] + cols and sorted(codes["Image_Name"]) == names
    vals = codes.set_index("Image_Name")
    meta = pd.DataFrame({"blur_kernel": [json.dumps([float(vals.loc[n, c]) for c in cols[:10]]) for n in names],
                         "noise": [json.dumps([float(vals.loc[n, "noise"])]) for n in names],
                         "jpeg_quality": [json.dumps([float(vals.loc[n, "jpeg_quality"])]) for n in names]}, index=names)
    meta_file = os.path.join(str(tmp_path), "from_codes.csv")
    meta.to_csv(meta_file)
    again, _ = sisr_amd.cli.eval_sisr(results_name="ev_file", metadata_file=meta_file, **common)
    assert list(again["Image_Name"]) == list(df["Image_Name"])
    assert list(again["PSNR"]) == list(df["PSNR"])
    assert not os.path.exists(os.path.join(str(tmp_path), "ev_file", "standard_metrics", "predicted_metadata.csv"))
    # next to a metadata file the predictor still supplies the codes, and reports its distance from the file's
    both, _ = sisr_amd.cli.eval_sisr(results_name="ev_both", metadata_predictor=["p", 0], metadata_file=meta_file, **common)
    assert list(both["PSNR"]) == list(df["PSNR"])
    mae = pd.read_csv(os.path.join(str(tmp_path), "ev_both", "standard_metrics", "predicted_metadata.csv"))["code_MAE"]
    assert (mae == 0).all()


def test_eval_sisr_with_self_ensemble_gives_the_code_to_all_eight_variants(tmp_path):
    _eval_fixture(tmp_path)
    lr_dir = P.lr_folder_without_metadata(tmp_path)
    df, _ = sisr_amd.cli.eval_sisr(results_name="ev", metadata_predictor=["p", 0], model_and_epoch=[["q", "0"]],
                                   model_loc=str(tmp_path), gpu=True, hr_dir=os.path.join(GOLDEN, "set5", "hr"), lr_dir=lr_dir,
                                   full_directory=True, scale=4, out_loc=str(tmp_path), time_models=False, self_ensemble=True)
    assert set(df["Model"]) == {"q+"} and len(df) == 5 and np.isfinite(df["PSNR"]).all()


def test_eval_sisr_refuses_a_different_metadata_list(tmp_path):
    _eval_fixture(tmp_path, q_metadata=["blur_kernel", "jpeg_quality", "noise"])
    with pytest.raises(ValueError) as err:
        sisr_amd.cli.eval_sisr(results_name="ev", metadata_predictor=["p", 0], model_and_epoch=[["q", "0"]],
                               model_loc=str(tmp_path), gpu=True, hr_dir=os.path.join(GOLDEN, "set5", "hr"),
                               lr_dir=P.lr_folder_without_metadata(tmp_path), full_directory=True, scale=4,
                               out_loc=str(tmp_path))
    assert "['blur_kernel', 'jpeg_quality', 'noise']" in str(err.value) and str(P.KEYS) in str(err.value)
