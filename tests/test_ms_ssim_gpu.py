"""Multi-scale SSIM on the GPU: ops.ms_ssim_mean and metrics.batch_ms_ssim against the float64 oracle with the stock torch
fp32 composition as the yardstick, the criterion, the handlers' training steps and the train / eval entry points."""
import copy
import os

import numpy as np
import pytest
import torch

import sisr_amd
from sisr_amd import architectures as A
from sisr_amd import basic, handlers, metrics, multiscale, ops

import _basic as B
import _ms_ssim as MS
import _ssim_loss as S
from conftest import GOLDEN, golden_json

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _hip(sr, y, weights, scale=1.0, data_range=1.0):
    """(value, d (scale * value) / d sr) from ops.ms_ssim_mean"""
    sr = sr.to(DEV).requires_grad_(True)
    v = ops.ms_ssim_mean(sr, y.to(DEV), data_range, weights)
    (scale * v).backward()
    return v.detach(), sr.grad


def _per_plane(sr, y, weights):
    """the float64 per-plane values of sisr_ms_ssim, every plane as given (batch_ms_ssim takes C = 1 planes so)"""
    h, w = sr.shape[2:]
    return torch.tensor(metrics.batch_ms_ssim(sr.reshape(-1, 1, h, w).to(DEV), y.reshape(-1, 1, h, w).to(DEV), weights=weights),
                        dtype=torch.float64).reshape(sr.shape[:2])


@pytest.fixture(scope="module")
def runs():
    """per case, computed once and never modified: the inputs and weights, (per-plane values, value, gradient) of the float64
    oracle on the host and of the stock torch fp32 composition on the device, (value, gradient) of the HIP operator"""
    out = {}
    for cid, case in zip(MS.CASE_IDS, MS.CASES):
        sr, y, weights = MS.make_case(case)
        ref = MS.autograd_grad(sr.double(), y.double(), weights)
        stock = MS.autograd_grad(sr.to(DEV), y.to(DEV), weights)
        out[cid] = (sr, y, weights, ref, stock, _hip(sr, y, weights))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cid", MS.CASE_IDS)
def test_value_is_the_float64_mean_rounded_to_fp32(runs, cid):
    """|v_hip - v_64| <= 2^-24: the value is a float64 quantity in [0.5, 1) (asserted on the oracle) rounded to fp32 once, so
    half a unit, 2^-25, is the rounding; the factor two leaves room for float64 summation order.  The per-plane float64
    output against the oracle's per-plane values: 1e-12.
    Measured on an MI355X, |v_hip - v_64| (the stock fp32 composition's in brackets), max per-plane difference:
      2 x 1 x 22 x 23, 2 scales, s 0.05: 1.82e-08 (1.97e-07), 1.1e-15    1 x 3 x 44 x 87, 3 scales, s 0.05: 1.92e-09 (5.77e-08), 1.3e-15
      1 x 1 x 176 x 176, 5 scales, s 0.05: 8.76e-09 (4.68e-07), 1.0e-15  2 x 3 x 183 x 201, 5 scales, s 0.05: 8.01e-09 (5.88e-07), 9.1e-15
      2 x 3 x 183 x 201, 5 scales, s 0.002: 2.88e-08 (1.48e-07), 1.0e-14
    all below the rounding alone, 2^-25 = 2.98e-08: the HIP value is the fp32 number nearest the float64 mean in every case."""
    sr, y, weights, (p64, v64, _), (_, v32, _), (vh, _) = runs[cid]
    assert 0.5 <= float(v64) < 1.0, float(v64)
    assert vh.dtype == torch.float32 and vh.shape == ()
    d = abs(float(vh.double().cpu()) - float(v64))
    dp = float((_per_plane(sr, y, weights) - p64).abs().max())
    print(f"value {cid}: oracle {float(v64):.9f} |hip - f64| {d:.3e} (stock fp32 {abs(float(v32.double().cpu()) - float(v64)):.3e}) "
          f"per plane {dp:.3e}")
    assert d <= 2.0 ** -24, d
    assert dp <= 1e-12, dp


@pytest.mark.parametrize("cid", MS.CASE_IDS)
def test_gradient_is_no_further_from_float64_than_stock_fp32(runs, cid):
    """relative L2 of d value / d sr against float64 autograd of the oracle, no element excluded.  Bound: the error of the stock
    torch fp32 composition (grouped conv2d + avg_pool2d + autograd, same device, same inputs) against the same float64 values,
    taken in this run, margin factor 1: the kernels hold everything in float64, so anything above the yardstick is a defect.
    Measured on an MI355X (relative L2 against float64: HIP / stock torch fp32):
      2 x 1 x 22 x 23, 2 scales, s 0.05: 2.27e-08 / 3.77e-06      1 x 3 x 44 x 87, 3 scales, s 0.05: 2.54e-08 / 7.27e-06
      1 x 1 x 176 x 176, 5 scales, s 0.05: 2.56e-08 / 1.43e-05    2 x 3 x 183 x 201, 5 scales, s 0.05: 2.54e-08 / 2.88e-05
      2 x 3 x 183 x 201, 5 scales, s 0.002: 2.52e-08 / 3.91e-04
    The HIP figure is the one rounding of each element to fp32 and does not grow with the scales or near convergence."""
    sr, y, weights, (_, _, g64), (_, _, g32), (_, gh) = runs[cid]
    assert gh.shape == sr.shape and gh.is_contiguous() and gh.dtype == torch.float32
    e, s = S.rel_l2(gh, g64), S.rel_l2(g32, g64)
    print(f"gradient {cid}: hip {e:.3e} stock {s:.3e}")
    assert bool(torch.isfinite(gh).all())
    assert e <= s, (e, s)


def test_upstream_gradient_scales_the_result(runs):
    """(3 * ms_ssim_mean).backward() is the unit gradient times 3, bit for bit"""
    sr, y, weights, _, _, (_, g1) = runs[MS.CASE_IDS[1]]
    _, gh = _hip(sr, y, weights, scale=3.0)
    assert torch.equal(gh, g1 * 3.0)


@pytest.mark.parametrize("case", MS.CASES[:4], ids=MS.CASE_IDS[:4])
def test_equal_images_give_exactly_one(case):
    _, y, weights = MS.make_case(case)
    v, g = _hip(y.clone(), y, weights)
    assert float(v) == 1.0
    assert bool((_per_plane(y, y, weights) == 1.0).all())
    # the maximum of every c_j: the terms of each scale's gradient, O(1 / B2) <= 1 / C2 ~ 1e3 each, cancel in float64
    assert float(g.abs().max()) <= 1e-9


def test_a_repeat_call_is_bit_identical(runs):
    for cid in MS.CASE_IDS[-2:]:
        sr, y, weights, _, _, (v1, g1) = runs[cid]
        ops.l1_loss(torch.rand(1 << 18, device=DEV), torch.rand(1 << 18, device=DEV))  # something else uses the workspace
        v2, g2 = _hip(sr, y, weights)
        assert torch.equal(v1, v2) and torch.equal(g1, g2)


def test_value_without_a_gradient_is_the_same_value(runs):
    sr, y, weights, _, _, (v1, _) = runs[MS.CASE_IDS[-1]]
    with torch.no_grad():
        v = ops.ms_ssim_mean(sr.to(DEV), y.to(DEV), weights=weights)
    assert not v.requires_grad and torch.equal(v, v1)
    # a non-contiguous operand is compared as the batch it shows
    wide = torch.zeros(sr.shape[:3] + (sr.shape[3] + 3,), device=DEV)
    wide[..., :sr.shape[3]] = sr.to(DEV)
    assert torch.equal(ops.ms_ssim_mean(wide[..., :sr.shape[3]], y.to(DEV), weights=weights), v1)


def test_target_takes_no_gradient():
    x = torch.rand(1, 1, 22, 22, device=DEV)
    with pytest.raises(RuntimeError, match="target takes no gradient"):
        ops.ms_ssim_mean(x, x.clone().requires_grad_(True), weights=(0.5, 0.5))


def test_an_anticorrelated_plane_is_zero_and_leaves_the_others_alone():
    """plane 0 of a 1 x 3 x 44 x 87 batch is 1 - y: its scale means are negative, so its value is exactly 0 and its gradient
    exactly 0, with everything finite (torch autograd gives NaN there: 0 * inf).  The other planes' gradients are those of
    the batch without plane 0 times 2 / 3, the plane-count ratio: both are one fp32 rounding (2^-24 relative each) of float64
    quantities that agree to float64 rounding, so 2^-23 bounds every element's relative difference and the relative L2.
    Measured on an MI355X: 3.58e-08."""
    sr, y, weights = MS.make_case(MS.CASES[1])
    sr = sr.clone()
    sr[:, 0] = 1 - y[:, 0]
    assert any(float(c[0, 0]) < 0 for c in MS.scale_means(sr.double(), y.double(), len(weights)))
    v, g = _hip(sr, y, weights)
    per = _per_plane(sr, y, weights)
    assert float(per[0, 0]) == 0.0 and bool((per[0, 1:] > 0.5).all())
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(v))
    assert bool((g[:, 0] == 0).all())
    assert abs(float(v.double().cpu()) - float(per.mean())) <= 2.0 ** -24
    _, g2 = _hip(sr[:, 1:], y[:, 1:], weights)
    e = S.rel_l2(g[:, 1:], g2.double() * (2.0 / 3.0))
    print(f"other planes against the batch without plane 0: rel L2 {e:.3e}")
    assert e <= 2.0 ** -23, e


def test_a_scale_mean_at_or_below_zero_zeroes_the_plane_whatever_its_weight():
    """plane 0 of a 1 x 2 x 22 x 22 batch is MS.checker_pair (c_0 < 0, c_1 = 1), plane 1 an ordinary pair; weights (0, 1).
    The bare product max(c_0, 0)^0 * c_1 would make plane 0's value 1; the kernel looks at the means, not at the weights, as
    metrics.ms_ssim does: plane 0 is exactly 0 with an exactly zero gradient, plane 1 is the host form (1e-12) and its
    gradient is alive, and everything is finite."""
    cs, cy = MS.checker_pair()
    ns, ny = S.make_pair((1, 1, 22, 22), 0.05)
    sr, y = torch.cat([cs, ns], 1), torch.cat([cy, ny], 1)
    c0, c1 = MS.scale_means(sr.double(), y.double(), 2)
    assert float(c0[0, 0]) < 0 and abs(float(c1[0, 0]) - 1) <= 1e-6 and float(c0[0, 1]) > 0
    weights = (0.0, 1.0)
    v, g = _hip(sr, y, weights)
    per = _per_plane(sr, y, weights)
    host = metrics.ms_ssim(sr[0, 1].numpy(), y[0, 1].numpy(), weights=weights)
    print(f"zero weight on a negative scale: per plane {per.tolist()} host plane 1 {host!r} value {float(v)!r}")
    assert float(per[0, 0]) == 0.0 == metrics.ms_ssim(sr[0, 0].numpy(), y[0, 0].numpy(), weights=weights)
    assert abs(float(per[0, 1]) - host) <= 1e-12 and 0 < host < 1
    assert bool(torch.isfinite(g).all()) and abs(float(v.double().cpu()) - host / 2) <= 2.0 ** -24
    assert bool((g[:, 0] == 0).all()) and float(g[:, 1].abs().max()) > 0


def test_one_weight_of_one_is_the_single_scale_operator():
    """weights (1.0,): the value agrees with ops.ssim_mean within 2^-24 and the gradient within 2^-23 relative L2 -- both
    sides are one fp32 rounding of float64 quantities that differ only in summation order (per plane here, over all tiles
    there).  Measured on an MI355X: both differences are exactly 0 at 1 x 3 x 43 x 75."""
    sr, y = S.make_pair((1, 3, 43, 75), 0.05)
    v, g = _hip(sr, y, (1.0,))
    xs = sr.to(DEV).requires_grad_(True)
    v1 = ops.ssim_mean(xs, y.to(DEV))
    v1.backward()
    d, e = abs(float(v.double().cpu()) - float(v1.detach().double().cpu())), S.rel_l2(g, xs.grad)
    print(f"weights (1.0,) against ssim_mean: value {d:.3e} gradient {e:.3e}")
    assert d <= 2.0 ** -24, d
    assert e <= 2.0 ** -23, e


@pytest.mark.parametrize("channels", [1, 3])
def test_batch_metric_is_the_host_form(channels):
    """metrics.batch_ms_ssim on device tensors against metrics.ms_ssim per image: 1e-12, the bound tests/test_ssim_gpu.py
    holds SSIM to.  C = 3 goes through the Y of the clipped image (values outside [0, 1] are in the batch), C = 1 is taken as
    given."""
    g = np.random.default_rng(17 + channels)
    shape = (2, channels, 183, 201)
    hr = g.random(shape, dtype=np.float32)
    sr = hr + np.float32(0.1) * g.standard_normal(shape, dtype=np.float32)
    assert sr.min() < 0 and sr.max() > 1
    dev = metrics.batch_ms_ssim(torch.from_numpy(sr).to(DEV), torch.from_numpy(hr))  # the host batch follows the device one
    if channels == 3:
        ys, yh = metrics.batch_rgb_to_ycbcr(sr)[:, 0], metrics.batch_rgb_to_ycbcr(hr)[:, 0]
    else:
        ys, yh = sr[:, 0], hr[:, 0]
    host = [metrics.ms_ssim(ys[i], yh[i]) for i in range(shape[0])]
    print(f"batch_ms_ssim C = {channels}: device {dev} host {host}")
    np.testing.assert_allclose(dev, host, rtol=0, atol=1e-12)
    assert metrics.batch_ms_ssim(sr, hr) == host
    assert all(0 < v < 1 for v in host)
    four = metrics.batch_ms_ssim(torch.from_numpy(sr).to(DEV), torch.from_numpy(hr).to(DEV), weights=MS.WEIGHTS[:4])
    np.testing.assert_allclose(four, [metrics.ms_ssim(ys[i], yh[i], weights=MS.WEIGHTS[:4]) for i in range(shape[0])],
                               rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="at least 176"):
        metrics.batch_ms_ssim(torch.zeros(1, channels, 175, 200, device=DEV), torch.zeros(1, channels, 175, 200, device=DEV))


# ----------------------------------------------------------------------------- criterion
def test_criterion_matches_float64_within_four_times_stock_fp32():
    """MultiScaleStructuralMechanism(L1Loss(), 0.2) on inputs with |sr - y| >= 0.01 (the L1 kink rule): loss and
    d loss / d sr against the float64 restatement, relative error no larger than 4 x that of the stock torch fp32 composition on
    the same device -- the L1 mean's fp32 rounding is shared with the yardstick, and 4 is what the structural criterion's
    test allows for the same reason.
    Measured on an MI355X (HIP / stock torch fp32): loss 6.39e-08 / 7.15e-07, d loss / d sr 2.87e-08 / 1.61e-05."""
    shape = (1, 3, 176, 177)
    sr, y = S.kink_free_pair(shape)
    assert float((sr - y).abs().min()) >= 0.01
    crit = multiscale.MultiScaleStructuralMechanism(handlers.L1Loss(), 0.2)

    def run(fn, sr, y):
        sr = sr.clone().requires_grad_(True)
        loss = fn(sr, y)
        (g,) = torch.autograd.grad(loss, sr)
        return loss.detach(), g

    l64, g64 = run(lambda a, b: MS.criterion(a, b, "l1", 0.2), sr.double(), y.double())
    l32, g32 = run(lambda a, b: MS.criterion(a, b, "l1", 0.2), sr.to(DEV), y.to(DEV))
    lh, gh = run(crit, sr.to(DEV), y.to(DEV))
    assert gh.shape == sr.shape and gh.is_contiguous()
    e_l, e_g = S.rel_l2(lh, l64), S.rel_l2(gh, g64)
    s_l, s_g = S.rel_l2(l32, l64), S.rel_l2(g32, g64)
    print(f"criterion: loss hip {e_l:.3e} stock {s_l:.3e}; gradient hip {e_g:.3e} stock {s_g:.3e}")
    assert float(l64) > float((sr.double() - y.double()).abs().mean())  # the multi-scale term is in it
    assert e_g <= 4 * s_g, (e_g, s_g)
    assert e_l <= 4 * s_l, (e_l, s_l)


# ----------------------------------------------------------------------------- handlers
class _SmallRCANHandler(handlers.BaseModel):
    """RCANHandler around a reduced RCAN: one group, one block, 64 features, x4 (as in test_ssim_loss_gpu.py)"""

    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, perceptual=None, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        self.net = A.RCAN(n_resblocks=1, n_resgroups=1, n_feats=64, scale=4)
        self.colorspace = 'rgb'
        self.im_input = 'unmodified'
        self.activate_device()
        self.training_setup(lr, None, None, perceptual, device)
        self.model_name = 'rcan'


def _float64_criterion(out, y, base, alpha, weights=MS.WEIGHTS):
    return float(MS.criterion(out.detach().double().cpu(), y.detach().double().cpu(), base, alpha, weights))


def test_handler_trains_with_the_multiscale_loss_eager_and_graphed(tmp_path):
    """three train_steps at B = 2, 44 x 44 LR -> 176 x 176, ms_ssim_loss = 0.2, eager and replayed from a hipGraph: the same
    loss trajectory and final parameters (1e-6 absolute per loss, 1e-5 on the parameter sum); the first loss is the float64
    criterion of the returned output within 1e-5 relative and exceeds its L1 term."""
    runs = {}
    for mode in (False, True):
        torch.manual_seed(8)
        h = _SmallRCANHandler(device=0, model_save_dir=str(tmp_path), ms_ssim_loss=0.2)
        h.use_graph = mode
        assert isinstance(h.criterion, multiscale.MultiScaleStructuralMechanism) and type(h.criterion.base) is handlers.L1Loss
        g = torch.Generator().manual_seed(5)
        ls, first = [], None
        for step in range(3):
            x, y = torch.rand(2, 3, 44, 44, generator=g), torch.rand(2, 3, 176, 176, generator=g)
            loss, out = h.train_step(x, y)
            if step == 0:
                first = (float(loss), _float64_criterion(out, y, "l1", 0.2), float((out.double().cpu() - y.double()).abs().mean()))
            ls.append(float(loss))
        torch.cuda.synchronize()
        print(f"rcan graph={mode}: losses {ls} first {first}")
        assert abs(first[0] - first[1]) <= 1e-5 * abs(first[1]), first
        assert first[0] > first[2], first  # above its L1 term
        runs[mode] = (ls, float(sum(p.double().sum() for p in h.net.parameters())))
    assert np.allclose(runs[True][0], runs[False][0], rtol=0, atol=1e-6), runs
    assert abs(runs[True][1] - runs[False][1]) < 1e-5


def test_y_channel_handler_trains_on_mse_plus_the_multiscale_term(tmp_path):
    """VDSRHandler (reduced: four 3 x 3 layers), one step at B = 2, 1 x 96 x 96 with four weights: the loss is the float64
    MSE + alpha (1 - MS-SSIM) of the returned output within 1e-5 relative, above its MSE term, and the parameters move."""
    torch.manual_seed(8)
    h = basic.VDSRHandler(device=0, model_save_dir=str(tmp_path), kernel_pattern=[3] * 4, channel_pattern=[1, 64, 64, 64, 1],
                          ms_ssim_loss=0.2, ms_ssim_weights=list(MS.WEIGHTS[:4]))
    assert isinstance(h.criterion, multiscale.MultiScaleStructuralMechanism) and type(h.criterion.base) is basic.MSELoss
    start = float(sum(p.double().abs().sum() for p in h.net.parameters()))
    g = torch.Generator().manual_seed(6)
    y = torch.rand(2, 1, 96, 96, generator=g)
    x = (y + 0.05 * torch.randn(2, 1, 96, 96, generator=g)).clamp(0, 1)
    loss, out = h.train_step(x, y)
    ref = _float64_criterion(out, y, "mse", 0.2, MS.WEIGHTS[:4])
    mse = float(((out.double().cpu() - y.double()) ** 2).mean())
    print(f"vdsr: loss {float(loss):.8f} float64 {ref:.8f} mse term {mse:.8f}")
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (float(loss), ref)
    assert float(loss) > mse
    assert float(sum(p.double().abs().sum() for p in h.net.parameters())) != start


# ----------------------------------------------------------------------------- entry points
def _config(name, tmp_path):
    cfg = copy.deepcopy(golden_json("g5_train_sisr")[name]["config"])
    cfg["experiment_save_loc"] = str(tmp_path)
    for part in ("training_sets", "eval_sets"):
        for d in cfg["data"][part].values():
            d["lr"] = d["lr"].replace("SET5", os.path.join(GOLDEN, "set5"))
            d["hr"] = d["hr"].replace("SET5", os.path.join(GOLDEN, "set5"))
    return cfg


def test_train_and_eval_entry_points_measure_ms_ssim_on_hip(tmp_path, monkeypatch):
    """train_sisr and eval_sisr on Set5 (every image at least 176 on a side) with metrics PSNR, SSIM, MS-SSIM: the new columns
    exist and hold the host form of the outputs the host sees, within 1e-9 (the bound the SSIM columns are held to)"""
    M = sisr_amd.metrics
    cfg = _config("edsr", tmp_path)
    cfg["training"].update(gpu="single", sp_gpu=0, metrics=["PSNR", "SSIM", "MS-SSIM"])
    seen = []  # the validation outputs (Y of the clipped output, as the host sees them), HR and what the device measured
    real = sisr_amd.handlers.ModelInterface.net_run_process_and_measure

    def spy(self, lr=None, hr=None, **kw):
        res = real(self, lr=lr, hr=hr, **kw)
        seen.append((res[1], M.batch_rgb_to_ycbcr(hr.numpy()), kw["max_value"], res[4]))
        return res
    monkeypatch.setattr(sisr_amd.handlers.ModelInterface, "net_run_process_and_measure", spy)
    total = sisr_amd.cli.train_sisr(cfg)
    assert {"val-PSNR", "val-SSIM", "val-MS-SSIM"} <= set(total)
    assert len(seen) == 10  # 5 validation images per epoch, 2 epochs
    last = []
    for ycbcr, y_hr, r, dev in seen[5:]:
        assert set(dev) == {"SSIM", "MS-SSIM"}
        for i in range(ycbcr.shape[0]):
            host = M.ms_ssim(ycbcr[i, 0], y_hr[i, 0], max_value=r)
            assert abs(dev["MS-SSIM"][i] - host) <= 1e-9
            assert abs(dev["SSIM"][i] - M.ssim(ycbcr[i, 0], y_hr[i, 0], max_value=r)) <= 1e-9
            last.append(host)
    assert abs(total["val-MS-SSIM"][-1] - np.mean(last)) <= 1e-9
    d = os.path.join(GOLDEN, "set5")
    df, avg = sisr_amd.cli.eval_sisr(model_and_epoch=[[cfg["experiment"], "1"]], model_loc=str(tmp_path), gpu=True,
                                     hr_dir=os.path.join(d, "hr"), lr_dir=os.path.join(d, "lr_random_blur"),
                                     full_directory=True, scale=4, out_loc=str(tmp_path), results_name="ev",
                                     metrics=["PSNR", "SSIM", "MS-SSIM"], lr_baseline=True)
    assert list(df.columns) == ["Image_Name", "Model", "PSNR", "SSIM", "MS-SSIM", "runtime"]
    assert list(avg.columns) == ["Model", "PSNR", "SSIM", "MS-SSIM", "runtime"]
    assert len(df) == 10 and sorted(avg["Model"]) == sorted(["LR", cfg["experiment"]])
    model = float(avg.loc[avg["Model"] == cfg["experiment"], "MS-SSIM"].iloc[0])
    assert abs(model - total["val-MS-SSIM"][-1]) <= 1e-9
    # the LR baseline rows: the host form of the Y of the Pillow-bicubic up-sampled LR image against the HR image's
    lr_rows = df[df["Model"] == "LR"]
    pairs = {name: (x[0, 0].numpy(), y[0, 0].numpy()) for name, x, y in B.set5_interp()}
    assert len(lr_rows) == 5 and sorted(lr_rows["Image_Name"]) == sorted(pairs)
    for _, row in lr_rows.iterrows():
        host = M.ms_ssim(*pairs[row["Image_Name"]], max_value=1)
        print(f"LR row {row['Image_Name']}: MS-SSIM {row['MS-SSIM']:.12f} host {host:.12f}")
        assert 0 < host < 1 and abs(row["MS-SSIM"] - host) <= 1e-9
        assert abs(row["SSIM"] - M.ssim(*pairs[row["Image_Name"]], max_value=1)) <= 1e-9
    lr_avg = float(avg.loc[avg["Model"] == "LR", "MS-SSIM"].iloc[0])
    assert abs(lr_avg - float(lr_rows["MS-SSIM"].mean())) <= 1e-9
    # without the metric in the list the column is absent
    df2, _ = sisr_amd.cli.eval_sisr(model_and_epoch=[[cfg["experiment"], "1"]], model_loc=str(tmp_path), gpu=True,
                                    hr_dir=os.path.join(d, "hr"), lr_dir=os.path.join(d, "lr_random_blur"),
                                    full_directory=True, scale=4, out_loc=str(tmp_path), results_name="ev2",
                                    metrics=["PSNR", "SSIM"])
    assert list(df2.columns) == ["Image_Name", "Model", "PSNR", "SSIM", "runtime"]
