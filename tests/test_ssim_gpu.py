"""Device SSIM (csrc/metrics.hip, sisr_ssim) against the host float64 form metrics.ssim, and SSIM validation through the
train / eval entry points on the HIP kernels.  numpy only: no scipy on the device tier."""
import copy
import os

import numpy as np
import pytest
import torch

import sisr_amd
from _ssim_common import set5_rgb_pairs, set5_y_pairs
from _ssim_loss import SHAPES
from conftest import GOLDEN, golden_json

M = sisr_amd.metrics
hip = sisr_amd.hip


def _device_ssim(a, b, data_range, channels):
    """(n, channels, h, w) fp32 numpy batches -> n float64 SSIMs from one sisr_ssim call (the raw float64 device values)."""
    n, c, h, w = a.shape
    assert c == channels
    da, db = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (a, b))
    L = hip.lib()
    nbytes = L.sisr_ssim_workspace_bytes(n, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    hip.check(L.sisr_ssim(da.data_ptr(), db.data_ptr(), n, channels, h, w, float(data_range), out.data_ptr(), ws.data_ptr(),
                          nbytes, hip.stream()), "sisr_ssim")
    return out.cpu().numpy()


def _planes(g, n, h, w):
    a = g.random((n, 1, h, w), dtype=np.float32)
    b = np.clip(a + np.float32(0.15) * g.standard_normal((n, 1, h, w)).astype(np.float32), 0, 1)
    return a, b


@pytest.mark.gpu
def test_y_planes_match_the_host_form():
    g = np.random.default_rng(11)
    cases = [_planes(g, 1, h, w) for h, w in ((11, 11), (11, 4096), (4096, 11), (228, 344), (1356, 2040))]
    cases.append(_planes(g, 4, 96, 96))
    for h, w in sorted({p[1].shape for p in set5_y_pairs()}):
        pairs = [p for p in set5_y_pairs() if p[1].shape == (h, w)]
        cases.append((np.stack([p[2] for p in pairs])[:, None], np.stack([p[1] for p in pairs])[:, None]))
    for a, b in cases:
        for r in (1, 255):
            ar, br = a * np.float32(r), b * np.float32(r)
            got = _device_ssim(ar, br, r, 1)
            want = [M.ssim(ar[i, 0], br[i, 0], max_value=r) for i in range(a.shape[0])]
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, err_msg=str((a.shape, r)))


@pytest.mark.gpu
def test_rgb_inputs_are_clipped_to_the_hosts_y_bit_for_bit():
    """channels = 3 on RGB with SR overshoot outside [0, 1] = channels = 1 on the Y planes metrics.batch_rgb_to_ycbcr makes."""
    g = np.random.default_rng(12)
    for n, h, w in ((2, 57, 86), (1, 512, 512), (3, 11, 300)):
        sr = g.random((n, 3, h, w), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)
        hr = g.random((n, 3, h, w), dtype=np.float32)
        ys, yh = M.batch_rgb_to_ycbcr(sr)[:, :1], M.batch_rgb_to_ycbcr(hr)[:, :1]
        rgb = _device_ssim(sr, hr, 1, 3)
        assert rgb.tobytes() == _device_ssim(ys, yh, 1, 1).tobytes()
        np.testing.assert_allclose(rgb, [M.ssim(ys[i, 0], yh[i, 0]) for i in range(n)], rtol=0, atol=1e-12)
        assert rgb.tobytes() == _device_ssim(sr, hr, 1, 3).tobytes()  # a repeat launch is bit-identical
        assert (_device_ssim(sr, sr, 1, 3) == 1.0).all() and (_device_ssim(ys, ys, 1, 1) == 1.0).all()
    for name, s_hr, s_lr in set5_rgb_pairs():
        got = _device_ssim(s_lr[None], s_hr[None], 1, 3)[0]
        assert abs(got - M.y_ssim(s_lr, s_hr)) <= 1e-12, name
    sr[0, 1, 5, 7] = np.nan  # NaN stays NaN through the clip, as with np.clip
    out = _device_ssim(sr, hr, 1, 3)
    assert np.isnan(out[0]) and not np.isnan(out[1:]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [s[2:] for s in SHAPES], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_edge_tiles_of_the_shared_window_kernel(hw):
    """the metric runs the loss's tile kernel: the smallest shapes at which its tiling can go wrong (tests/_ssim_loss.py),
    as Y planes and as RGB with overshoot"""
    h, w = hw
    g = np.random.default_rng(14 + h * w)
    a, b = _planes(g, 2, h, w)
    for r in (1, 255):
        ar, br = a * np.float32(r), b * np.float32(r)
        want = [M.ssim(ar[i, 0], br[i, 0], max_value=r) for i in range(2)]
        np.testing.assert_allclose(_device_ssim(ar, br, r, 1), want, rtol=0, atol=1e-12)
    sr = g.random((2, 3, h, w), dtype=np.float32) * np.float32(1.5) - np.float32(0.25)
    hr = g.random((2, 3, h, w), dtype=np.float32)
    ys, yh = M.batch_rgb_to_ycbcr(sr)[:, :1], M.batch_rgb_to_ycbcr(hr)[:, :1]
    rgb = _device_ssim(sr, hr, 1, 3)
    assert rgb.tobytes() == _device_ssim(ys, yh, 1, 1).tobytes()
    np.testing.assert_allclose(rgb, [M.ssim(ys[i, 0], yh[i, 0]) for i in range(2)], rtol=0, atol=1e-12)


@pytest.mark.gpu
def test_batch_entry_takes_device_tensors():
    g = np.random.default_rng(13)
    sr = torch.from_numpy(g.random((2, 3, 40, 52), dtype=np.float32) * np.float32(1.2))
    hr = torch.from_numpy(g.random((2, 3, 40, 52), dtype=np.float32))
    dev = M.batch_ssim(sr.cuda(), hr)  # the host batch follows the device one
    host = M.batch_ssim(sr, hr)
    np.testing.assert_allclose(dev, host, rtol=0, atol=1e-12)
    nc = M.batch_ssim(sr.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2), hr.cuda())  # made contiguous here
    assert nc == dev


def _config(name, tmp_path):
    cfg = copy.deepcopy(golden_json("g5_train_sisr")[name]["config"])
    cfg["experiment_save_loc"] = str(tmp_path)
    for part in ("training_sets", "eval_sets"):
        for d in cfg["data"][part].values():
            d["lr"] = d["lr"].replace("SET5", os.path.join(GOLDEN, "set5"))
            d["hr"] = d["hr"].replace("SET5", os.path.join(GOLDEN, "set5"))
    return cfg


@pytest.mark.gpu
def test_train_and_eval_entry_points_measure_ssim_on_hip(tmp_path, monkeypatch):
    ref = golden_json("g5_train_sisr")["edsr"]["summary"]
    cfg = _config("edsr", tmp_path)
    cfg["training"].update(gpu="single", sp_gpu=0, metrics=["PSNR", "SSIM"])
    seen = []  # the validation outputs (Y of the clipped output, as the host sees them), HR and what the device measured
    real = sisr_amd.handlers.ModelInterface.net_run_process_and_measure

    def spy(self, lr=None, hr=None, **kw):
        res = real(self, lr=lr, hr=hr, **kw)
        seen.append((res[1], M.batch_rgb_to_ycbcr(hr.numpy()), kw["max_value"], res[4]["SSIM"]))
        return res
    monkeypatch.setattr(sisr_amd.handlers.ModelInterface, "net_run_process_and_measure", spy)
    total = sisr_amd.cli.train_sisr(cfg)
    np.testing.assert_allclose(total["train-loss"], ref["train-loss"], rtol=2e-4, atol=2e-5)
    np.testing.assert_allclose(total["val-loss"], ref["val-loss"], rtol=5e-4, atol=5e-5)
    np.testing.assert_allclose(total["val-PSNR"], ref["val-PSNR"], rtol=0, atol=5e-3)  # dB
    assert len(seen) == 10  # 5 validation images per epoch, 2 epochs
    last = []
    for ycbcr, y_hr, r, dev in seen[5:]:
        for i in range(ycbcr.shape[0]):
            host = M.ssim(ycbcr[i, 0], y_hr[i, 0], max_value=r)
            assert abs(dev[i] - host) <= 1e-9
            last.append(host)
    assert abs(total["val-SSIM"][-1] - np.mean(last)) <= 1e-9
    d = os.path.join(GOLDEN, "set5")
    df, avg = sisr_amd.cli.eval_sisr(model_and_epoch=[[cfg["experiment"], "1"]], model_loc=str(tmp_path), gpu=True,
                                     hr_dir=os.path.join(d, "hr"), lr_dir=os.path.join(d, "lr_random_blur"),
                                     full_directory=True, scale=4, out_loc=str(tmp_path), results_name="ev",
                                     metrics=["PSNR", "SSIM"])
    assert list(df.columns) == ["Image_Name", "Model", "PSNR", "SSIM", "runtime"]
    assert len(df) == 5 and abs(float(avg["SSIM"].iloc[0]) - total["val-SSIM"][-1]) <= 1e-9
