"""The output stage of evaluation without a device: the host forms of metrics.batch_psnr / batch_rgb8 / eval_output, the
refusals of sisr_eval_output before any launch, and the device_outputs / device_metrics / psnr_shave keys of eval_sisr and
train_sisr on a CPU model."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sisr_amd
from conftest import GOLDEN, golden_json
from oracle import sisr_oracle as O

M = sisr_amd.metrics


def _noisy_pair(seed, shape, sigma=0.2):
    g = np.random.default_rng(seed)
    hr = g.random(shape, dtype=np.float32)
    sr = hr + np.float32(sigma) * g.standard_normal(shape).astype(np.float32)  # overshoots [0, 1]
    return sr, hr


# ----------------------------------------------------------------------------- host forms
def test_host_batch_psnr_is_y_psnr_and_psnr_of_the_cropped_planes():
    sr, hr = _noisy_pair(1, (3, 3, 24, 31))
    assert (sr < 0).any() and (sr > 1).any()
    got = M.batch_psnr(torch.from_numpy(sr), torch.from_numpy(hr))
    assert got == [M.y_psnr(sr[i], hr[i]) for i in range(3)]
    ys, yh = M.batch_rgb_to_ycbcr(sr)[:, :1], M.batch_rgb_to_ycbcr(hr)[:, :1]
    assert M.batch_psnr(ys, yh) == got  # Y planes in place of RGB
    for shave in (1, 4, 11):
        want = [M.psnr(ys[i, 0, shave:24 - shave, shave:31 - shave], yh[i, 0, shave:24 - shave, shave:31 - shave], 1)
                for i in range(3)]
        assert M.batch_psnr(sr, hr, shave=shave) == want
        assert M.batch_psnr(ys, yh, shave=shave) == want
    assert M.batch_psnr(sr, hr, max_value=255) == [M.y_psnr(sr[i], hr[i], max_value=255) for i in range(3)]
    assert M.batch_psnr(hr, hr) == [100, 100, 100]
    for shave in (-1, 12, 40):  # 2 * 12 >= 24: nothing is left
        with pytest.raises(ValueError, match="psnr_shave"):
            M.batch_psnr(sr, hr, shave=shave)
    with pytest.raises(ValueError):
        M.batch_psnr(sr[:, :2], hr[:, :2])


def test_host_batch_rgb8_is_the_clipped_rounded_cast_in_hwc():
    sr, _ = _noisy_pair(2, (2, 3, 9, 14))
    got = M.batch_rgb8(sr)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (2, 9, 14, 3)
    want = (np.clip(sr, 0, 1) * 255).round().astype(np.uint8).transpose(0, 2, 3, 1)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(M.batch_rgb8(torch.from_numpy(sr)), want)
    ties = ((np.arange(256, dtype=np.float64) + 0.5) / 255).astype(np.float32)  # every product with 255 is an exact tie
    assert ((ties * np.float32(255)) == np.arange(256, dtype=np.float32) + np.float32(0.5)).all()
    b = M.batch_rgb8(np.broadcast_to(ties.reshape(1, 1, 16, 16), (1, 3, 16, 16)).copy())
    k = np.arange(256)
    np.testing.assert_array_equal(b[0, :, :, 0].reshape(-1), np.minimum(np.where(k % 2 == 0, k, k + 1), 255))


def test_host_one_plane_form_saturates_where_the_cast_wraps():
    g = np.random.default_rng(3)
    ycc = (g.random((2, 3, 12, 17), dtype=np.float32) * np.float32(1.2) - np.float32(0.1))  # [-0.1, 1.1]
    got = M.batch_rgb8(ycc[:, :1], chroma=ycc)
    v = (M.batch_ycbcr_to_rgb(ycc) * 255).round().transpose(0, 2, 3, 1)
    inside = (v >= 0) & (v <= 255)
    assert inside.any() and (v < 0).any() and (v > 255).any()
    host_cast = v.astype(np.int64).astype(np.uint8)  # the wrapping cast of the existing path
    np.testing.assert_array_equal(got[inside], host_cast[inside])
    assert (got[v < 0] == 0).all() and (got[v > 255] == 255).all()
    assert (host_cast[v < 0] != 0).any()  # ... which is what wraps
    with pytest.raises(ValueError, match="chroma"):
        M.batch_rgb8(ycc[:, :1])


def test_one_helper_gives_both_results():
    sr, hr = _noisy_pair(4, (2, 3, 10, 12))
    values, rgb8 = M.eval_output(sr, hr, shave=2, want_rgb8=True)
    assert values == M.batch_psnr(sr, hr, shave=2)
    np.testing.assert_array_equal(rgb8, M.batch_rgb8(sr))
    assert M.eval_output(sr, want_psnr=False, want_rgb8=False) == (None, None)
    with pytest.raises(RuntimeError, match="reference"):
        M.eval_output(sr)
    # a Y output against a YCbCr reference: plane 0 of it
    ys, ycc = M.batch_rgb_to_ycbcr(sr)[:, :1], M.batch_rgb_to_ycbcr(hr)
    assert M.eval_output(ys, ycc)[0] == M.batch_psnr(ys, ycc[:, :1])


# ----------------------------------------------------------------------------- C ABI
def test_eval_output_refuses_bad_arguments_before_any_device_call():
    """sisr_eval_output validates everything on the host and returns an error code without a launch (no GPU here)."""
    L = sisr_amd.hip.lib()
    ERR_ARG, ERR_ALIGN = -1, -2
    buf = (C.c_double * 64)()
    a = C.addressof(buf)
    a += (16 - a % 16) % 16  # a non-null, 16-byte aligned stand-in: every call must fail before it is dereferenced
    wsb = L.sisr_eval_output_workspace_bytes
    assert wsb(1, 16, 16) >= 8 and wsb(1, 16, 16) % 16 == 0
    assert wsb(2, 1356, 2040) >= 2 * 8 * -(-1356 * 2040 // 2048)
    for n, h, w in ((0, 16, 16), (-1, 16, 16), (1, 0, 16), (1, 16, 0), (1, -4, 16), (1, 16, -4), (1, 65536, 65536)):
        assert wsb(n, h, w) == 0, (n, h, w)

    def call(sr=a, sr_planes=3, chroma=None, hr=a, hr_form=0, hr_planes=3, n=1, h=16, w=16, shave=0, mse=a, rgb8=a, ws=a,
             nbytes=None):
        nbytes = wsb(1, 16, 16) if nbytes is None else nbytes
        return L.sisr_eval_output(sr, sr_planes, chroma, hr, hr_form, hr_planes, n, h, w, shave, mse, rgb8, ws, nbytes, None)
    assert call(sr=None) == ERR_ARG
    assert call(mse=None, rgb8=None) == ERR_ARG                      # neither result
    assert call(hr=None) == ERR_ARG                                  # mse without hr
    for planes in (0, 2, 4, -1):
        assert call(sr_planes=planes) == ERR_ARG, planes
    assert call(sr_planes=1, chroma=None) == ERR_ARG                 # bytes of a Y plane need chroma
    for form in (-1, 2, 7):
        assert call(hr_form=form) == ERR_ARG, form
    assert call(hr_form=1, hr_planes=0) == ERR_ARG and call(hr_form=1, hr_planes=-2) == ERR_ARG
    assert call(hr_form=0, hr_planes=1) == ERR_ARG                   # RGB needs three planes
    for kw in ({"n": 0}, {"n": -1}, {"h": 0}, {"w": 0}, {"h": -16}, {"w": -16}):
        assert call(**kw) == ERR_ARG, kw
    for shave in (-1, 8, 9, 1000):                                   # 2 * 8 >= 16
        assert call(shave=shave) == ERR_ARG, shave
    assert call(h=5, w=40, shave=3) == ERR_ARG
    assert call(ws=None) == ERR_ARG and call(nbytes=wsb(1, 16, 16) - 1) == ERR_ARG and call(nbytes=0) == ERR_ARG
    assert call(n=3, nbytes=wsb(2, 16, 16) - 8) == ERR_ARG
    assert call(ws=a + 8) == ERR_ALIGN
    assert call(sr=a + 2) == ERR_ALIGN and call(hr=a + 1) == ERR_ALIGN and call(mse=a + 4) == ERR_ALIGN
    assert call(sr_planes=1, chroma=a + 2) == ERR_ALIGN
    assert call(h=65536, w=65536) != 0                               # a plane past 2^31 pixels


def test_device_forms_refuse_what_the_host_forms_refuse():
    """the Python entry checks shapes before it looks for a device"""
    sr, hr = _noisy_pair(5, (1, 3, 8, 8))
    with pytest.raises(ValueError):
        M.eval_output(sr[:, :2], hr)
    with pytest.raises(ValueError):
        M.eval_output(sr, hr[:, :, :7])
    with pytest.raises(ValueError, match="psnr_shave"):
        M.eval_output(sr, hr, shave=4)


# ----------------------------------------------------------------------------- train_sisr / eval_sisr
def _config(tmp_path):
    cfg = copy.deepcopy(golden_json("g5_train_sisr")["edsr"]["config"])
    cfg["experiment_save_loc"] = str(tmp_path)
    cfg["training"]["metrics"] = ["PSNR", "SSIM"]
    cfg["training"]["num_epochs"] = 1
    for part in ("training_sets", "eval_sets"):
        for d in cfg["data"][part].values():
            d["lr"] = d["lr"].replace("SET5", os.path.join(GOLDEN, "set5"))
            d["hr"] = d["hr"].replace("SET5", os.path.join(GOLDEN, "set5"))
    return cfg


def _oracle_interfaces(monkeypatch):
    """Drive every ModelInterface's network by the oracle forward, as test_ssim_cpu.py does."""
    real_init = sisr_amd.cli.ModelInterface.__init__

    def patched(self, *a, **k):
        real_init(self, *a, **k)
        net = self.model.net
        net.forward = lambda x: O.edsr(dict(net.state_dict(keep_vars=True)), x, num_blocks=2, scale=4, res_scale=0.1)
        self.model.criterion = torch.nn.L1Loss()
    monkeypatch.setattr(sisr_amd.cli.ModelInterface, "__init__", patched)


def _eval(tmp_path, cfg, results_name, **kw):
    d = os.path.join(GOLDEN, "set5")
    return sisr_amd.cli.eval_sisr(model_and_epoch=[[cfg["experiment"], "0"]], model_loc=str(tmp_path),
                                  hr_dir=os.path.join(d, "hr"), lr_dir=os.path.join(d, "lr_random_blur"), full_directory=True,
                                  scale=4, out_loc=str(tmp_path), results_name=results_name, time_models=False, **kw)


def test_cli_keys_on_a_cpu_model(tmp_path, monkeypatch):
    """psnr_shave without its switch raises; device_outputs / device_metrics on a CPU model take the host forms: the same
    CSVs as the default path, PSNR exactly equal, and the same PNGs"""
    import pandas as pd
    from PIL import Image
    _oracle_interfaces(monkeypatch)
    cfg = _config(tmp_path)
    bad = copy.deepcopy(cfg)
    bad["training"]["psnr_shave"] = 4
    with pytest.raises(ValueError, match="psnr_shave"):
        sisr_amd.cli.train_sisr(bad)
    plain = sisr_amd.cli.train_sisr(copy.deepcopy(cfg))
    with pytest.raises(ValueError, match="psnr_shave"):
        _eval(tmp_path, cfg, "ev_bad", psnr_shave=4)

    sw = copy.deepcopy(cfg)
    sw["experiment"] = cfg["experiment"] + "_dm"
    sw["training"]["device_metrics"] = True
    switched = sisr_amd.cli.train_sisr(sw)
    for key in ("train-loss", "val-loss", "val-PSNR", "val-SSIM"):
        assert list(switched[key]) == list(plain[key]), key
    assert list(pd.read_csv(os.path.join(str(tmp_path), sw["experiment"], "result_outputs", "summary.csv")).columns) == \
        list(pd.read_csv(os.path.join(str(tmp_path), cfg["experiment"], "result_outputs", "summary.csv")).columns)

    df0, avg0 = _eval(tmp_path, cfg, "ev_plain", metrics=["PSNR", "SSIM"], save_im=True)
    df1, avg1 = _eval(tmp_path, cfg, "ev_dev", metrics=["PSNR", "SSIM"], save_im=True, device_outputs=True)
    assert list(df1.columns) == list(df0.columns) and list(avg1.columns) == list(avg0.columns)
    assert list(df1["Image_Name"]) == list(df0["Image_Name"]) and list(df1["Model"]) == list(df0["Model"])
    np.testing.assert_array_equal(df1["PSNR"], df0["PSNR"])
    np.testing.assert_array_equal(df1["SSIM"], df0["SSIM"])
    for name in ("individual_metrics.csv", "average_metrics.csv"):
        a, b = (pd.read_csv(os.path.join(str(tmp_path), r, "standard_metrics", name)) for r in ("ev_plain", "ev_dev"))
        pd.testing.assert_frame_equal(a, b)
    for tag in df0["Image_Name"]:
        a, b = (np.asarray(Image.open(os.path.join(str(tmp_path), r, cfg["experiment"], os.path.basename(tag))))
                for r in ("ev_plain", "ev_dev"))
        np.testing.assert_array_equal(a, b)

    df2, _ = _eval(tmp_path, cfg, "ev_shave", device_outputs=True, psnr_shave=4)
    assert list(df2.columns) == ["Image_Name", "Model", "PSNR", "runtime"]
    assert (np.asarray(df2["PSNR"]) != np.asarray(df0["PSNR"])).all()
    assert np.abs(np.asarray(df2["PSNR"]) - np.asarray(df0["PSNR"])).max() < 1.0  # a border crop, not another metric
