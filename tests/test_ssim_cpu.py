"""SSIM on the host (metrics.ssim, the float64 form of the reference's skimage call), its place in train_sisr / eval_sisr,
and the host-side argument checks of the device entry points (no GPU needed)."""
import copy
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import sisr_amd
from _ssim_common import set5_y_pairs
from conftest import GOLDEN, golden_json
from oracle import sisr_oracle as O

M = sisr_amd.metrics


def _scipy_ssim(a, b, data_range):
    """skimage.metrics.structural_similarity(a, b, data_range, gaussian_weights=True, sigma=1.5,
    use_sample_covariance=False), float64 form, restated on scipy.ndimage."""
    nd = pytest.importorskip("scipy.ndimage")
    x, y = np.asarray(a, np.float64), np.asarray(b, np.float64)

    def f(m):
        return nd.gaussian_filter(m, sigma=1.5, truncate=3.5, mode="reflect")
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    return s[5:-5, 5:-5].mean(dtype=np.float64)


def test_host_ssim_matches_the_scipy_restatement():
    pytest.importorskip("scipy.ndimage")
    for name, hr, lr in set5_y_pairs():
        assert abs(M.ssim(lr, hr, max_value=1) - _scipy_ssim(lr, hr, 1)) <= 1e-13, name
    g = np.random.default_rng(5)
    for h, w in ((11, 11), (11, 40), (37, 13), (228, 344)):
        a = g.random((h, w), dtype=np.float32)
        b = np.clip(a + np.float32(0.2) * g.standard_normal((h, w)).astype(np.float32), 0, 1)
        for r in (1, 255):
            assert abs(M.ssim(a * np.float32(r), b * np.float32(r), max_value=r) -
                       _scipy_ssim(a * np.float32(r), b * np.float32(r), r)) <= 1e-13, (h, w, r)


def test_host_ssim_exact_cases():
    g = np.random.default_rng(6)
    x = g.random((40, 33), dtype=np.float32)
    assert M.ssim(x, x) == 1.0
    assert M.ssim(x * np.float32(255), x * np.float32(255), max_value=255) == 1.0
    # Two constant images: (2 c1 c2 + C1) / (c1^2 + c2^2 + C1), up to rounding.  The filtered maps of a constant image are
    # c and c^2 only up to the taps' rounding, which leaves a variance of a few ulp of c^2; S divides it by C2 = (0.03 R)^2.
    # That stays under 1e-14 for these pairs; it need not for every pair (0.25 against 0.75 gives 1.8e-13), hence the
    # looser bound on random pairs.
    def const_pair(c1, c2, r):
        a, b = np.full((19, 23), c1, np.float32), np.full((19, 23), c2, np.float32)
        x, y, k1 = float(a[0, 0]), float(b[0, 0]), (0.01 * r) ** 2
        return M.ssim(a, b, max_value=r), (2 * x * y + k1) / (x * x + y * y + k1)
    for c1, c2, r in ((0.0, 1.0, 1.0), (0.25, 0.5, 1.0), (0.125, 0.5, 1.0), (0.3, 0.6, 1.0), (12.0, 200.0, 255.0),
                      (64.0, 128.0, 255.0)):
        got, want = const_pair(c1, c2, r)
        assert abs(got - want) <= 1e-14, (c1, c2, r)
    for c1, c2 in g.random((20, 2)):
        got, want = const_pair(c1, c2, 1.0)
        assert abs(got - want) <= 1e-12, (c1, c2)
    for shape in ((10, 50), (50, 10), (10, 10)):
        with pytest.raises(ValueError, match="win_size exceeds image extent"):
            M.ssim(np.zeros(shape, np.float32), np.zeros(shape, np.float32))


def test_host_batch_entry_compares_clipped_y():
    """batch_ssim on host data = y_ssim per image: RGB clipped to [0, 1], then Y; a 1-channel batch is used as given."""
    g = np.random.default_rng(7)
    sr = (g.random((3, 3, 24, 31), dtype=np.float32) * np.float32(1.4) - np.float32(0.2))
    hr = g.random((3, 3, 24, 31), dtype=np.float32)
    got = M.batch_ssim(torch.from_numpy(sr), torch.from_numpy(hr))
    assert got == [M.y_ssim(sr[i], hr[i]) for i in range(3)]
    ys, yh = M.batch_rgb_to_ycbcr(sr)[:, :1], M.batch_rgb_to_ycbcr(hr)[:, :1]
    assert M.batch_ssim(ys, yh, max_value=1) == got
    with pytest.raises(ValueError):
        M.batch_ssim(sr[:, :2], hr[:, :2])


# ----------------------------------------------------------------------------- train_sisr / eval_sisr
def _config(tmp_path, metrics):
    cfg = copy.deepcopy(golden_json("g5_train_sisr")["edsr"]["config"])
    cfg["experiment_save_loc"] = str(tmp_path)
    cfg["training"]["metrics"] = metrics
    for part in ("training_sets", "eval_sets"):
        for d in cfg["data"][part].values():
            d["lr"] = d["lr"].replace("SET5", os.path.join(GOLDEN, "set5"))
            d["hr"] = d["hr"].replace("SET5", os.path.join(GOLDEN, "set5"))
    return cfg


def _oracle_interfaces(monkeypatch):
    """Drive every ModelInterface's network by the oracle forward, as test_train_cli.py does."""
    real_init = sisr_amd.cli.ModelInterface.__init__

    def patched(self, *a, **k):
        real_init(self, *a, **k)
        net = self.model.net
        net.forward = lambda x: O.edsr(dict(net.state_dict(keep_vars=True)), x, num_blocks=2, scale=4, res_scale=0.1)
        self.model.criterion = torch.nn.L1Loss()
    monkeypatch.setattr(sisr_amd.cli.ModelInterface, "__init__", patched)


def _eval(tmp_path, cfg, results_name, **kw):
    d = os.path.join(GOLDEN, "set5")
    return sisr_amd.cli.eval_sisr(model_and_epoch=[[cfg["experiment"], "1"]], model_loc=str(tmp_path),
                                  hr_dir=os.path.join(d, "hr"), lr_dir=os.path.join(d, "lr_random_blur"), full_directory=True,
                                  scale=4, out_loc=str(tmp_path), results_name=results_name, time_models=False, **kw)


def test_train_and_eval_write_ssim_columns_with_oracle_net(tmp_path, monkeypatch):
    import pandas as pd
    ref = golden_json("g5_train_sisr")["edsr"]["summary"]
    cfg = _config(tmp_path, ["PSNR", "SSIM"])
    _oracle_interfaces(monkeypatch)
    total = sisr_amd.cli.train_sisr(cfg)
    for key in ("train-loss", "val-loss", "val-PSNR", "learning-rate"):  # SSIM draws nothing from any RNG
        np.testing.assert_allclose(total[key], ref[key], rtol=2e-5, atol=2e-6, err_msg=key)
    assert len(total["val-SSIM"]) == 2 and all(0.0 < v < 1.0 for v in total["val-SSIM"])
    summary = os.path.join(str(tmp_path), cfg["experiment"], "result_outputs", "summary.csv")
    cols = list(pd.read_csv(summary).columns)
    assert cols.index("val-SSIM") == cols.index("val-PSNR") + 1 and cols.index("epoch") == cols.index("val-SSIM") + 1

    df, avg = _eval(tmp_path, cfg, "ev_ssim", metrics=["PSNR", "SSIM"])
    assert list(df.columns) == ["Image_Name", "Model", "PSNR", "SSIM", "runtime"]
    assert list(avg.columns) == ["Model", "PSNR", "SSIM", "runtime"]
    assert len(df) == 5 and abs(float(avg["SSIM"].iloc[0]) - total["val-SSIM"][-1]) <= 1e-12
    assert abs(float(avg["PSNR"].iloc[0]) - ref["val-PSNR"][1]) < 1e-4
    mdir = os.path.join(str(tmp_path), "ev_ssim", "standard_metrics")
    assert "SSIM" in pd.read_csv(os.path.join(mdir, "individual_metrics.csv")).columns
    assert "SSIM" in pd.read_csv(os.path.join(mdir, "average_metrics.csv")).columns

    df0, avg0 = _eval(tmp_path, cfg, "ev_plain")  # without `metrics`: the columns of before
    assert list(df0.columns) == ["Image_Name", "Model", "PSNR", "runtime"]
    assert list(avg0.columns) == ["Model", "PSNR", "runtime"]
    np.testing.assert_array_equal(df0["PSNR"], df["PSNR"])


def test_train_metric_columns_follow_the_listed_order(tmp_path, monkeypatch):
    import pandas as pd
    cfg = _config(tmp_path, ["SSIM", "PSNR"])
    cfg["training"]["num_epochs"] = 1
    _oracle_interfaces(monkeypatch)
    sisr_amd.cli.train_sisr(cfg)
    cols = list(pd.read_csv(os.path.join(str(tmp_path), cfg["experiment"], "result_outputs", "summary.csv")).columns)
    assert cols[-3:] == ["val-SSIM", "val-PSNR", "epoch"]


# ----------------------------------------------------------------------------- C ABI
def test_ssim_entry_points_refuse_bad_arguments_before_any_device_call():
    """sisr_ssim validates everything on the host and returns SISR_ERR_ARG without a launch (this runs with no GPU)."""
    L = sisr_amd.hip.lib()
    buf = (C.c_double * 64)()
    p = C.addressof(buf)  # a non-null stand-in: every call below must fail before it is dereferenced
    ERR_ARG = -1
    ws = L.sisr_ssim_workspace_bytes(2, 64, 48)
    assert ws > 0 and ws % 8 == 0
    assert L.sisr_ssim_workspace_bytes(4, 64, 48) == 2 * ws
    for n, h, w in ((0, 64, 48), (-1, 64, 48), (2, 10, 48), (2, 64, 10)):
        assert L.sisr_ssim_workspace_bytes(n, h, w) == 0

    def call(a=p, b=p, n=2, ch=3, h=64, w=48, r=1.0, out=p, work=p, nbytes=ws):
        return L.sisr_ssim(a, b, n, ch, h, w, r, out, work, nbytes, None)
    assert call(a=None) == ERR_ARG
    assert call(b=None) == ERR_ARG
    assert call(out=None) == ERR_ARG
    assert call(work=None) == ERR_ARG
    assert call(n=0) == ERR_ARG and call(n=-3) == ERR_ARG
    assert call(h=10) == ERR_ARG and call(w=10) == ERR_ARG and call(h=0) == ERR_ARG
    for ch in (0, 2, 4, -1):
        assert call(ch=ch) == ERR_ARG, ch
    for r in (0.0, -1.0, math.inf, -math.inf, math.nan):
        assert call(r=r) == ERR_ARG, r
    assert call(nbytes=ws - 1) == ERR_ARG and call(nbytes=0) == ERR_ARG
    assert call(n=3) == ERR_ARG  # the workspace of two images is short for three
