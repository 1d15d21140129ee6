"""The evaluator's bicubic pre-up-sampling on the device (csrc/interp.hip, degrade.pil_bicubic_upsample) against its host form
(Pillow), bit for bit, and eval_sisr on the HIP path for an interpolated-YCbCr model (srcnn) and an interpolated-RGB model
(a reduced sparnet), both evaluated from the raw LR folder."""
import os

import numpy as np
import pytest
import torch

import _basic as R
import sisr_amd
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
SET5 = os.path.join(GOLDEN, "set5")
# (2, 3, 5, 7): two images, x3 gives a width that is no multiple of 4 (the lane-by-lane store form); (1, 3, 1, 1): one pixel;
# (1, 3, 33, 65) x4: partial tiles in both directions and fewer rows than a tile's halo; (1, 3, 57, 86): Set5's odd one;
# (1, 3, 16, 16) x1: the resampler is the identity there, so the plane of all 256 bytes comes out as all 256 bytes / 255
CASES = [((2, 3, 5, 7), 2), ((2, 3, 5, 7), 3), ((2, 3, 5, 7), 4), ((1, 3, 1, 1), 4), ((1, 3, 33, 65), 4), ((1, 3, 57, 86), 4),
         ((1, 3, 16, 16), 1)]


def _batch(shape, seed):
    """seeded fp32 in [0, 1) -- general floats, not only k / 255; where a plane has room, its first 256 values are k / 255"""
    lr = torch.rand(shape, generator=torch.Generator().manual_seed(seed))
    if shape[2] * shape[3] >= 256:
        lr[0, 0].view(-1)[:256] = torch.arange(256, dtype=torch.float32).div(255)
    return lr


@pytest.mark.parametrize("shape, scale", CASES)
def test_kernel_equals_the_host_form_bit_for_bit(shape, scale):
    lr = _batch(shape, seed=shape[2] * 10 + scale)
    want_rgb = sisr_amd.cli._low_res_prep(lr, scale).numpy()
    want_ycc = sisr_amd.metrics.batch_rgb_to_ycbcr(want_rgb)
    if scale == 1:
        assert len(np.unique(want_rgb[0, 0])) == 256
    dev = lr.to("cuda:0")
    rgb, ycc = sisr_amd.degrade.pil_bicubic_upsample(dev, scale, rgb=True, ycbcr=True)
    assert rgb.is_cuda and ycc.is_cuda and rgb.dtype == torch.float32
    np.testing.assert_array_equal(rgb.cpu().numpy(), want_rgb)
    np.testing.assert_array_equal(ycc.cpu().numpy(), want_ycc)
    # one output at a time: the same launch with the other pointer null
    np.testing.assert_array_equal(sisr_amd.degrade.pil_bicubic_upsample(dev, scale).cpu().numpy(), want_rgb)
    only = sisr_amd.degrade.pil_bicubic_upsample(dev, scale, rgb=False, ycbcr=True)
    np.testing.assert_array_equal(only.cpu().numpy(), want_ycc)


def _train(tmp_path, model=None, experiment=None):
    cfg = R.b4_config(tmp_path)
    if model is not None:
        cfg["model"], cfg["experiment"] = model, experiment
    cfg["training"].update(gpu="single", sp_gpu=0, metrics=["PSNR", "SSIM"])
    return cfg, sisr_amd.cli.train_sisr(cfg)


def _eval(tmp_path, cfg, total, **kw):
    last = len(total["epoch"]) - 1
    return sisr_amd.cli.eval_sisr(model_and_epoch=[[cfg["experiment"], str(last)]], model_loc=str(tmp_path), gpu=True,
                                  hr_dir=os.path.join(SET5, "hr"), lr_dir=os.path.join(SET5, "lr_random_blur"),
                                  full_directory=True, scale=4, out_loc=str(tmp_path), results_name="ev",
                                  metrics=["PSNR", "SSIM"], **kw)


def _check(df, avg, cfg, total):
    assert list(df.columns) == ["Image_Name", "Model", "PSNR", "SSIM", "runtime"]
    mine = avg[avg["Model"] == cfg["experiment"]]
    assert len(df[df["Model"] == cfg["experiment"]]) == 5 and len(mine) == 1
    print(float(mine["PSNR"].iloc[0]), total["val-PSNR"][-1], float(mine["SSIM"].iloc[0]), total["val-SSIM"][-1])
    assert abs(float(mine["PSNR"].iloc[0]) - total["val-PSNR"][-1]) < 5e-3
    assert abs(float(mine["SSIM"].iloc[0]) - total["val-SSIM"][-1]) <= 1e-9


def test_eval_sisr_on_hip_feeds_srcnn_interpolated_ycbcr(tmp_path):
    """train_sisr validates on a Pillow-made folder of interpolated images; eval_sisr makes them on the device from the raw
    LR folder and reproduces the last validation.  The LR baseline rows are the device images' own Y-PSNR."""
    cfg, total = _train(tmp_path)
    df, avg = _eval(tmp_path, cfg, total, lr_baseline=True)
    _check(df, avg, cfg, total)
    base = df[df["Model"] == "LR"]
    want = {name: R.psnr(x[0, 0].numpy(), y[0, 0].numpy()) for name, x, y in R.set5_interp()}
    assert dict(zip(base["Image_Name"], base["PSNR"])) == want
    assert all(t is not None and t > 0 for t in base["runtime"])


def test_eval_sisr_on_hip_feeds_sparnet_interpolated_rgb(tmp_path):
    """a reduced SPARNet whose maps halve twice at most (Set5's sides are multiples of 4, not all of 8)"""
    model = {"name": "sparnet", "internal_params": {"scale": 1, "lr": 1e-4, "min_ch": 32, "max_ch": 128, "in_size": 32,
                                                    "out_size": 32, "min_feat_size": 8, "res_depth": 1, "bottleneck_size": 32}}
    cfg, total = _train(tmp_path, model, "b4_sparnet")
    df, avg = _eval(tmp_path, cfg, total)
    assert len(df) == 5
    _check(df, avg, cfg, total)
