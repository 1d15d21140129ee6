"""The evaluator's bicubic pre-up-sampling on the host (cli._low_res_prep, the tables of degrade.pil_bicubic_table) against
Pillow, eval_sisr's choice of each model's input (raw LR / interpolated RGB / interpolated YCbCr), its `lr_dir_interp` and
`lr_baseline` keys, and the host-side argument checks of sisr_pil_upsample (no GPU needed)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from PIL import Image

import _basic as R
import sisr_amd
from conftest import GOLDEN

SIZES = [(1, 1), (2, 3), (5, 7), (33, 65), (57, 86)]
SCALES = [2, 3, 4]
SET5 = os.path.join(GOLDEN, "set5")


def _bytes_image(h, w, seed):
    """(h, w, 3) uint8, seeded; where it has room, its first plane starts with every byte value 0 ... 255"""
    u8 = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if h * w >= 256:
        u8[:, :, 0].flat[:256] = np.arange(256, dtype=np.uint8)
    return u8


def _two_pass(u8, scale):
    """libImaging/Resample.c's 8-bit resampler in numpy integers on the tables the device kernel is given"""
    h, w, _ = u8.shape
    passes = []
    for size in (w, h):
        bounds, coef, ksize = sisr_amd.degrade.pil_bicubic_table(size, size * scale)
        assert ksize == 5
        passes.append((bounds, coef))
    img = u8.astype(np.int64)
    for axis, (bounds, coef) in ((1, passes[0]), (0, passes[1])):
        img = np.moveaxis(img, axis, 0)
        out = np.empty((len(bounds),) + img.shape[1:], np.int64)
        for o, (lo, n) in enumerate(bounds):
            ss = (1 << 21) + np.tensordot(coef[o, :n].astype(np.int64), img[lo:lo + n], axes=1)
            out[o] = np.clip(ss >> 22, 0, 255)
        img = np.moveaxis(out, 0, axis)
    return img.astype(np.uint8)


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("hw", SIZES)
def test_host_prep_and_tables_equal_pillow(hw, scale):
    h, w = hw
    u8 = _bytes_image(h, w, seed=100 * h + scale)
    pil = np.asarray(Image.fromarray(u8).resize((w * scale, h * scale), Image.BICUBIC))
    # ToTensor's float32 division; for bytes it is the float64 quotient rounded once
    want = pil.astype(np.float32) / np.float32(255)
    np.testing.assert_array_equal(want, (pil / 255).astype(np.float32))
    lr = torch.from_numpy(u8.transpose(2, 0, 1).copy()).float().div(255)[None]  # k / 255 * 255 must truncate back to k
    got = sisr_amd.cli._low_res_prep(lr, scale)
    assert got.dtype == torch.float32 and tuple(got.shape) == (1, 3, h * scale, w * scale)
    np.testing.assert_array_equal(got[0].numpy().transpose(1, 2, 0), want)
    np.testing.assert_array_equal(_two_pass(u8, scale), pil)


def test_host_prep_truncates_general_floats_as_to_pil_image():
    g = torch.Generator().manual_seed(9)
    lr = torch.rand(2, 3, 5, 7, generator=g)
    got = sisr_amd.cli._low_res_prep(lr, 3)
    for i in range(2):
        u8 = (lr[i].numpy() * np.float32(255)).astype(np.int32).astype(np.uint8).transpose(1, 2, 0)
        pil = np.asarray(Image.fromarray(u8).resize((21, 15), Image.BICUBIC))
        np.testing.assert_array_equal(got[i].numpy().transpose(1, 2, 0), pil.astype(np.float32) / np.float32(255))


# ----------------------------------------------------------------------------- eval_sisr
@pytest.fixture(scope="module")
def trained_srcnn(tmp_path_factory):
    """the b4 fixture's srcnn run (its validation reads a Pillow-made folder of interpolated images), the network driven by
    a plain torch forward as in test_basic_cpu.py; the patch stays for the module's eval_sisr calls"""
    tmp = tmp_path_factory.mktemp("interp_eval")
    cfg = R.b4_config(tmp)
    real_init = sisr_amd.cli.ModelInterface.__init__

    def patched(self, *a, **k):
        real_init(self, *a, **k)
        net = self.model.net
        net.forward = lambda x: R.net_ref(dict(net.state_dict(keep_vars=True)), x, False, dtype=torch.float32)
        self.model.criterion = torch.nn.MSELoss()
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(sisr_amd.cli.ModelInterface, "__init__", patched)
        total = sisr_amd.cli.train_sisr(cfg)
        yield tmp, cfg, total


def _eval(trained, results_name, **kw):
    tmp, cfg, total = trained
    last = len(total["epoch"]) - 1
    return sisr_amd.cli.eval_sisr(model_and_epoch=[[cfg["experiment"], str(last)]], model_loc=str(tmp),
                                  hr_dir=os.path.join(SET5, "hr"), lr_dir=os.path.join(SET5, "lr_random_blur"),
                                  full_directory=True, scale=4, out_loc=str(tmp), results_name=results_name, time_models=False,
                                  **kw)


def test_eval_sisr_feeds_a_y_channel_model_from_the_raw_lr_folder(trained_srcnn):
    """fails without the input selection: the net would be handed the R plane of the LR image"""
    df, avg = _eval(trained_srcnn, "ev_y")
    total = trained_srcnn[2]
    assert len(df) == 5 and list(df.columns) == ["Image_Name", "Model", "PSNR", "runtime"]
    assert abs(float(avg["PSNR"].iloc[0]) - total["val-PSNR"][-1]) < 1e-4


def test_eval_sisr_lr_baseline_and_interp_folder(trained_srcnn):
    tmp, cfg, _ = trained_srcnn
    df0, avg0 = _eval(trained_srcnn, "ev_plain")
    df, avg = _eval(trained_srcnn, "ev_base", lr_baseline=True)
    assert list(df.columns) == list(df0.columns) and len(df0) == 5 and len(df) == 10
    base, rest = df[df["Model"] == "LR"], df[df["Model"] != "LR"]
    assert len(base) == 5 and list(rest["Model"]) == [cfg["experiment"]] * 5
    np.testing.assert_array_equal(rest["PSNR"].to_numpy(), df0["PSNR"].to_numpy())
    want = {name: R.psnr(x[0, 0].numpy(), y[0, 0].numpy()) for name, x, y in R.set5_interp()}
    got = dict(zip(base["Image_Name"], base["PSNR"]))
    assert got == want
    assert sorted(avg["Model"]) == sorted(["LR", cfg["experiment"]])
    # SSIM listed: the baseline rows carry it too
    dfs, _ = _eval(trained_srcnn, "ev_base_ssim", lr_baseline=True, metrics=["PSNR", "SSIM"])
    assert list(dfs.columns) == ["Image_Name", "Model", "PSNR", "SSIM", "runtime"]
    pairs = {name: (x, y) for name, x, y in R.set5_interp()}
    for _, row in dfs[dfs["Model"] == "LR"].iterrows():
        x, y = pairs[row["Image_Name"]]
        assert abs(row["SSIM"] - sisr_amd.metrics.ssim(x[0, 0].numpy(), y[0, 0].numpy(), max_value=1)) <= 1e-12
    # ready-made interpolated images (the folder b4_config wrote with Pillow) in place of computing them
    dfi, _ = _eval(trained_srcnn, "ev_folder", lr_baseline=True, lr_dir_interp=os.path.join(str(tmp), "interp"))
    np.testing.assert_array_equal(dfi["PSNR"].to_numpy(), df["PSNR"].to_numpy())
    assert list(dfi["Model"]) == list(df["Model"]) and list(dfi["Image_Name"]) == list(df["Image_Name"])


def test_eval_sisr_still_refuses_another_scale_for_an_lr_input_model(tmp_path):
    """the scale check now lives in eval_sisr; a model fed the raw LR image keeps it"""
    params = {"name": "edsr", "internal_params": {"scale": 2, "num_blocks": 1, "num_features": 64}}
    torch.manual_seed(8)
    mi = sisr_amd.ModelInterface(str(tmp_path), "exp", mode="train", new_params=params)
    sisr_amd.cli._dump_toml({"model": params}, os.path.join(mi.base_folder, "config.toml"))
    mi.save()
    with pytest.raises(Exception, match="trained for a different scale"):
        sisr_amd.cli.eval_sisr(model_and_epoch=[["exp", "0"]], model_loc=str(tmp_path), hr_dir=os.path.join(SET5, "hr"),
                               lr_dir=os.path.join(SET5, "lr_random_blur"), full_directory=True, scale=4,
                               out_loc=str(tmp_path))


# ----------------------------------------------------------------------------- C ABI
def test_pil_upsample_refuses_bad_arguments_before_any_device_call():
    """sisr_pil_upsample validates everything on the host and returns an error code without a launch (no GPU here)"""
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)  # a non-null stand-in: every call below must fail before it is dereferenced
    ARG, UNSUPPORTED = -1, -4

    def call(lr=p, rgb=p, ycbcr=p, bh=p, ch=p, bv=p, cv=p, ksize=5, B=1, Cn=3, h=8, w=6, H=32, W=24):
        return L.sisr_pil_upsample(lr, rgb, ycbcr, bh, ch, bv, cv, ksize, B, Cn, h, w, H, W, None)
    assert call(lr=None) == ARG
    assert call(rgb=None, ycbcr=None) == ARG
    for name in ("bh", "ch", "bv", "cv"):
        assert call(**{name: None}) == ARG, name
    for name in ("ksize", "B", "Cn", "h", "w", "H", "W"):
        for v in (0, -2):
            assert call(**{name: v}) == ARG, (name, v)
    assert call(Cn=1) == UNSUPPORTED and call(Cn=4) == UNSUPPORTED       # YCbCr needs the three RGB planes
    assert call(H=33) == UNSUPPORTED and call(W=25) == UNSUPPORTED       # not an integer scale
    assert call(H=24, W=24) == UNSUPPORTED                               # two different scales
    assert call(ksize=9) == UNSUPPORTED and call(ksize=4) == UNSUPPORTED  # not the five taps of bicubic up-sampling
    assert call(B=65536) == UNSUPPORTED                                  # grid z
    assert call(ycbcr=None, B=21846, Cn=9) == UNSUPPORTED                # 21846 * 3 channel groups
    assert call(h=65535 * 32 + 1, H=(65535 * 32 + 1) * 4) == UNSUPPORTED  # grid y


def test_device_entry_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="HIP device"):
        sisr_amd.degrade.pil_bicubic_upsample(torch.zeros(1, 3, 4, 4), 4)
