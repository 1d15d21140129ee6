"""Shared inputs of the SSIM tests: Set5 HR images against their LR images brought back up by bicubic resampling."""
import glob
import os

import numpy as np

from conftest import GOLDEN


def _rgb(path, size=None):
    from PIL import Image
    im = Image.open(path).convert("RGB")
    if size is not None:
        im = im.resize(size, Image.BICUBIC)
    return np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / np.float32(255)


def set5_rgb_pairs():
    """[(name, hr, bicubic-up lr)], (3, H, W) fp32 RGB in [0, 1]."""
    d = os.path.join(GOLDEN, "set5")
    out = []
    for hr_path in sorted(glob.glob(os.path.join(d, "hr", "*.png"))):
        name = os.path.basename(hr_path)
        hr = _rgb(hr_path)
        lr = _rgb(os.path.join(d, "lr_random_blur", name), size=(hr.shape[2], hr.shape[1]))
        out.append((name, hr, lr))
    return out


def set5_y_pairs():
    """[(name, Y of hr, Y of bicubic-up lr)], (H, W) fp32, Y as metrics.batch_rgb_to_ycbcr forms it."""
    import sisr_amd
    to_y = sisr_amd.metrics.batch_rgb_to_ycbcr
    return [(n, to_y(hr[None])[0, 0], to_y(lr[None])[0, 0]) for n, hr, lr in set5_rgb_pairs()]
