"""Shared pieces of the tile-level degradation tests (test_degrade_tiles_cpu.py, test_degrade_tiles_gpu.py).

Expected values never come from the code under test: the whole-image LR image is built from the EXISTING entry points
(blur_quant, sisr_noise_quant with an explicit field, pil_bicubic_downsample, jpeg_roundtrip) and a tile is read out of it with
the index map of tests/test_device_tiles.py::gather_on_host."""
import itertools
import os

import numpy as np
import torch

import sisr_amd
from conftest import GOLDEN

D = sisr_amd.degrade
data = sisr_amd.data

FLIPS = list(itertools.product((False, True), repeat=3))  # (hflip, vflip, transpose): all 8

# Philox4x32-10 known answers (counter, key, output), checked against a direct implementation of the published rounds
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def gather_on_host(img, rec, crop):
    """tests/test_device_tiles.py::gather_on_host: sisr_crop_augment's index map, evaluated with torch on the CPU."""
    H, W, top, left, hf, vf, rot = rec
    i = torch.arange(crop).view(crop, 1).expand(crop, crop)
    j = torch.arange(crop).view(1, crop).expand(crop, crop)
    y, x = top + i, left + j
    y2, x2 = (x, y) if rot else (y, x)
    sy = (H - 1 - y2) if vf else y2
    sx = (W - 1 - x2) if hf else x2
    return img[:, sy, sx]


def draw_for_origin(h, w, crop, ty, tx, hf, vf, rot):
    """The (top, left) draw for which the index map reads the source square with origin (ty, tx): gather_on_host's map solved
    for its arguments, independently of data.tile_source_box."""
    y0 = h - crop - ty if vf else ty   # where the square starts along the (flipped) source rows ...
    x0 = w - crop - tx if hf else tx   # ... and columns
    return (x0, y0) if rot else (y0, x0)  # the transpose swaps which of them `top` counts


def random_image(H, W, seed, C=3):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(C, H, W, generator=g)


def random_kernel(l, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    k = torch.rand(l, l, generator=g)
    return k / k.sum()


def woman():
    from PIL import Image
    hr = np.asarray(Image.open(os.path.join(GOLDEN, "set5", "hr", "woman.png")).convert("RGB"))
    return torch.from_numpy(hr.transpose(2, 0, 1).copy()).float().div(255)


def whole_image_lr(hr_dev, kernel, scale, sigma=None, seed=None, to_float=True):
    """The whole-image path, stage by stage, from the existing entry points -> the (C, h, w) LR image on the device (uint8 or
    fp32 / 255).  sigma not None: the noise stage (sisr_noise_quant) fed normal_field(seed)."""
    if sigma is None:
        u8 = D.blur_quant(hr_dev, kernel)
    else:
        _, blurred = D.blur_quant(hr_dev, kernel, want_float=True, want_u8=False)
        C, H, W = hr_dev.shape
        field = D.normal_field(seed, C, H, W, hr_dev.device)
        u8 = torch.empty((C, H, W), device=hr_dev.device, dtype=torch.uint8)
        hip = sisr_amd.hip
        hip.check(hip.lib().sisr_noise_quant(hip.ptr(blurred), hip.ptr(field), float(sigma), u8.data_ptr(), blurred.numel(),
                                             hip.stream()), "sisr_noise_quant")
    top, left, rh, rw = D.center_crop_box(hr_dev.shape[1], hr_dev.shape[2], scale)
    u8 = u8[:, top:top + rh, left:left + rw].contiguous()
    return D.pil_bicubic_downsample(u8, scale, to_float=to_float)


def origins_for(h, w, c):
    """All four corners, one interior tile, one with ty + c = h (at an interior column)."""
    iy, ix = (h - c) // 2, (w - c) // 2
    return [(0, 0), (0, w - c), (h - c, 0), (h - c, w - c), (iy, ix), (h - c, ix)]
