"""Float64 restatements of SRCNN / VDSR and of the kernels of csrc/basic.hip (helper module, not collected; torch only, no HIP
import).  The convolutions are _exact.conv_ref's K*K shifted matmuls; gradients come from float64 autograd on them.  The
exact-data generators and the significand budget are _exact's: on such operands every correct summation order gives the
float64 result bit for bit."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import _exact as E
from conftest import GOLDEN

SIZES = [(5, 7), (9, 21), (37, 70)]  # smaller than a 9 x 9 kernel's half-width / odd, one partial tile / several ragged tiles
B = 2  # every case: two images, to catch batch strides


def pad_width(c):
    return 32 if c <= 32 else 64


# ----------------------------------------------------------------------------- the nets
def net_ref(sd, x, residual, dtype=torch.float64):
    """SRCNN (residual False) / VDSR (True) from a state dict with the reference's keys (layer_dict.conv_<i>.weight/bias):
    conv K x K, padding K // 2, ReLU after every layer but the last (ref: basic/architectures.py:47-52, :67-77)."""
    depth = len([k for k in sd if k.endswith(".weight")])
    t = x.to(dtype)
    for i in range(depth):
        w, b = sd[f"layer_dict.conv_{i}.weight"].to(dtype), sd[f"layer_dict.conv_{i}.bias"].to(dtype)
        t = F.conv2d(t, w, b, padding=w.shape[-1] // 2)
        if i != depth - 1:
            t = F.relu(t)
    return t + x.to(dtype) if residual else t


# ----------------------------------------------------------------------------- the kernels
def conv_act(x, w, bias=None, relu=False, residual=None):
    """act(conv(x, w) + bias) [+ residual], float64, differentiable"""
    y = E.conv_ref(x, w, bias)
    if relu:
        y = F.relu(y)
    return y if residual is None else y + residual.double()


def to_map(t, cp, device):
    """(B, c, H, W) -> channels-last fp32 map of cp channels on `device`, channels >= c zero"""
    b, c, h, w = t.shape
    out = torch.zeros((b, cp, h, w), dtype=torch.float32).contiguous(memory_format=torch.channels_last)
    out[:, :c] = t.float()
    return out.to(device)


def mse_ref(a, b):
    """(mean squared difference, its gradient 2 (a - b) / n) in float64"""
    d = a.double() - b.double()
    return (d * d).mean(), 2 * d / d.numel()


# ----------------------------------------------------------------------------- Y-channel images
def jpg_ycbcr(rgb):
    """(3, H, W) fp32 RGB tensor -> (3, H, W) YCbCr, full-range BT.601, written as the reference writes it
    (sr_tools/image_manipulation.py:65-75), so the fp32 roundings are the fixture's"""
    bias_c = 128. * (1 / 255)
    y = (0.299 * rgb[0, :, :] + 0.587 * rgb[1, :, :] + 0.114 * rgb[2, :, :])
    cb = bias_c + (-0.168736 * rgb[0, :, :] - 0.331264 * rgb[1, :, :] + 0.5 * rgb[2, :, :])
    cr = bias_c + (0.5 * rgb[0, :, :] - 0.418688 * rgb[1, :, :] - 0.081312 * rgb[2, :, :])
    return torch.stack([y, cb, cr], 0)


def set5_interp(scale=4):
    """[(name, x, y)]: the stored Set5 LR images PIL-bicubic-upsampled x scale (ref: evaluation/standard_eval.py:146-158) and
    their HR images, both as (1, 3, H, W) YCbCr"""
    from PIL import Image
    d = os.path.join(GOLDEN, "set5")
    out = []
    for name in sorted(f for f in os.listdir(os.path.join(d, "hr")) if f.endswith(".png")):
        lr = Image.open(os.path.join(d, "lr_random_blur", name)).convert("RGB")
        hr = Image.open(os.path.join(d, "hr", name)).convert("RGB")
        up = lr.resize((lr.width * scale, lr.height * scale), resample=Image.BICUBIC)
        pair = [jpg_ycbcr(torch.from_numpy(np.asarray(im).transpose(2, 0, 1).copy()).float().div(255))[None] for im in (up, hr)]
        out.append((name, pair[0], pair[1]))
    return out


def psnr(a, b, max_value=1.0):
    """ref: sr_tools/metrics.py psnr"""
    mse = np.mean((np.array(a, dtype=np.float32) - np.array(b, dtype=np.float32)) ** 2)
    return 100 if mse == 0 else 20 * np.log10(max_value / np.sqrt(mse))


def b4_config(tmp_path, scale=4):
    """the stored config of the reference's srcnn train_sisr run (fixture b4) with its paths filled in: the Set5 LR images
    are written PIL-bicubic-upsampled x scale to <tmp_path>/interp, which is what input = 'interp' reads"""
    import copy
    from PIL import Image
    from conftest import golden_json
    d = os.path.join(GOLDEN, "set5")
    interp = os.path.join(str(tmp_path), "interp")
    os.makedirs(interp, exist_ok=True)
    for f in sorted(os.listdir(os.path.join(d, "lr_random_blur"))):
        if f.endswith(".png"):
            lr = Image.open(os.path.join(d, "lr_random_blur", f)).convert("RGB")
            lr.resize((lr.width * scale, lr.height * scale), resample=Image.BICUBIC).save(os.path.join(interp, f))
    cfg = copy.deepcopy(golden_json("b4_train_sisr")["srcnn"]["config"])
    cfg["experiment_save_loc"] = str(tmp_path)
    for part in ("training_sets", "eval_sets"):
        for ds in cfg["data"][part].values():
            ds["lr"], ds["hr"] = interp, os.path.join(d, "hr")
    return cfg
