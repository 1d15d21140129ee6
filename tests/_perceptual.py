"""Perceptual-loss testing (helper module, not collected; torch only, no HIP import).

A restatement of the reference's feature extractor phi (VGG19 features[:35] on ImageNet-normalised RGB: ref
feature_extractors/VGGNets.py:118-131) and of its criterion (ref sr_tools/loss_functions.py:6-22) with F.conv2d /
F.max_pool2d, in whatever dtype its operands have -- float64 for the references, float32 for the stock-torch yardstick --
and a seeded generator of weights.  The published weights are not available to the tests (and far too large for a
fixture), so the tests run on He-normal weights: randn * sqrt(2 / (9 cin)), biases uniform in +-0.05, which keep the
activations' scale through all sixteen layers and leave no output dead.
"""
import math

import torch
import torch.nn.functional as F

BLOCKS = ((64, 64), (128, 128), (256, 256, 256, 256), (512, 512, 512, 512), (512, 512, 512, 512))
CONV_INDICES = (0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def state_keys(prefix="vgg19_54"):
    return [f"{prefix}.{i}.{leaf}" for i in CONV_INDICES for leaf in ("weight", "bias")]


def shapes():
    """{conv index: (cout, cin)} -- torchvision's"""
    out, cin, it = {}, 3, iter(CONV_INDICES)
    for block in BLOCKS:
        for cout in block:
            out[next(it)] = (cout, cin)
            cin = cout
    return out


def seeded_state(seed=0, prefix="vgg19_54"):
    """fp32 state dict of the sixteen convs under `prefix` ('vgg19_54': the reference's keys, 'features': torchvision's)"""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for i, (co, ci) in shapes().items():
        sd[f"{prefix}.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * math.sqrt(2.0 / (9 * ci))
        sd[f"{prefix}.{i}.bias"] = (torch.rand(co, generator=g) * 2 - 1) * 0.05
    return sd


def phi(img, sd, prefix="vgg19_54", normalise=True):
    """features of `img` (B, 3, H, W) in img's dtype and on its device; sd: state dict as above (converted on the way)"""
    t = img
    if normalise:
        mean = torch.tensor(MEAN, dtype=torch.float32).to(img.device, img.dtype).view(1, 3, 1, 1)
        std = torch.tensor(STD, dtype=torch.float32).to(img.device, img.dtype).view(1, 3, 1, 1)
        t = (t - mean) / std
    it = iter(CONV_INDICES)
    for bi, block in enumerate(BLOCKS):
        if bi:
            t = F.max_pool2d(t, 2, 2)
        for li in range(len(block)):
            i = next(it)
            t = F.conv2d(t, sd[f"{prefix}.{i}.weight"].to(img.device, img.dtype), sd[f"{prefix}.{i}.bias"].to(img.device, img.dtype),
                         padding=1)
            if i != CONV_INDICES[-1]:
                t = F.relu(t)
    return t


def criterion(sr, y, sd, lambda_pixel=1.0, lambda_per=0.01, prefix="vgg19_54"):
    """lambda_pixel * L1(sr, y) + lambda_per * L1(phi(sr), phi(y).detach()) in sr's dtype"""
    f_sr = phi(sr, sd, prefix)
    with torch.no_grad():
        f_y = phi(y, sd, prefix)
    return lambda_pixel * (sr - y).abs().mean() + lambda_per * (f_sr - f_y).abs().mean()


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm())
