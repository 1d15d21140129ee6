"""The degradation predictor restated in stock torch.nn (helper module, not collected; torch only, no HIP import), and the
small experiment folders the command-line tests need.  The twin is the issue's definition, line for line:

    for i in range(num_layers): Conv2d(c_i, c_{i+1}, K, padding=K // 2); LeakyReLU(slope)
    output = map.mean(dim=(2, 3))

It runs in float64 as the reference of the tests and in fp32 where a test records what stock torch gives."""
import math
import os
import shutil

import torch
import torch.nn.functional as F
from torch import nn

from conftest import GOLDEN

KEYS = ["blur_kernel", "noise", "jpeg_quality"]  # the code of blur + noise + JPEG degradations: 10 + 1 + 1 = 12 entries
DEGRADATIONS = {"noise": True, "noise_high": 0.08, "rate_cln": 0.2, "jpeg": True, "jpeg_quality": [30, 95]}


class Twin(nn.Module):
    def __init__(self, in_channels=3, num_outputs=12, num_features=64, num_layers=6, kernel_size=5, slope=0.2):
        super().__init__()
        widths = [in_channels] + [num_features] * (num_layers - 1) + [num_outputs]
        self.slope, self.depth = slope, num_layers
        self.layer_dict = nn.ModuleDict()
        for i in range(num_layers):
            self.layer_dict["conv_%d" % i] = nn.Conv2d(widths[i], widths[i + 1], kernel_size, padding=kernel_size // 2)

    def forward(self, x):
        t = x
        for i in range(self.depth):
            t = F.leaky_relu(self.layer_dict["conv_%d" % i](t), self.slope)
        return t.mean(dim=(2, 3))


def kaiming_state(net, seed):
    """seeded Kaiming-scale weights (std sqrt(2 / fan_in), so maps keep their magnitude through the stack and the outputs are
    O(0.1 - 1)) and small biases, as an fp32 state dict with `net`'s keys"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith(".weight"):
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            sd[k] = torch.randn(v.shape, generator=g) * math.sqrt(2.0 / fan_in)
        else:
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * 0.2
    return sd


def twin64(sd, **cfg):
    t = Twin(**cfg).double()
    t.load_state_dict({k: v.double() for k, v in sd.items()})
    return t


# LeakyReLU has a kink at 0: a pre-activation z closer to 0 than the fp32 forward can resolve takes either branch, and the two
# gradients differ by (1 - slope) * dy at that element -- one such element in a 37 x 70 map moves the gradients of the layers
# below it by 1e-4 relative (measured on an MI355X: |z64| = 4.3e-7 and 8.7e-7 at the two elements that took the other branch;
# with the branch the fp32 forward took, every gradient is back within 7e-6 of float64).  Every z here is an fp32 sum of up to
# 1600 products of magnitude O(1): a few 1e-7 of rounding, and as much inherited from the layer before.  KINK is ten times
# that.  Inside |z64| < KINK the float64 reference takes the branch handed to it; everywhere else its own.
KINK = 4e-6


class _LeakyAt(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, slope, pos):
        ctx.save_for_backward(pos)
        ctx.slope = slope
        return F.leaky_relu(z, slope)

    @staticmethod
    def backward(ctx, g):
        (pos,) = ctx.saved_tensors
        return torch.where(pos, g, g * ctx.slope), None, None


def twin_forward(ref, x, branches):
    """Twin.forward in float64 where, for pre-activations inside |z| < KINK only, the LeakyReLU derivative is the branch
    `branches[i]` names (bool maps, True = the positive one).  -> (output, number of elements decided that way)"""
    t, decided = x.double(), 0
    for i in range(ref.depth):
        z = ref.layer_dict["conv_%d" % i](t)
        near = z.detach().abs() < KINK
        decided += int((near & (branches[i] != (z.detach() > 0))).sum())
        t = _LeakyAt.apply(z, ref.slope, torch.where(near, branches[i], z.detach() > 0))
    return t.mean(dim=(2, 3)), decided


def rel_l2(got, want):
    got, want = got.detach().double().cpu().reshape(-1), want.detach().double().cpu().reshape(-1)
    return float((got - want).norm() / (want.norm() + 1e-30))


def metadata_batch(B, seed):
    """A hand-made (metadata, metadata_keys) pair as a collated batch carries it: 10 kernel-code entries, the noise level, a
    'qpi' column no predictor of KEYS lists (so the key mask drops it) and the JPEG quality.  -> (metadata (B, 13) float64,
    keys, the (B, 12) values KEYS select)"""
    g = torch.Generator().manual_seed(seed)
    names = ["blur_kernel"] * 10 + ["noise", "qpi", "jpeg_quality"]
    md = torch.rand(B, len(names), generator=g, dtype=torch.float64)
    keys = [tuple(n for _ in range(B)) for n in names]
    keep = [n != "qpi" for n in names]
    return md, keys, md[:, keep].float()


def lr_folder_without_metadata(tmp_path):
    """the Set5 LR images alone (the fixture folder also holds a degradation_metadata.csv)"""
    src = os.path.join(GOLDEN, "set5", "lr_random_blur")
    dst = os.path.join(str(tmp_path), "lr_plain")
    os.makedirs(dst, exist_ok=True)
    for f in sorted(os.listdir(src)):
        if f.endswith(".png"):
            shutil.copy(os.path.join(src, f), os.path.join(dst, f))
    return dst


def train_config(tmp_path, experiment="pred", **data_extra):
    """one epoch of train_sisr on the Set5 HR images with blur + noise + JPEG drawn online: three batches of 32 x 32 LR crops"""
    hr = os.path.join(GOLDEN, "set5", "hr")
    ds = {"name": None, "lr": hr, "hr": hr, "cutoff": 5, "online_degradations": True,
          "online_degradation_params": dict(DEGRADATIONS)}
    return {"experiment": experiment, "experiment_save_loc": str(tmp_path),
            "data": {"batch_size": 2, "dataloader_threads": 0, **data_extra,
                     "training_sets": {"data_1": dict(ds, crop=32, random_augment=True)},
                     "eval_sets": {"data_1": dict(ds)}},
            "model": {"name": "predictor",
                      "internal_params": {"scale": 4, "lr": 1e-4, "metadata": list(KEYS), "num_layers": 3, "num_features": 32}},
            "training": {"gpu": "single", "sp_gpu": 0, "seed": 8, "num_epochs": 2, "metrics": ["PSNR"]}}


def save_experiment(sisr_amd, tmp_path, experiment, params, gpu):
    """a new model of `params` saved as epoch 0 of <tmp_path>/<experiment> with its config.toml, as train_sisr leaves one"""
    torch.manual_seed(8)
    mi = sisr_amd.ModelInterface(str(tmp_path), experiment, gpu="single" if gpu else "off", sp_gpu=0, mode="train",
                                 new_params=params)
    mi.save()
    sisr_amd.cli._dump_toml({"model": params}, os.path.join(mi.base_folder, "config.toml"))
    return mi
