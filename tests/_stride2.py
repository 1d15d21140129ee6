"""Stride-2 K x K convolution: float64 references and the strided predictor twin (helper module, not collected; torch only,
no HIP import).  The reference of every kernel test is torch's own float64 `F.conv2d(stride=2, padding=K // 2)` and its
autograd on the host; on the dyadic data of tests/_exact.py every sum is exact in any order, so it is THE value."""
import torch
import torch.nn.functional as F
from torch import nn

import _exact as E
import _predictor as P

# (H, W) of the conv's input.  The forward kernel's tile is 4 x 32 outputs (8 x 64 inputs), a phase of the input gradient
# is tiled 8 x 32 (16 x 64 pixels of dx):
#   (1, 1) one pixel; (2, 3) smaller than the kernel; (9, 21) odd, one partial tile; (8, 64) exactly one forward tile;
#   (9, 65) one output row / column over it; (16, 64) exactly one tile per phase of dx, two forward tiles; (17, 65) one row /
#   column over that -- and with (16, 64) an even / odd pair that shares Ho = 8 but differs in the taps its last row feeds;
#   (37, 70) several ragged tiles.
SIZES = [(1, 1), (2, 3), (9, 21), (8, 64), (9, 65), (16, 64), (17, 65), (37, 70)]
WIDTHS = [(3, 64), (64, 64), (64, 12), (48, 48)]  # (cin, cout)
IKC_STRIDES = [1, 1, 1, 2, 1, 1]


def out_size(n):
    return (n - 1) // 2 + 1


def conv_s2(x, w, b=None):
    """float64 nn.Conv2d(K, stride=2, padding=K // 2), differentiable"""
    return F.conv2d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=w.shape[-1] // 2)


def gradient_magnitudes(x, w, cot):
    """(|dx|, |dw|, |db|) bounds of the stride-2 conv's gradients: the same contractions on absolute values"""
    xa, wa = x.double().abs().requires_grad_(True), w.double().abs().requires_grad_(True)
    ba = torch.zeros(w.shape[0], dtype=torch.float64, requires_grad=True)
    conv_s2(xa, wa, ba).backward(cot.double().abs())
    return xa.grad, wa.grad, ba.grad


def assert_gradient_budgets(x, w, cot, slope, what):
    """the gradient kernels contract dy_eff in {cot, slope * cot}: magnitudes of cot (|slope| <= 1), granule of slope * cot"""
    gc = E.granule(cot) if slope is None else E.granule(cot * slope, cot)
    mx, mw, mb = gradient_magnitudes(x, w, cot)
    E.assert_budget(mx, gc * E.granule(w), what + " input gradient")
    E.assert_budget(mw, gc * E.granule(x), what + " weight gradient")
    E.assert_budget(mb, gc, what + " bias gradient")


class Twin(P.Twin):
    """tests/_predictor.Twin with a stride per layer"""

    def __init__(self, strides=None, **cfg):
        super().__init__(**cfg)
        for i, s in enumerate(strides or [1] * self.depth):
            old = self.layer_dict["conv_%d" % i]
            self.layer_dict["conv_%d" % i] = nn.Conv2d(old.in_channels, old.out_channels, old.kernel_size, stride=s,
                                                       padding=old.padding)


def twin(sd, dtype, **cfg):
    t = Twin(**cfg).to(dtype)
    t.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    return t


def layer_branches(net32, x):
    """the LeakyReLU branch (True = positive) every element of every layer takes in a stock fp32 forward of `net32`"""
    t, out = x.float(), []
    with torch.no_grad():
        for i in range(net32.depth):
            z = net32.layer_dict["conv_%d" % i](t)
            out.append(z > 0)
            t = F.leaky_relu(z, net32.slope)
    return out
