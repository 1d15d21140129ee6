"""Frequency-domain (FFT L1) training loss on the HIP path.

  FrequencyMechanism   loss = base(sr, y) + beta * mean |rfft2(sr - y, norm='ortho')|   (real and imaginary parts apart)

The reference has no such term (its criteria are nn.L1Loss, nn.MSELoss and PerceptualMechanism: ref sr_tools/loss_functions.py,
models/__init__.py:268); it is the spectral L1 term of MIMO-UNet and of most current restoration code bases, the usual remedy
for the over-smoothed high frequencies of an L1-trained network.  Value and gradient come from csrc/freq_loss.hip
(ops.spectral_l1): the DFT as matrix products on the fp32 MFMA against cached tables, any H x W.  A handler builds it when its
model parameter `freq_loss` is set (handlers.BaseModel.training_setup), around whatever criterion it has by then; unset,
nothing changes.
"""
import math

from torch import nn

from . import ops


class FrequencyMechanism(nn.Module):
    """Wraps the criterion a handler had (handlers.L1Loss, basic.MSELoss, perceptual.PerceptualMechanism,
    structural.StructuralMechanism), kept as the submodule `base`: its state dict keys appear under `base.`.  No parameters
    of its own.  Capture-safe where `base` is, once the tables of the batch's (H, W) are cached -- the eager warm-up pass of
    the graphed step sees to that."""

    def __init__(self, base, beta):
        super().__init__()
        beta = float(beta)
        if not math.isfinite(beta) or beta < 0:
            raise ValueError(f"freq_loss: the weight of the frequency-domain term must be a finite number >= 0; got {beta}")
        self.base = base
        self.beta = beta

    def forward(self, sr, y):
        return self.base(sr, y) + self.beta * ops.spectral_l1(sr, y)
