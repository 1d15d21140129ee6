"""Structural (SSIM) training loss on the HIP path.

  StructuralMechanism   loss = base(sr, y) + alpha * (1 - mean SSIM(sr, y))

The reference has no such term (its criteria are nn.L1Loss, nn.MSELoss and PerceptualMechanism: ref sr_tools/loss_functions.py,
models/__init__.py:268); it is the SSIM the engine already reports as a metric (metrics.ssim, csrc/metrics.hip), turned into
a criterion: every plane of the output compared with the target's as given, float64 window statistics, value and gradient
from csrc/ssim_loss.hip (ops.ssim_mean).  A handler builds it when its model parameter `ssim_loss` is set
(handlers.BaseModel.training_setup); unset, nothing changes.
"""
import math

from torch import nn

from . import ops


class StructuralMechanism(nn.Module):
    """Wraps the criterion a handler had (handlers.L1Loss, basic.MSELoss, perceptual.PerceptualMechanism), kept as the
    submodule `base`: its state dict keys appear under `base.`.  No parameters of its own.  Capture-safe where `base` is:
    the SSIM term makes no allocation of its own beyond its outputs and no host synchronisation."""

    def __init__(self, base, alpha, data_range=1.0):
        super().__init__()
        alpha, data_range = float(alpha), float(data_range)
        if not math.isfinite(alpha) or alpha < 0:
            raise ValueError(f"ssim_loss: the weight of the structural term must be a finite number >= 0; got {alpha}")
        if not math.isfinite(data_range) or data_range <= 0:
            raise ValueError(f"ssim_data_range must be a finite number > 0; got {data_range}")
        self.base = base
        self.alpha = alpha
        self.data_range = data_range

    def forward(self, sr, y):
        return self.base(sr, y) + self.alpha * (1 - ops.ssim_mean(sr, y, self.data_range))
