"""Multi-scale structural (MS-SSIM) training loss on the HIP path.

  MultiScaleStructuralMechanism   loss = base(sr, y) + alpha * (1 - mean MS-SSIM(sr, y))

The reference has no such term.  It is the "MS-SSIM + L1" family of Zhao et al. 2017: contrast and structure compared on a
pyramid of 2 x 2 means (five scales with the default weights of Wang et al. 2003), luminance on the coarsest only, so
structure far coarser than the 11-pixel window of structural.StructuralMechanism counts.  Every plane of the output is
compared with the target's as given; value and gradient come from csrc/ms_ssim.hip (ops.ms_ssim_mean), float64 throughout.
The pyramid drops a trailing odd row or column (F.avg_pool2d(t, 2)); pytorch_msssim zero-pads odd sides instead, so its
values differ on such images.  A handler builds the term when its model parameter `ms_ssim_loss` is set
(handlers.BaseModel.training_setup), with the scale weights of `ms_ssim_weights`; unset, nothing changes.
"""
import math

from torch import nn

from . import ops


class MultiScaleStructuralMechanism(nn.Module):
    """Wraps the criterion a handler had by then, kept as the submodule `base`: its state dict keys appear under `base.`.
    No parameters of its own.  Capture-safe where `base` is: the term makes no allocation of its own beyond its outputs and
    no host synchronisation.  Both image sides must be at least 11 * 2^(len(weights) - 1): 176 for the five default weights,
    88 for four."""

    def __init__(self, base, alpha, data_range=1.0, weights=ops.MS_SSIM_WEIGHTS):
        super().__init__()
        alpha, data_range = float(alpha), float(data_range)
        if not math.isfinite(alpha) or alpha < 0:
            raise ValueError(f"ms_ssim_loss: the weight of the multi-scale structural term must be a finite number >= 0; "
                             f"got {alpha}")
        if not math.isfinite(data_range) or data_range <= 0:
            raise ValueError(f"ssim_data_range must be a finite number > 0; got {data_range}")
        self.base = base
        self.alpha = alpha
        self.data_range = data_range
        self.weights = ops.ms_ssim_weights(weights)

    def forward(self, sr, y):
        return self.base(sr, y) + self.alpha * (1 - ops.ms_ssim_mean(sr, y, self.data_range, self.weights))
