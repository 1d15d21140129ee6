"""Degradation-consistency training loss on the HIP path.

  ConsistencyMechanism   loss = base(sr, y) + gamma * mean |D_k(sr) - lr|   on the LR pixels whose footprint lies inside the tile

The data term of blind SR (USRNet, DualSR, ZSSR, the NTIRE LR-consistency score): the output, degraded again by the kernel that
made the input, must give the input back.  The reference has no such term (its criteria are nn.L1Loss, nn.MSELoss and
PerceptualMechanism: ref sr_tools/loss_functions.py, models/__init__.py:268).  D_k is ops.degrade_valid (csrc/consistency.hip):
blur with the sample's kernel + Pillow's bicubic down-sampling as one strided correlation with the composed kernel
(degrade.compose_degradation), the float form of what OnlineDegrader does in 8 bits.  The kernels reach the batch as
'blur_kernels', the augmentation's flags as 'flips'; the handler composes K on the host and binds it, with the LR tiles,
before it calls the criterion (handlers.BaseModel.train_step / _graphed_step).  A handler builds the mechanism when its model
parameter `consistency_loss` is set (training_setup), outermost, around whatever criterion it has by then; unset, nothing
changes.  Noise and JPEG stages of the degrader are not part of D_k: they raise the floor of the term and leave its gradient
meaningful.
"""
import math

from torch import nn

from . import degrade, ops


def check_weight(gamma):
    """The model parameter: None, or a finite number >= 0 (0: no term)."""
    if gamma is None:
        return None
    if isinstance(gamma, bool) or not isinstance(gamma, (int, float)) or not (math.isfinite(gamma) and gamma >= 0):
        raise ValueError(f"consistency_loss: the weight of the degradation-consistency term must be a finite number >= 0; "
                         f"got {gamma!r}")
    return float(gamma)


class ConsistencyMechanism(nn.Module):
    """Wraps the criterion a handler had, kept as the submodule `base`: its state dict keys appear under `base.`.  No parameters
    of its own.  scale: the SR factor (2, 3 or 4); None takes it from the tiles.  The LR tiles and the composed kernels of the
    batch at hand are bound by bind() and dropped by clear(); with nothing bound (run_eval(request_loss=True): an evaluation
    batch carries no kernel) the loss is base(sr, y) alone.  Capture-safe where `base` is: two kernels, one slice copy and the
    L1 launch, no allocation outside torch's."""

    def __init__(self, base, gamma, scale=None):
        super().__init__()
        gamma = check_weight(gamma)
        if gamma is None:
            raise ValueError("consistency_loss: the weight of the degradation-consistency term must be a finite number >= 0; got None")
        if scale is not None and scale not in degrade.CONSISTENCY_SCALES:
            raise ValueError(f"consistency_loss: the degradation operator takes scales {degrade.CONSISTENCY_SCALES}; got {scale!r}")
        self.base = base
        self.gamma = gamma
        self.scale = scale
        self._bound = None

    def bind(self, lr, K):
        """lr (B, C, h, w): the network's LR input, the tiles D_k(sr) is held against; K (B, n, n) float64 on their device."""
        self._bound = (lr, K)

    def clear(self):
        self._bound = None

    def forward(self, sr, y):
        loss = self.base(sr, y)
        if self._bound is None:
            return loss
        lr, K = self._bound
        scale = self.scale if self.scale is not None else sr.shape[2] // max(lr.shape[2], 1)
        if tuple(sr.shape[:2]) != tuple(lr.shape[:2]) or sr.shape[2] != scale * lr.shape[2] or sr.shape[3] != scale * lr.shape[3]:
            raise RuntimeError(f"consistency_loss: the output {tuple(sr.shape)} is not x {scale} the LR tiles {tuple(lr.shape)}")
        _, m, _ = degrade.consistency_geometry(scale, K.shape[1])
        h, w = lr.shape[2:]
        return loss + self.gamma * ops.l1_loss(ops.degrade_valid(sr, K, scale), lr[:, :, m:h - m, m:w - m])
