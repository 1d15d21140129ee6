"""SRCNN and VDSR: the luminance-channel baselines on the HIP path.

ref: Code/SISR/models/basic/architectures.py:6-77 (SRCNN, VDSR), basic/handlers.py:6-35 (SRCNNHandler, VDSRHandler).

Both take a bicubic-pre-upsampled Y image (B, 1, H, W) and return one of the same size.  The layers are plain K x K
convolutions with a ReLU after every layer but the last; VDSR adds its input to the result.  `layer_dict` keeps the reference's
construction order and names, so the seed-8 initial weights and the state-dict keys (layer_dict.conv_<i>.weight / .bias, OIHW)
are the reference's.  Routing of the layers:
  first layer (1 -> C)             ops.conv_y2f   VALU kernel, planar image -> channels-last map
  runs of 3 x 3, 64 -> 64 layers   ops.conv_chain the direct / Winograd MFMA kernels, ReLU masks in the input-gradient epilogues
  every other inner layer          ops.conv_kxk   K x K implicit GEMM on the fp32 matrix cores
  last layer (C -> 1)              ops.conv_f2y   channels-last map -> planar image (+ VDSR's residual)
"""
from torch import nn

from . import ops
from .handlers import BaseModel

MAX_KERNEL, MAX_WIDTH = 9, 64


class MSELoss(nn.Module):
    """nn.MSELoss() stand-in running the HIP loss kernel (ref: basic/handlers.py:14)."""

    def forward(self, out, target):
        return ops.mse_loss(out, target)


class SRCNN(nn.Module):
    """ref: basic/architectures.py:6-60.  Defaults: kernels [9, 5, 5], channels [1, 64, 32, 1]."""
    residual = False

    def __init__(self, kernel_pattern=None, channel_pattern=None, padding='same'):
        super().__init__()
        if kernel_pattern is None:
            kernel_pattern = [9, 5, 5]
        if channel_pattern is None:
            channel_pattern = [1, 64, 32, 1]
        kernel_pattern, channel_pattern = list(kernel_pattern), list(channel_pattern)
        if padding != 'same':
            raise NotImplementedError("padding: only 'same' runs on the HIP kernels (got %r)" % (padding,))
        if len(channel_pattern) != len(kernel_pattern) + 1 or len(kernel_pattern) < 2:
            raise NotImplementedError("channel_pattern must list one more entry than kernel_pattern, for at least two layers "
                                      "(got %d kernels, %d channel counts)" % (len(kernel_pattern), len(channel_pattern)))
        if any(k % 2 == 0 or k < 1 or k > MAX_KERNEL for k in kernel_pattern):
            raise NotImplementedError("kernel_pattern: odd kernel sizes up to %d only (got %s)" % (MAX_KERNEL, kernel_pattern))
        if channel_pattern[0] != 1 or channel_pattern[-1] != 1:
            raise NotImplementedError("channel_pattern must start and end at one channel, the Y image (got %s)" % channel_pattern)
        if any(c < 1 or c > MAX_WIDTH for c in channel_pattern[1:-1]):
            raise NotImplementedError("channel_pattern: inner widths of 1 to %d only (got %s)" % (MAX_WIDTH, channel_pattern))
        self.layer_dict = nn.ModuleDict()
        self.depth = len(kernel_pattern)
        for index, k in enumerate(kernel_pattern):
            self.layer_dict['conv_{}'.format(index)] = nn.Conv2d(channel_pattern[index], channel_pattern[index + 1],
                                                                 kernel_size=k, padding=k // 2)

    def plan(self):
        """[(kind, layers)] for the inner layers, kind 'chain' (a run of 3 x 3 64 -> 64 convs) or 'kxk' (one conv)."""
        convs = [self.layer_dict['conv_{}'.format(i)] for i in range(1, self.depth - 1)]

        def chained(m):
            return m.kernel_size == (3, 3) and m.in_channels == 64 and m.out_channels == 64

        steps = []
        for m in convs:
            if chained(m) and steps and steps[-1][0] == 'chain':
                steps[-1][1].append(m)
            else:
                steps.append(('chain' if chained(m) else 'kxk', [m]))
        return steps

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("%s: this network only runs on a HIP device (no CPU fallback); got a CPU tensor"
                               % type(self).__name__)
        if x.dim() != 4 or x.shape[1] != 1:
            raise RuntimeError("%s takes a one-channel (Y) image batch (B, 1, H, W); got %s" % (type(self).__name__, tuple(x.shape)))
        first, last = self.layer_dict['conv_0'], self.layer_dict['conv_{}'.format(self.depth - 1)]
        t = ops.conv_y2f(x, first.weight, first.bias, relu=True)
        for kind, layers in self.plan():
            if kind == 'chain':
                t = ops.conv_chain(t, [(m.weight, m.bias, 1) for m in layers])
            else:
                t = ops.conv_kxk(t, layers[0].weight, layers[0].bias, relu=True)
        return ops.conv_f2y(t, last.weight, last.bias, residual=x if self.residual else None)

    def reset_parameters(self):
        for layer in self.layer_dict.children():
            layer.reset_parameters()


class VDSR(SRCNN):
    """ref: basic/architectures.py:63-77: the same stack, with the input added to the result."""
    residual = True


class SRCNNHandler(BaseModel):
    """ref: basic/handlers.py:6-17"""

    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, kernel_pattern=None, channel_pattern=None,
                 padding='same', scheduler=None, scheduler_params=None, perceptual=None, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        self.net = SRCNN(kernel_pattern=kernel_pattern, channel_pattern=channel_pattern, padding=padding)
        self.colorspace = 'ycbcr'
        self.im_input = 'interp'
        self.criterion = MSELoss()
        self.activate_device()
        self.training_setup(lr, scheduler, scheduler_params, perceptual, device)
        self.model_name = 'srcnn'


class VDSRHandler(BaseModel):
    """ref: basic/handlers.py:20-35"""

    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, kernel_pattern=None, channel_pattern=None,
                 padding='same', grad_clip=0.1, scheduler=None, scheduler_params=None, perceptual=None, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, grad_clip=grad_clip, **kwargs)
        if kernel_pattern is None:
            kernel_pattern = [3] * 20
        if channel_pattern is None:
            channel_pattern = [1] + [64] * 19 + [1]
        self.net = VDSR(kernel_pattern=kernel_pattern, channel_pattern=channel_pattern, padding=padding)
        self.colorspace = 'ycbcr'
        self.im_input = 'interp'
        self.criterion = MSELoss()
        self.activate_device()
        self.training_setup(lr, scheduler, scheduler_params, perceptual, device)
        self.model_name = 'vdsr'
