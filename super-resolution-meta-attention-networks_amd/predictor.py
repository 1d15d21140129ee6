"""Degradation predictor: a small regression CNN that estimates a degradation code from an LR image, so the meta-attention
networks can run on images that come with no metadata file.

It is the Predictor of IKC (Gu et al., "Blind Super-Resolution With Iterative Kernel Correction", CVPR 2019): `num_layers`
K x K convolutions, each followed by LeakyReLU(slope) -- the last one included, as in IKC -- and a global mean over the map.
`strides` gives each layer's stride, 1 or 2: None is all ones (the net without IKC's one stride-2 layer),
[1, 1, 1, 2, 1, 1] is IKC's.  The reference tree has no counterpart.  Routing of the layers:
  input (B, in_channels, H, W)     ops.nchw_to_nhwc_pad(cp=32)   planar image -> channels-last map, channels zero-padded
  every layer                      ops.conv_kxk(slope, stride)   K x K implicit GEMM on the fp32 matrix cores, leaky forms
  output                           ops.map_mean                  (B, num_outputs) means of the last map's real channels
`layer_dict` names the layers conv_<i> as basic.SRCNN does, so state-dict keys are layer_dict.conv_<i>.weight / .bias (OIHW).
"""
import torch
from torch import nn

from . import ops
from .basic import MSELoss
from .handlers import QModel

MAX_KERNEL, MAX_WIDTH, MAX_INPUT = 9, 64, 32


class DegradationPredictor(nn.Module):
    def __init__(self, in_channels=3, num_outputs=1, num_features=64, num_layers=6, kernel_size=5, slope=0.2,
                 strides=None):
        super().__init__()
        if not 1 <= num_outputs <= MAX_WIDTH:
            raise NotImplementedError("num_outputs: the predictor estimates 1 to %d code entries (got %r); "
                                      "'unmodified_blur_kernel' with its 441 values is out of reach" % (MAX_WIDTH, num_outputs))
        if not 1 <= num_features <= MAX_WIDTH:
            raise NotImplementedError("num_features: inner widths of 1 to %d only (got %r)" % (MAX_WIDTH, num_features))
        if kernel_size % 2 == 0 or not 1 <= kernel_size <= MAX_KERNEL:
            raise NotImplementedError("kernel_size: odd kernel sizes up to %d only (got %r)" % (MAX_KERNEL, kernel_size))
        if num_layers < 2:
            raise NotImplementedError("num_layers: at least two layers (got %r)" % (num_layers,))
        if not 1 <= in_channels <= MAX_INPUT:
            raise NotImplementedError("in_channels: images of 1 to %d channels only (got %r)" % (MAX_INPUT, in_channels))
        strides = [1] * num_layers if strides is None else [int(s) for s in strides]
        if len(strides) != num_layers or any(s not in (1, 2) for s in strides):
            raise NotImplementedError("strides: one stride of 1 or 2 per layer, %d of them (got %r)" % (num_layers, strides))
        self.in_channels, self.num_outputs, self.depth, self.slope = in_channels, num_outputs, num_layers, float(slope)
        self.strides = strides
        widths = [in_channels] + [num_features] * (num_layers - 1) + [num_outputs]
        self.layer_dict = nn.ModuleDict()
        for index in range(num_layers):
            self.layer_dict['conv_{}'.format(index)] = nn.Conv2d(widths[index], widths[index + 1], kernel_size=kernel_size,
                                                                 stride=strides[index], padding=kernel_size // 2)

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("%s: this network only runs on a HIP device (no CPU fallback); got a CPU tensor"
                               % type(self).__name__)
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise RuntimeError("%s takes a %d-channel image batch (B, %d, H, W); got %s"
                               % (type(self).__name__, self.in_channels, self.in_channels, tuple(x.shape)))
        t = ops.nchw_to_nhwc_pad(x.detach(), cp=32)
        for index in range(self.depth):
            m = self.layer_dict['conv_{}'.format(index)]
            t = ops.conv_kxk(t, m.weight, m.bias, slope=self.slope, stride=self.strides[index])
        return ops.map_mean(t, self.num_outputs)

    def reset_parameters(self):
        for layer in self.layer_dict.children():
            layer.reset_parameters()


class PredictorHandler(QModel):
    """Trains / runs a DegradationPredictor from the batches a Q-model is given: the target of a step is the code
    `generate_channels` makes from the batch's metadata, the HR image is ignored.  `metadata` lists the keys it predicts."""
    predicts_metadata = True

    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, scale=None, in_features=3, num_features=64,
                 num_layers=6, kernel_size=5, slope=0.2, strides=None, scheduler=None, scheduler_params=None, perceptual=None,
                 **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        if perceptual is not None:
            raise NotImplementedError("predictor: the output is a degradation code, a perceptual loss has nothing to read")
        self.net = DegradationPredictor(in_channels=in_features, num_outputs=self.num_metadata, num_features=num_features,
                                        num_layers=num_layers, kernel_size=kernel_size, slope=slope, strides=strides)
        self.colorspace = 'rgb'
        self.im_input = 'unmodified'
        self.criterion = MSELoss()
        self.activate_device()
        self.training_setup(lr, scheduler, scheduler_params, None, device)
        self.model_name = 'predictor'

    def target_codes(self, x, metadata, metadata_keys):
        """(B, num_metadata) fp32 codes of a batch on the handler's device (style None: the values as the data set gives them)"""
        return self.generate_channels(x, metadata, metadata_keys)[:, :, 0, 0].to(self.device)

    def run_train(self, x, y, metadata=None, metadata_keys=None, extra_channels=None, tag=None, mask=None,
                  keep_on_device=False, *args, **kwargs):
        target = self.target_codes(x, metadata, metadata_keys)
        loss, out = self.train_step(x, target, tag=tag, **kwargs)
        return loss.cpu().numpy(), (out if keep_on_device else out.cpu())

    def train_step(self, x, y, metadata=None, metadata_keys=None, extra_channels=None, **kwargs):
        """y: the (B, num_metadata) target codes (run_train makes them); or the batch's metadata, from which they are made"""
        if metadata is not None:
            y = self.target_codes(x, metadata, metadata_keys)
        return super(QModel, self).train_step(x, y, **kwargs)

    def run_eval(self, x, y=None, request_loss=False, metadata=None, metadata_keys=None, extra_channels=None, *args,
                 **kwargs):
        """-> (codes (B, num_metadata), loss | None, timing).  The loss is taken against the codes of `metadata` when that
        is given and a loss is requested; `y` (an HR image) is ignored."""
        target = self.target_codes(x, metadata, metadata_keys) if (request_loss and metadata is not None) else None
        return super(QModel, self).run_eval(x, target, request_loss=request_loss, **kwargs)

    def run_model(self, x, *args, **kwargs):
        return self.net.forward(x)

    def _run_ensemble(self, x, tag, kwargs):
        raise NotImplementedError("predictor: the code describes the image as it is; there is no self-ensemble of it")
