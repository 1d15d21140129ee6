"""Degradation corrector: the Corrector of IKC (Gu et al., "Blind Super-Resolution With Iterative Kernel Correction", CVPR
2019).  From an SR image and the degradation code it was made with, it estimates the correction of that code; IKC's loop is
h <- h + C(SR(lr, h), h).  The reference tree has no counterpart.

    features F   on the image (B, in_channels, sH, sW): `num_layers` K x K convs of num_features, strides 1, 1, 2, 1, 2,
                 LeakyReLU(slope) after each                                   ops.nchw_to_nhwc_pad(cp=32), ops.conv_kxk
    code c       on the code (B, M): Linear(M, nf), LeakyReLU, Linear(nf, nf)  torch, (B, nf) tensors
    head         on [F ; c at every pixel]: 1 x 1 2nf -> 2nf, LeakyReLU, 1 x 1 2nf -> 2nf, LeakyReLU, 1 x 1 2nf -> M
                                                                               ops.conv_1x1
    output       the global mean of the head's map, (B, M)                     ops.map_mean

The concatenated map [F ; c] is never built: W [F ; c] = W[:, :nf] F + W[:, nf:] c, and the second term is one vector per
image, computed on (B, nf) tensors and handed to the first head layer as its per-image bias.  The parameters keep the shapes
of the concatenated formulation (head_dict.conv_0.weight is (2nf, 2nf, 1, 1)), so a state dict is that of the plain torch.nn
net with a real torch.cat.  State-dict keys: layer_dict.conv_<i>, code_dict.linear_<i>, head_dict.conv_<i>.

CorrectorHandler (registry key 'corrector') trains the net inside IKC's loop around a frozen SR Q-model (SFTMD in IKC) and,
optionally, a frozen predictor that gives the first code; `correct` is the loop itself."""
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .basic import MSELoss
from .handlers import QModel
from .predictor import MAX_INPUT, MAX_KERNEL, MAX_WIDTH

IKC_STRIDES = (1, 1, 2, 1, 2)


class DegradationCorrector(nn.Module):
    def __init__(self, in_channels=3, num_codes=1, num_features=64, num_layers=5, kernel_size=5, slope=0.2, strides=None):
        super().__init__()
        if not 1 <= num_codes <= MAX_WIDTH:
            raise NotImplementedError("num_codes: the corrector takes codes of 1 to %d entries (got %r); "
                                      "'unmodified_blur_kernel' with its 441 values is out of reach" % (MAX_WIDTH, num_codes))
        if not 1 <= num_features <= MAX_WIDTH:
            raise NotImplementedError("num_features: inner widths of 1 to %d only (got %r)" % (MAX_WIDTH, num_features))
        if kernel_size % 2 == 0 or not 1 <= kernel_size <= MAX_KERNEL:
            raise NotImplementedError("kernel_size: odd kernel sizes up to %d only (got %r)" % (MAX_KERNEL, kernel_size))
        if num_layers < 1:
            raise NotImplementedError("num_layers: at least one layer (got %r)" % (num_layers,))
        if not 1 <= in_channels <= MAX_INPUT:
            raise NotImplementedError("in_channels: images of 1 to %d channels only (got %r)" % (MAX_INPUT, in_channels))
        if strides is None:
            strides = IKC_STRIDES if num_layers == len(IKC_STRIDES) else [1] * num_layers
        strides = [int(s) for s in strides]
        if len(strides) != num_layers or any(s not in (1, 2) for s in strides):
            raise NotImplementedError("strides: one stride of 1 or 2 per layer, %d of them (got %r)" % (num_layers, strides))
        nf = num_features
        self.in_channels, self.num_codes, self.num_features, self.depth = in_channels, num_codes, nf, num_layers
        self.slope, self.strides = float(slope), strides
        self.layer_dict, self.code_dict, self.head_dict = nn.ModuleDict(), nn.ModuleDict(), nn.ModuleDict()
        for index in range(num_layers):
            self.layer_dict['conv_{}'.format(index)] = nn.Conv2d(in_channels if index == 0 else nf, nf, kernel_size=kernel_size,
                                                                 stride=strides[index], padding=kernel_size // 2)
        self.code_dict['linear_0'] = nn.Linear(num_codes, nf)
        self.code_dict['linear_1'] = nn.Linear(nf, nf)
        for index, width in enumerate([2 * nf, 2 * nf, num_codes]):
            self.head_dict['conv_{}'.format(index)] = nn.Conv2d(2 * nf, width, kernel_size=1)

    def forward(self, x, codes):
        name = type(self).__name__
        if not (x.is_cuda and codes.is_cuda):
            raise RuntimeError("%s: this network only runs on a HIP device (no CPU fallback); got a CPU tensor" % name)
        if x.dim() != 4 or x.shape[1] != self.in_channels:
            raise RuntimeError("%s takes a %d-channel image batch (B, %d, H, W); got %s"
                               % (name, self.in_channels, self.in_channels, tuple(x.shape)))
        if tuple(codes.shape) != (x.shape[0], self.num_codes):
            raise RuntimeError("%s takes one code of %d entries per image, (%d, %d); got %s"
                               % (name, self.num_codes, x.shape[0], self.num_codes, tuple(codes.shape)))
        nf = self.num_features
        t = ops.nchw_to_nhwc_pad(x.detach(), cp=32)
        for index in range(self.depth):
            m = self.layer_dict['conv_{}'.format(index)]
            t = ops.conv_kxk(t, m.weight, m.bias, slope=self.slope, stride=self.strides[index])
        c = self.code_dict['linear_1'](F.leaky_relu(self.code_dict['linear_0'](codes), self.slope))
        head = [self.head_dict['conv_{}'.format(index)] for index in range(3)]
        w0 = head[0].weight
        image_bias = c @ w0[:, nf:, 0, 0].t()  # the code half of the first head layer: one vector per image
        t = ops.conv_1x1(t, w0[:, :nf].contiguous(), head[0].bias, slope=self.slope, image_bias=image_bias)
        t = ops.conv_1x1(t, head[1].weight, head[1].bias, slope=self.slope)
        t = ops.conv_1x1(t, head[2].weight, head[2].bias)
        return ops.map_mean(t, self.num_codes)

    def reset_parameters(self):
        for group in (self.layer_dict, self.code_dict, self.head_dict):
            for layer in group.children():
                layer.reset_parameters()


class CorrectorHandler(QModel):
    """Trains / runs a DegradationCorrector in IKC's loop  h <- h + C(SR(lr, h), h).  Internal params beside the net's:
      sr_model = [experiment, epoch]   the SR network: any Q-model whose `metadata` list equals this handler's, loaded frozen
                                       in eval mode from `model_loc` (default: the folder this experiment lies in);
      predictor = [experiment, epoch]  optional, frozen: the first code; without it the loop starts from the mean code 0.5;
      iterations                       steps of the loop (7).
    A train batch takes one optimiser step per iteration on MSE(h + C(sr, h), h*), h* the batch's true code; the code that
    enters a step is the detached result of the one before.  Each iteration copies nothing to the host for a Q-model that
    takes `extra_channels`; SRMD / SFTMD build their maps from host metadata, one (B, M) copy per iteration."""
    predicts_metadata = True

    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, scale=None, in_features=3, num_features=64,
                 num_layers=5, kernel_size=5, slope=0.2, strides=None, sr_model=None, predictor=None, iterations=7,
                 model_loc=None, scheduler=None, scheduler_params=None, perceptual=None, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        if perceptual is not None:
            raise NotImplementedError("corrector: the output is a degradation code, a perceptual loss has nothing to read")
        if sr_model is None:
            raise ValueError("corrector: sr_model = [experiment, epoch] names the SR network of the loop and is required")
        if int(iterations) < 1:
            raise ValueError("corrector: iterations must be at least 1 (got %r)" % (iterations,))
        self.iterations = int(iterations)
        self.net = DegradationCorrector(in_channels=in_features, num_codes=self.num_metadata, num_features=num_features,
                                        num_layers=num_layers, kernel_size=kernel_size, slope=slope, strides=strides)
        self.colorspace = 'rgb'
        self.im_input = 'unmodified'
        self.criterion = MSELoss()
        self.activate_device()
        self.training_setup(lr, scheduler, scheduler_params, None, device)
        self.model_name = 'corrector'
        loc = model_loc if model_loc is not None else os.path.dirname(os.path.dirname(os.path.abspath(model_save_dir)))
        # (plain attributes of a dict: the frozen models are no sub-modules, their weights are not this handler's to save)
        self.frozen = {'sr_model': self._load_frozen(loc, 'sr_model', sr_model),
                       'predictor': self._load_frozen(loc, 'predictor', predictor) if predictor else None}
        if self.frozen['predictor'] is not None and not getattr(self.frozen['predictor'].model, 'predicts_metadata', False):
            raise ValueError("corrector: predictor: experiment %r holds a %r model, which predicts no degradation code"
                             % (predictor[0], self.frozen['predictor'].name))

    def _load_frozen(self, loc, what, key):
        from .handlers import ModelInterface
        name, ep = key
        on_gpu = self.device != torch.device('cpu')
        model = ModelInterface(loc, name, gpu='single' if on_gpu else 'off', sp_gpu=self.device if on_gpu else 0, mode='eval',
                               load_epoch=ep if ep in ('best', 'last') else int(ep))
        if not isinstance(model.model, QModel):
            raise ValueError("corrector: %s: experiment %r holds a %r model, which reads no degradation code"
                             % (what, name, model.name))
        if list(model.model.metadata) != list(self.metadata):
            raise ValueError("corrector: %s %r reads the metadata %s, the corrector corrects %s; the two lists must be the same, "
                             "in the same order" % (what, name, list(model.model.metadata), list(self.metadata)))
        for p in model.model.parameters():
            p.requires_grad_(False)
        return model

    def target_codes(self, x, metadata, metadata_keys):
        """(B, num_metadata) fp32 codes of a batch on the handler's device (style None: the values as the data set gives them)"""
        return self.generate_channels(x, metadata, metadata_keys)[:, :, 0, 0].to(self.device)

    def initial_codes(self, lr):
        """the code the loop starts from: the frozen predictor's, or the mean code 0.5 (generate_channels normalises to [0, 1])"""
        if self.frozen['predictor'] is not None:
            return self.frozen['predictor'].model.run_eval(lr, keep_on_device=True)[0].to(self.device)
        return torch.full((lr.shape[0], self.num_metadata), 0.5, device=self.device)

    def super_resolve(self, lr, codes):
        """the frozen SR model on `lr` with `codes` (B, M) as its metadata, under no_grad; the image stays on the device"""
        from .cli import _with_predicted_codes
        handler = self.frozen['sr_model'].model
        feed = _with_predicted_codes(handler, self, {'lr': lr}, codes)
        return handler.run_eval(feed.pop('lr'), keep_on_device=True, **feed)[0].to(self.device)

    def run_model(self, x, extra_channels=None, *args, **kwargs):
        """x: the SR image, extra_channels: the (B, M) code it was made with -> the corrected code h + C(x, h)"""
        return extra_channels + self.net.forward(x, extra_channels)

    def correct(self, lr, codes=None, iterations=None, want_sr=True):
        """IKC's loop on an LR batch -> (SR image made with the final codes | None, final codes, [codes per iteration]),
        entry 0 of the list being the codes the loop started from (`codes`, or initial_codes(lr))."""
        self.net.eval()
        with torch.no_grad():
            lr = lr.to(self.device)
            h = self.initial_codes(lr) if codes is None else codes.detach().to(self.device, torch.float32)
            history = [h]
            for _ in range(self.iterations if iterations is None else int(iterations)):
                h = self.run_model(self.super_resolve(lr, h), extra_channels=h)
                history.append(h)
            return (self.super_resolve(lr, h) if want_sr else None), h, history

    def run_train(self, x, y, metadata=None, metadata_keys=None, extra_channels=None, tag=None, mask=None,
                  keep_on_device=False, *args, **kwargs):
        target = self.target_codes(x, metadata, metadata_keys)
        lr = x.to(self.device)
        h = self.initial_codes(lr)
        for _ in range(self.iterations):
            loss, h = self.train_step(self.super_resolve(lr, h), target, extra_channels=h, tag=tag, **kwargs)
        return loss.cpu().numpy(), (h if keep_on_device else h.cpu())

    def train_step(self, x, y, metadata=None, metadata_keys=None, extra_channels=None, **kwargs):
        """one optimiser step: x the SR image, extra_channels the code it was made with, y the (B, M) target codes"""
        if extra_channels is None:
            raise RuntimeError("corrector: a step takes the SR image and, as extra_channels, the code it was made with")
        return super(QModel, self).train_step(x, y, extra_channels=extra_channels.detach(), **kwargs)

    def run_eval(self, x, y=None, request_loss=False, metadata=None, metadata_keys=None, extra_channels=None,
                 keep_on_device=False, *args, **kwargs):
        """-> (final codes of the loop on the LR batch x, loss | None, None).  extra_channels: the codes to start from.  The
        loss is taken against the codes of `metadata` when that is given and a loss is requested; `y` is ignored."""
        _, codes, _ = self.correct(x, extra_channels, want_sr=False)
        loss = None
        if request_loss and metadata is not None:
            with torch.no_grad():
                loss = self.criterion(codes, self.target_codes(x, metadata, metadata_keys)).detach().cpu().numpy()
        return (codes if keep_on_device else codes.cpu()), loss, None

    def _run_ensemble(self, x, tag, kwargs):
        raise NotImplementedError("corrector: the code describes the image as it is; there is no self-ensemble of it")
