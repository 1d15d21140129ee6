"""Model-handler / operator API of the reference, kept intact over the HIP networks.

Mirrors (names, arguments, return values, error behaviour):
  registry + ModelInterface   ref: Code/SISR/models/__init__.py:20-254
  BaseModel                   ref: Code/SISR/models/__init__.py:257-575
  QModel                      ref: Code/SISR/models/attention_manipulators/__init__.py:6-118
  EDSR/RCAN/HAN handlers      ref: Code/SISR/models/advanced/handlers.py:7-55
  QRCAN/QEDSR/QHAN handlers   ref: Code/SISR/models/attention_manipulators/handlers.py:7-76,156-171
so TrainingHandler / EvalHub style callers (train_batch, net_run_and_process, save, ...) work unchanged
and checkpoints ({'network','optimizer','model_name','model_epoch'[,'scheduler_G']}) interchange with the
reference; a handler that keeps an average of the weights (ema_decay) adds 'network_ema'.  The only intentional difference: gpu='multi' means one process per GPU + RCCL gradient
all-reduce (parallel.py) instead of single-process nn.DataParallel (ref :344-347).
"""
import contextlib
import glob
import math
import os
import time
from collections import OrderedDict

import numpy as np
import torch
from torch import nn, optim

from . import architectures as A
from . import ensemble, metrics, ops
from .metrics import batch_ms_ssim, batch_ssim, eval_output


class L1Loss(nn.Module):
    """nn.L1Loss() stand-in running the HIP loss kernel (ref: models/__init__.py:268)."""

    def forward(self, out, target):
        return ops.l1_loss(out, target)


def create_dir_if_empty(*directories):
    for d in directories:
        os.makedirs(d, exist_ok=True)  # exist_ok: every rank of a data-parallel run builds the interface


class BaseModel(nn.Module):
    def __init__(self, device, model_save_dir, eval_mode, grad_clip=None, **kwargs):
        super().__init__()
        self.criterion = L1Loss()
        self.device = torch.device('cpu') if device == 'cpu' else device
        self.optimizer = None
        self.net = None
        self.face_finder = False
        self.model_name = None
        self.im_input = None
        self.colorspace = None
        self.grad_clip = None if grad_clip == 0 else grad_clip
        self.model_save_dir = model_save_dir
        self.eval_mode = eval_mode
        self.curr_epoch = 0
        self.state = {}
        self.learning_rate_scheduler = None
        self.legacy_load = True
        self.reducer = None  # parallel.GradReducer when running data-parallel
        # hipGraph replay of forward+loss+backward for fixed-shape training batches (launch-bound regime: at
        # <= 4 tiles per GPU the ~3700 launches of an RCAN step cost more host time than GPU time)
        self.use_graph = os.environ.get("SISR_GRAPH", "0") == "1"
        self._graphs = {}
        # file of VGG19 weights for training_setup(perceptual=...); a model parameter, so it can sit in a config's internal_params
        self.perceptual_weights = kwargs.get('perceptual_weights')
        # weight of the structural term alpha * (1 - SSIM(sr, y)) added to the criterion by training_setup (None / 0: no such
        # term), and the data range of its constants; model parameters as well (no counterpart in the reference)
        self.ssim_loss = kwargs.get('ssim_loss')
        self.ssim_data_range = kwargs.get('ssim_data_range', 1.0)
        if self.ssim_loss is not None and not self.ssim_loss >= 0:
            raise ValueError("ssim_loss: the weight of the structural term must be >= 0; got %r" % (self.ssim_loss,))
        # weight of the multi-scale structural term alpha * (1 - MS-SSIM(sr, y)) added after the single-scale one (None / 0: no
        # such term) and its scale weights (None: the five of ops.MS_SSIM_WEIGHTS, images from 176 x 176); its data range
        # is ssim_data_range.  Model parameters as well (no counterpart in the reference)
        self.ms_ssim_loss = kwargs.get('ms_ssim_loss')
        self.ms_ssim_weights = kwargs.get('ms_ssim_weights')
        if self.ms_ssim_loss is not None and not (self.ms_ssim_loss >= 0 and math.isfinite(self.ms_ssim_loss)):
            raise ValueError("ms_ssim_loss: the weight of the multi-scale structural term must be a finite number >= 0; got %r"
                             % (self.ms_ssim_loss,))
        if self.ms_ssim_weights is not None:
            self.ms_ssim_weights = ops.ms_ssim_weights(self.ms_ssim_weights)
        # weight of the frequency-domain term beta * mean |rfft2(sr - y, norm='ortho')| added after the structural one (None / 0: no
        # such term); a model parameter as well (no counterpart in the reference)
        self.freq_loss = kwargs.get('freq_loss')
        if self.freq_loss is not None and not (self.freq_loss >= 0 and math.isfinite(self.freq_loss)):
            raise ValueError("freq_loss: the weight of the frequency-domain term must be a finite number >= 0; got %r"
                             % (self.freq_loss,))
        # weight of the degradation-consistency term gamma * mean |D_k(sr) - lr| added last (None / 0: no such term): the output,
        # degraded again by the blur kernel the batch carries, against the LR input (consistency.py; no counterpart in the
        # reference); a model parameter as well
        from .consistency import check_weight
        self.consistency_loss = check_weight(kwargs.get('consistency_loss'))
        self._consistency = None  # the ConsistencyMechanism training_setup wrapped the criterion in
        # the optional parts of the update step, all carried out by optim.FlatAdam in its one pass over the arenas (no
        # counterpart in the reference; model parameters, so a config's internal_params can hold them):
        #   weight_decay  decoupled (AdamW) weight decay;   ema_decay  an exponential moving average of the weights,
        #   validated on / saved as 'network_ema';   fused_clip  grad_clip on the device instead of clip_grad_norm_
        self.weight_decay = kwargs.get('weight_decay')
        self.ema_decay = kwargs.get('ema_decay')
        self.fused_clip = bool(kwargs.get('fused_clip'))
        self._averaged = False  # inside averaged_weights()
        if self.weight_decay is not None and not (self.weight_decay >= 0 and math.isfinite(self.weight_decay)):
            raise ValueError("weight_decay must be a finite number >= 0; got %r" % (self.weight_decay,))
        if self.ema_decay is not None and not 0 <= self.ema_decay < 1:
            raise ValueError("ema_decay must be in [0, 1); got %r" % (self.ema_decay,))
        if self.fused_clip and self.grad_clip is None:
            raise ValueError("fused_clip=True moves gradient clipping into the optimiser's pass, but no grad_clip is in effect")

    # -- optimiser / scheduler (ref :292-335)
    def define_optimizer(self, lr=1e-4, optimizer_params=None):
        params = [p for p in self.net.parameters() if p.requires_grad]
        betas = (optimizer_params['beta_1'], optimizer_params['beta_2']) if optimizer_params is not None else (0.9, 0.999)
        options = {}
        if self.weight_decay:
            options['weight_decay'] = self.weight_decay
        if self.ema_decay is not None:
            options['ema_decay'] = self.ema_decay
        if self.fused_clip:
            options['max_norm'] = self.grad_clip
        if params and all(p.is_cuda for p in params) and os.environ.get("SISR_FLAT_ADAM", "1") != "0":
            from .optim import FlatAdam  # one-launch Adam over a flat arena, torch.optim.Adam's schema (optim.py)
            # the meta-attention layers a network runs as ONE launch deliver their gradients at the very end of backward
            # (architectures.meta_gates); layers applied block by block (QSPARNet, the metadata-mixing styles) do not
            self.optimizer = FlatAdam(params, lr=lr, betas=betas, late=A.late_parameters(self.net), **options)
        elif options:
            why = ("SISR_FLAT_ADAM=0 selects torch.optim.Adam" if params and all(p.is_cuda for p in params)
                   else "the parameters are not on a HIP device")
            asked = ' / '.join('fused_clip' if k == 'max_norm' else k for k in options)
            raise RuntimeError("%s: %s is carried out by optim.FlatAdam's pass over its arenas, and this handler's optimiser is "
                               "not one (%s)" % (type(self).__name__, asked, why))
        else:  # CPU handlers exist for construction / checkpoint plumbing only and are never stepped
            self.optimizer = optim.Adam(params, lr=lr, betas=betas)

    def has_ema(self):
        return getattr(self.optimizer, 'flat_e', None) is not None

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the block the network holds the averaged weights (validation, export); on exit the trained ones are back,
        bit for bit.  The CONTENTS of the parameter and average arenas are exchanged, not the pointers, so captured graphs,
        ops.GRAD_SINK and every view stay valid.  Not nestable."""
        if not self.has_ema():
            raise RuntimeError("%s keeps no average of the weights (ema_decay is not set)" % type(self).__name__)
        if self._averaged:
            raise RuntimeError("averaged_weights() is already active: it cannot be nested")
        opt = self.optimizer

        def exchange():
            with torch.no_grad():
                keep = opt.flat_p.clone()
                opt.flat_p.copy_(opt.flat_e)
                opt.flat_e.copy_(keep)
            ops.invalidate_packs()
        self._averaged = True
        exchange()
        try:
            yield self
        finally:
            exchange()
            self._averaged = False

    def _averaged_state_dict(self):
        """net.state_dict() with every trained parameter replaced by its average (buffers and frozen parameters as they are)"""
        sd = self.net.state_dict()
        names = {id(p): k for k, p in self.net.named_parameters()}
        ema = self.optimizer.ema_state()
        out = OrderedDict(sd)
        for k, p in enumerate(self.optimizer.param_groups[0]['params']):
            out[names[id(p)]] = ema[k]
        return out

    def define_scheduler(self, scheduler, scheduler_params):
        if scheduler == 'cosine_annealing_warm_restarts':
            self.learning_rate_scheduler = optim.lr_scheduler.CosineAnnealingWarmRestarts(
                self.optimizer, T_mult=scheduler_params['t_mult'], T_0=scheduler_params['restart_period'],
                eta_min=scheduler_params['lr_min'])
        elif scheduler == 'multi_step_lr':
            self.learning_rate_scheduler = optim.lr_scheduler.MultiStepLR(
                self.optimizer, milestones=scheduler_params['milestones'], gamma=scheduler_params['gamma'])
        elif scheduler == 'custom_dasr':
            def dasr(epoch):
                if epoch < 60:
                    return 1e-3
                if epoch < 225:
                    return 1e-4
                return 1e-4 * math.pow(0.5, (epoch - 100) // 125)
            self.learning_rate_scheduler = optim.lr_scheduler.LambdaLR(self.optimizer, lr_lambda=dasr)
        elif scheduler == 'step_lr':
            self.learning_rate_scheduler = optim.lr_scheduler.StepLR(
                self.optimizer, step_size=scheduler_params['step_size'], gamma=scheduler_params['gamma'])
        else:
            raise RuntimeError('%s scheduler not implemented' % scheduler)

    def activate_device(self):
        self.net.to(self.device)

    def training_setup(self, lr, scheduler, scheduler_params, perceptual, device, optimizer_params=None):
        if not self.eval_mode:
            self.define_optimizer(lr=lr, optimizer_params=optimizer_params)
            if scheduler is not None:
                self.define_scheduler(scheduler=scheduler, scheduler_params=scheduler_params)
        if perceptual is not None and self.eval_mode is False:
            self.criterion = self._perceptual_criterion(perceptual)
        if self.ssim_loss is not None and self.ssim_loss != 0 and self.eval_mode is False:
            # every handler sets its criterion before it calls training_setup: whichever it is becomes the pixel term
            from . import structural
            self.criterion = structural.StructuralMechanism(self.criterion, self.ssim_loss, self.ssim_data_range)
        if self.ms_ssim_loss is not None and self.ms_ssim_loss != 0 and self.eval_mode is False:
            from . import multiscale
            self.criterion = multiscale.MultiScaleStructuralMechanism(
                self.criterion, self.ms_ssim_loss, self.ssim_data_range,
                ops.MS_SSIM_WEIGHTS if self.ms_ssim_weights is None else self.ms_ssim_weights)
        if self.freq_loss is not None and self.freq_loss != 0 and self.eval_mode is False:
            # outermost: pixel or perceptual base -> StructuralMechanism -> MultiScaleStructuralMechanism -> FrequencyMechanism
            from . import frequency
            self.criterion = frequency.FrequencyMechanism(self.criterion, self.freq_loss)
        if self.consistency_loss:
            self._check_consistency_support()
            if self.eval_mode is False:
                # outermost: ... -> FrequencyMechanism -> ConsistencyMechanism; the SR factor is read off the tiles
                from . import consistency
                self.criterion = self._consistency = consistency.ConsistencyMechanism(self.criterion, self.consistency_loss)

    def _check_consistency_support(self):
        """consistency_loss compares D_k(output) with the network's input: that input must be the LR image in RGB"""
        name = type(self).__name__
        if getattr(self, 'predicts_metadata', False):
            raise NotImplementedError("consistency_loss: %s estimates a degradation code, not an image: there is no output to "
                                      "degrade again" % name)
        if self.im_input != 'unmodified':
            raise NotImplementedError("consistency_loss: the input of %s is the interpolated image (im_input = %r), not the LR "
                                      "image the degraded output is compared with" % (name, self.im_input))
        if 'rgb' not in (self.colorspace or ''):
            raise NotImplementedError("consistency_loss: %s works in the %r colorspace; the term degrades an RGB output with the "
                                      "kernel that made the RGB LR image" % (name, self.colorspace))

    def _consistency_operands(self, x, y, kwargs):
        """None without the term; with it (lr, K): the LR tiles -- the first y.shape[1] planes of x (SRMD's x carries its metadata
        planes behind them) -- and the batch's composed kernels (B, n, n), float64 on the device, from kwargs['blur_kernels']
        (B, l, l) under kwargs['flips'] (B, 3) (absent: tiles that were not augmented)."""
        if self._consistency is None:
            return None
        from . import degrade
        kernels = kwargs.get('blur_kernels')
        k = None if kernels is None else torch.as_tensor(kernels).detach().cpu()
        if k is None or k.dim() != 3 or k.shape[0] != x.shape[0]:
            raise RuntimeError("consistency_loss: the batch carries no blur kernels ('blur_kernels' is %s): the term needs the "
                               "kernel that made each LR tile, which the online degradation loaders supply; sets degraded "
                               "offline are not supported" % ('missing' if k is None else 'of shape %s' % (tuple(k.shape),)))
        if y.shape[2] % x.shape[2] or y.shape[3] != x.shape[3] * (y.shape[2] // x.shape[2]):
            raise RuntimeError("consistency_loss: HR tiles %s are no integer multiple of the LR tiles %s"
                               % (tuple(y.shape), tuple(x.shape)))
        flips = kwargs.get('flips')
        flips = None if flips is None else torch.as_tensor(flips).detach().cpu().numpy()
        K, _ = degrade.compose_degradation(k.numpy(), y.shape[2] // x.shape[2], flips)
        K = torch.from_numpy(K)
        if x.is_cuda:  # from pinned memory, without a host synchronisation: consecutive steps keep queueing back to back
            K = K.pin_memory().to(self.device, non_blocking=True)
        return x[:, :y.shape[1]], K

    def _criterion(self, out, y, cons):
        """self.criterion(out, y) with the consistency operands bound for exactly this call"""
        if cons is None:
            return self.criterion(out, y)
        self._consistency.bind(*cons)
        try:
            return self.criterion(out, y)
        finally:
            self._consistency.clear()

    def _perceptual_criterion(self, lambda_per):
        """ref: models/__init__.py:341-342 PerceptualMechanism(lambda_per=perceptual, device=device), with the extractor's weights
        read from a local file (perceptual.load_vgg19_weights) instead of fetched.  The extractor hangs off the criterion, not
        off self.net: the optimiser, the gradient reducer, the step-level weight packing and checkpoints never see it."""
        from . import perceptual
        name = type(self).__name__
        if 'rgb' not in (self.colorspace or ''):
            raise NotImplementedError("perceptual loss: %s works in the %r colorspace, the VGG19 feature extractor reads "
                                      "three-channel RGB images" % (name, self.colorspace))
        ops._fp32_only("perceptual loss (%s)" % name)
        path = self.perceptual_weights or os.environ.get("SISR_VGG19_WEIGHTS")
        if not path:
            raise RuntimeError("perceptual loss (%s, perceptual=%r) needs a file of VGG19 weights, which is never fetched: pass "
                               "perceptual_weights=<path> to the handler (a model parameter) or set SISR_VGG19_WEIGHTS; the "
                               "file is torchvision's vgg19 state dict, or one with the reference's vgg19_54.* keys"
                               % (name, lambda_per))
        criterion = perceptual.PerceptualMechanism(lambda_per=lambda_per)
        perceptual.load_vgg19_weights(criterion.vgg_extractor, path)
        return criterion.to(self.device)

    def set_multi_gpu(self, device_ids=None, bucket_mb=None):
        """One process per GPU: gradients are averaged over the torch.distributed (RCCL) world.  bucket_mb: size of the
        all-reduce buckets (default 8, or SISR_DP_BUCKET_MB)."""
        from .parallel import GradReducer
        self.remove_multi_gpu()  # graphs captured with another reducer signal ITS progress words and write into its buckets
        self._graphs = {}
        self.reducer = GradReducer(self.net, bucket_mb=bucket_mb, arena=getattr(self.optimizer, 'grad_views', None),
                                   arena_flat=getattr(self.optimizer, 'flat_g', None),
                                   arena_offsets=getattr(self.optimizer, 'offsets', None),
                                   arena_order=getattr(self.optimizer, 'arena_order', None))

    def remove_multi_gpu(self):
        """Back to a single-process handler: the captured graphs go first (their signal nodes hold raw pointers to the reducer's
        pinned progress words), then the reducer's hooks, words and gradient sinks."""
        if self.reducer is None:
            return
        if self._graphs:
            torch.cuda.synchronize()
            self._graphs = {}
        red, self.reducer = self.reducer, None
        red.remove()
        if getattr(self.optimizer, 'grad_views', None) is not None:  # the optimiser's arena stays the gradients' home
            for p, view in self.optimizer.grad_views.items():
                ops.GRAD_SINK[p.data_ptr()] = view

    # -- checkpoints (ref :349-464)
    def save_model(self, model_save_name, model_idx, extract_state_only=False):
        if self._averaged:
            raise RuntimeError("save_model inside averaged_weights(): the network holds the averaged weights")
        self.state['network'] = self.net.state_dict()
        if self.has_ema():  # the averaged network, loadable as it is (load_model(ema=True)); absent without an average
            self.state['network_ema'] = OrderedDict((k, v.detach().clone()) for k, v in self._averaged_state_dict().items())
        self.state['optimizer'] = self.optimizer.state_dict()
        self.state['model_name'] = self.model_name
        self.state['model_epoch'] = self.curr_epoch
        if self.learning_rate_scheduler is not None:
            self.state['scheduler_G'] = self.learning_rate_scheduler.state_dict()
        if extract_state_only:
            return self.state
        torch.save(self.state, f=os.path.join(self.model_save_dir, "{}_{}".format(model_save_name, str(model_idx))))

    @staticmethod
    def legacy_switch(state_dict):
        out = OrderedDict()
        for k, v in state_dict.items():
            if k[:13] == 'model.module.':
                out[k[13:]] = v
            elif k[:6] == 'model.':
                out[k[6:]] = v
            else:
                out[k] = v
        return out

    def load_model(self, model_save_name, model_idx, legacy=False, load_override=None, preloaded_state=None, ema=False):
        """ema: load the checkpoint's averaged weights ('network_ema') as the network.  In training mode a handler that keeps
        an average restores it from the checkpoint, or starts it from the loaded weights if the checkpoint has none."""
        loc = self.device if self.device == torch.device('cpu') else "cuda:%d" % self.device
        folder = self.model_save_dir if load_override is None else load_override
        load_file = os.path.join(folder, "{}_{}".format(model_save_name, str(model_idx)))
        if preloaded_state is None:
            # checkpoints are plain tensor/number dicts: the safe loader is enough
            state = torch.load(f=load_file, map_location=loc, weights_only=True)
        else:
            state = preloaded_state
        if ema and 'network_ema' not in state:
            raise RuntimeError("%s holds no averaged weights ('network_ema'): it was saved by a run without ema_decay"
                               % load_file)
        net_state = state['network_ema'] if ema else state['network']
        net_state = self.legacy_switch(net_state) if legacy else net_state
        self.net.load_state_dict(state_dict=net_state)
        if not self.eval_mode:
            self.optimizer.load_state_dict(state['optimizer'])  # (restarts the average from the loaded weights)
            if self.has_ema() and 'network_ema' in state:
                avg = self.legacy_switch(state['network_ema']) if legacy else state['network_ema']
                names = {id(p): k for k, p in self.net.named_parameters()}
                self.optimizer.load_ema({k: avg[names[id(p)]]
                                         for k, p in enumerate(self.optimizer.param_groups[0]['params'])})
            if self.learning_rate_scheduler is not None:
                self.learning_rate_scheduler.load_state_dict(state['scheduler_G'])
        self.set_epoch(state['model_epoch'])
        if state['model_name'] == 'qpircan':
            state['model_name'] = 'qrcan'
        print('Loaded model uses the following architecture:', state['model_name'])
        return state

    # -- train / eval steps (ref :466-533)
    def train_step(self, x, y, tag=None, loss_scale=1.0, **kwargs):
        """run_train without its host round trips: returns (loss, out) as device tensors and never
        synchronises, so consecutive steps queue back to back on the stream.
        loss_scale: weight of this rank's mean loss in the data-parallel average (parallel.shard_batch sets it for
        ragged batches); 0 with an empty shard = take part in the gradient exchange and the update with zero gradients."""
        if self.eval_mode:
            raise RuntimeError('Model initialized in eval mode, training not possible.')
        self.net.train()
        x, y = x.to(device=self.device), y.to(device=self.device)
        if x.shape[0] == 0:
            self.optimizer.zero_grad()
            self._finish_update()
            nan = torch.full((), float('nan'), device=x.device)
            return nan, x.new_zeros((0,) + tuple(y.shape[1:]))
        if self.use_graph and x.is_cuda and loss_scale == 1.0:
            return self._graphed_step(x, y, kwargs)
        cons = self._consistency_operands(x, y, kwargs)
        try:
            ops.pack_all(self.net, A.conv_weights)  # every conv weight repacked by one launch
            out = self.run_model(x, image_names=tag, **kwargs)
            loss = self._criterion(out, y, cons)
            scale = loss_scale * self._dp_scale()
            self.standard_update(loss if scale == 1.0 else loss * scale)
        finally:
            ops.invalidate_packs()  # the optimiser moved the weights
        return loss.detach(), out.detach()

    def _dp_scale(self):
        """1 / world with a reducer: backward then produces this rank's share of the AVERAGE gradient, the all-reduce sums the
        shares, and nothing is left to scale between the exchange and the optimiser (GradReducer.reduce(prescaled=True))."""
        return 1.0 / self.reducer.world if self.reducer is not None else 1.0

    def _graphed_step(self, x, y, kwargs):
        """Forward + loss + backward captured once per batch shape into a hipGraph and replayed; the reducer,
        gradient clipping, Adam and the scheduler stay eager (they are a handful of launches).

        A replay writes gradients into the tensors that were the parameters' .grad at capture time, so every
        entry keeps those tensors and re-binds p.grad to them after each replay: the data-parallel join (which
        hands out bucket views as .grad) and a capture for another batch shape both re-point p.grad in between.
        With a GradReducer the captured weight-gradient kernels write straight into its buckets (ops.GRAD_SINK).  A
        replay fires no hooks; instead the capture places a signal node behind every bucket's last gradient kernel and the
        host issues each all-reduce as soon as the replay reports the bucket complete (GradReducer.launch_signalled), so the
        exchange overlaps the rest of the replayed backward as it does in eager mode.  SISR_GRAPH_OVERLAP=0 (or a CPU
        reducer): all buckets are all-reduced at the join."""
        extra = kwargs.get('extra_channels')
        cons = self._consistency_operands(x, y, kwargs)  # (LR view of x, this batch's composed kernels) or None
        key = (tuple(x.shape), tuple(y.shape), None if extra is None else tuple(extra.shape),
               None if cons is None else tuple(cons[1].shape))
        entry = self._graphs.get(key)
        red = self.reducer
        signal = red is not None and red.can_signal()
        if red is not None:
            red.hooks_enabled = False
        try:
            if entry is None:
                sx, sy = x.clone(), y.clone()
                se = None if extra is None else extra.to(self.device).clone()
                # the composed kernels live in a static buffer like sx / sy / se, refilled before every replay; the LR tiles the
                # term reads are a view of sx
                sk = None if cons is None else cons[1].clone()
                scons = None if cons is None else (sx[:, :y.shape[1]], sk)
                kw = dict(kwargs)
                if se is not None:
                    kw['extra_channels'] = se
                # The warm-up pass below is a real forward: a network with batch norms (SPARNet) would advance its running
                # statistics and step counters once more than the eager path does for this batch.  Buffers are put back after it.
                saved_buffers = [(b, b.detach().clone()) for b in self.net.buffers()]
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):  # one eager pass off the default stream: allocator + lazy-init warm-up
                    self.optimizer.zero_grad(set_to_none=True)
                    ops.pack_all(self.net, A.conv_weights)
                    with ops.deferred_wgrads():
                        (self._criterion(self.run_model(sx, **kw), sy, scons) * self._dp_scale()).backward()
                torch.cuda.current_stream().wait_stream(side)
                self.optimizer.zero_grad(set_to_none=True)
                with torch.no_grad():
                    for b, keep in saved_buffers:
                        b.copy_(keep)
                graph = torch.cuda.CUDAGraph()
                dump = os.environ.get("SISR_GRAPH_DUMP")  # diagnostic: write the captured graph as a DOT file
                if dump:
                    graph.enable_debug_mode()
                order = []
                with torch.cuda.graph(graph):
                    ops.pack_all(self.net, A.conv_weights)  # first node of the graph: the replay repacks
                    out = self.run_model(sx, **kw)
                    loss = self._criterion(out, sy, scons)
                    if signal:
                        red.begin_capture()
                    try:
                        # with signal nodes a gradient must be launched before its parameter's hook runs: nothing is deferred
                        # past the autograd node that produces it (the group nodes flush their own batches before they return)
                        with ops.deferred_wgrads(enabled=not signal):
                            (loss if red is None or red.world == 1 else loss * self._dp_scale()).backward()
                    finally:
                        if signal:
                            order = red.end_capture()
                if dump:
                    graph.debug_dump(dump)
                grads = [(p, p.grad) for p in self.net.parameters()]
                entry = (graph, sx, sy, se, loss, out, grads, order, sk)
                self._graphs[key] = entry
            graph, sx, sy, se, loss, out, grads, order, sk = entry
            sx.copy_(x)
            sy.copy_(y)
            if se is not None:
                se.copy_(extra)
            if sk is not None:
                sk.copy_(cons[1])
            graph.replay()
            for p, g in grads:  # this replay's gradients live in this entry's capture-time tensors
                p.grad = g
            if signal and order:
                red.launch_signalled(order)
        finally:
            ops.invalidate_packs()
            if red is not None:
                red.hooks_enabled = True
        if red is not None:
            red.reduce(prescaled=True)
        if self.grad_clip is not None and not self.fused_clip:  # fused: the optimiser's own pass clips (max_norm)
            nn.utils.clip_grad_norm_(self.net.parameters(), self.grad_clip)
        self.optimizer.step()
        if self.learning_rate_scheduler is not None:
            self.learning_rate_scheduler.step()
        return loss.detach().clone(), out.detach()

    def run_train(self, x, y, tag=None, mask=None, keep_on_device=False, *args, **kwargs):
        loss, out = self.train_step(x, y, tag=tag, **kwargs)
        if keep_on_device:
            return loss.cpu().numpy(), out
        return loss.cpu().numpy(), out.cpu()

    def standard_update(self, loss):
        self.optimizer.zero_grad()
        with ops.deferred_wgrads(enabled=self.reducer is None):  # with a reducer its hooks read gradients mid-backward
            loss.backward()
        self._finish_update()

    def _finish_update(self):
        if self.reducer is not None:
            self.reducer.reduce(prescaled=True)
        if self.grad_clip is not None and not self.fused_clip:  # fused: the optimiser's own pass clips (max_norm)
            nn.utils.clip_grad_norm_(self.net.parameters(), self.grad_clip)
        self.optimizer.step()
        if self.learning_rate_scheduler is not None:
            self.learning_rate_scheduler.step()

    def run_eval(self, x, y=None, request_loss=False, tag=None, timing=False, keep_on_device=False, *args,
                 self_ensemble=False, **kwargs):
        """self_ensemble: the geometric self-ensemble (the papers' "+" rows; ensemble.py) in place of the plain forward: the
        network runs on the eight flips / transposes of `x` as two batches of 4n and the outputs, mapped back, are averaged.
        `x` is what reaches the forward (concatenated metadata planes included); `extra_channels` follows it -- (B, M, 1, 1)
        vectors repeated, maps of x's size flipped along -- with its VALUES unchanged: a degradation code describes the
        un-flipped image, exact for isotropic blur codes and QPI, the protocol's usual caveat for anisotropic kernels.  The
        `timing` window holds fan, both forwards and merge; a requested loss is taken on the merged output."""
        self.net.eval()
        tic = toc = None
        with torch.no_grad():
            x = x.to(device=self.device)
            if timing:
                torch.cuda.synchronize()  # the reference times without a device sync (ref :508-512); we do sync
                tic = time.perf_counter()
            try:
                if x.is_cuda:
                    ops.pack_all(self.net, A.conv_weights)
                if self_ensemble:
                    out = self._run_ensemble(x, tag, kwargs)
                else:
                    out = self.run_model(x, image_names=tag, **kwargs)
            finally:
                ops.invalidate_packs()
            if timing:
                torch.cuda.synchronize()
                toc = time.perf_counter()
            if request_loss and y is not None:
                loss = self.criterion(out, y.to(device=self.device)).detach().cpu().numpy()
            else:
                loss = None
        if keep_on_device:
            return out.detach(), loss, toc - tic if timing else None
        return out.detach().cpu(), loss, toc - tic if timing else None

    def run_model(self, x, *args, **kwargs):
        return self.net.forward(x)

    def _run_ensemble(self, x, tag, kwargs):
        """run_model under ensemble.self_ensemble: two calls at batch 4n, each with its share of `extra_channels`"""
        kw = dict(kwargs)
        extra = kw.pop('extra_channels', None)

        def forward(t, e):
            return self.run_model(t, image_names=tag, **({} if e is None else {'extra_channels': e}), **kw)
        return ensemble.self_ensemble(forward, x, extra)

    def print_parameters(self, verbose=False):
        total = 0
        for name, value in self.named_parameters():
            if verbose:
                print(name, value.shape)
            total += np.prod(value.shape)
        return total

    def epoch_end_calls(self):
        pass

    def set_epoch(self, epoch):
        self.curr_epoch = epoch

    def get_learning_rate(self):
        return self.optimizer.param_groups[0]['lr']

    def extra_diagnostics(self):
        pass

    def pre_training_model_load(self):
        pass


class QModel(BaseModel):
    """Metadata plumbing for the meta-attention networks (host side, stays Python)."""

    def __init__(self, metadata=None, **kwargs):
        self.style = None
        self.channel_concat = False
        if metadata is not None:
            self.num_metadata = len(metadata)
            if 'all' in metadata:
                self.num_metadata += 39
            if 'blur_kernel' in metadata:
                self.num_metadata += 9
            elif 'unmodified_blur_kernel' in metadata:
                self.num_metadata += 440
            self.metadata = metadata
        else:
            self.metadata = ['qpi']
            self.num_metadata = 1
        super().__init__(**kwargs)

    def generate_channels(self, x, metadata, keys):
        """collated (B,M) metadata + list[M] of B-tuples of keys -> fp32 (B,num_metadata,1,1) on the host."""
        if metadata is None:
            raise RuntimeError('Metadata needs to be specified for this network to run properly.')
        if 'all' in self.metadata:
            mask = [True] * self.num_metadata
        else:
            mask = [key[0] in self.metadata for key in keys]
        md = torch.as_tensor(np.asarray(metadata)) if not torch.is_tensor(metadata) else metadata
        rows = []
        for index in range(x.size(0)):
            row = md[index] if len(keys) == 1 else md[index][mask]
            rows.append((torch.ones(self.num_metadata) * row).to(torch.float32))
        extra = torch.stack(rows)[:, :, None, None]
        if self.style == 'modulate':
            extra = self.scale_qpi(extra)
        return extra

    def channels_from_codes(self, codes):
        """(B, num_metadata) codes as a model estimated them (predictor.PredictorHandler) -> what generate_channels makes of
        the same values: (B, num_metadata, 1, 1) fp32, through scale_qpi for the 'modulate' style.  The tensor stays where it
        is (the 'modulate' curve is evaluated on the host, as for file metadata)."""
        if codes.dim() != 2 or codes.shape[1] != self.num_metadata:
            raise ValueError("%s takes codes of %d entries per image; got %s"
                             % (type(self).__name__, self.num_metadata, tuple(codes.shape)))
        extra = codes.detach().to(torch.float32)[:, :, None, None]
        if self.style == 'modulate':
            extra = self.scale_qpi(extra.cpu())
        return extra

    def channel_concat_logic(self, x, extra_channels, metadata, metadata_keys):
        if extra_channels is None:
            extra_channels = self.generate_channels(x, metadata, metadata_keys)
            if not self.channel_concat and self.device != extra_channels.device:
                extra_channels = extra_channels.to(self.device)
        input_data = torch.cat((x, extra_channels), 1) if self.channel_concat else x
        return input_data, extra_channels

    def run_train(self, x, y, metadata=None, extra_channels=None, metadata_keys=None, *args, **kwargs):
        input_data, extra_channels = self.channel_concat_logic(x, extra_channels, metadata, metadata_keys)
        return super().run_train(input_data, y, extra_channels=extra_channels, **kwargs)

    def train_step(self, x, y, metadata=None, extra_channels=None, metadata_keys=None, **kwargs):
        if extra_channels is None and metadata is None:
            raise RuntimeError('Metadata needs to be specified for this network to run properly.')
        if extra_channels is None:  # (callers that pass ready-made channels have also prepared the input: run_train above)
            x, extra_channels = self.channel_concat_logic(x, None, metadata, metadata_keys)
        return super().train_step(x, y, extra_channels=extra_channels, **kwargs)

    def run_eval(self, x, y=None, request_loss=False, metadata=None, metadata_keys=None, extra_channels=None, *args,
                 **kwargs):
        input_data, extra_channels = self.channel_concat_logic(x, extra_channels, metadata, metadata_keys)
        return super().run_eval(input_data, y, request_loss=request_loss, extra_channels=extra_channels, **kwargs)

    def run_model(self, x, extra_channels=None, *args, **kwargs):
        return self.net.forward(x, metadata=extra_channels)


# ----------------------------------------------------------------------------- handlers
class EDSRHandler(BaseModel):
    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, scale=4, in_features=3, hr_data_loc=None,
                 scheduler=None, scheduler_params=None, perceptual=None, num_features=64, num_blocks=16,
                 res_scale=0.1, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, hr_data_loc=hr_data_loc,
                         **kwargs)
        self.net = A.EDSR(scale=scale, in_features=in_features, net_features=num_features, num_blocks=num_blocks,
                          res_scale=res_scale)
        self.colorspace = 'rgb'
        self.im_input = 'unmodified'
        self.activate_device()
        self.training_setup(lr, scheduler, scheduler_params, perceptual, device)
        self.model_name = 'edsr'


class RCANHandler(BaseModel):
    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, scale=4, in_features=3, perceptual=None,
                 scheduler=None, scheduler_params=None, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        self.net = A.RCAN(scale=scale, in_feats=in_features)
        self.colorspace = 'rgb'
        self.im_input = 'unmodified'
        self.activate_device()
        self.training_setup(lr, scheduler, scheduler_params, perceptual, device)
        self.model_name = 'rcan'


class QRCANHandler(QModel):
    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, scale=4, in_features=3, scheduler=None,
                 scheduler_params=None, style='modulate', perceptual=None, clamp=False, min_mu=-0.2, max_mu=0.8,
                 n_feats=64, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        self.net = A.QRCAN(scale=scale, in_feats=in_features, num_metadata=self.num_metadata, n_feats=n_feats,
                           style=style, **kwargs)
        self.colorspace = 'augmented_rgb'
        self.im_input = 'unmodified'
        self.activate_device()
        self.training_setup(lr, scheduler, scheduler_params, perceptual, device)
        self.model_name = 'qrcan'
        self.min_mu = min_mu
        self.max_mu = max_mu
        self.base_scaler = np.linspace(0, 1, n_feats)
        self.clamp = clamp
        self.style = style

    @staticmethod
    def gaussian(x, mu, sig=0.2):
        return torch.from_numpy((1 / (np.sqrt(2 * np.pi) * sig)) *
                                np.exp(-np.power(x - mu, 2.) / (2 * np.power(sig, 2.)))).type(torch.float32)

    def scale_qpi(self, qpi):
        scaled = (qpi * (self.max_mu - self.min_mu)) + self.min_mu
        full = torch.stack([self.gaussian(self.base_scaler, scaled[i].squeeze().numpy())
                            for i in range(scaled.size(0))])
        if self.clamp:
            full = torch.clamp(full, 0, 1)
        return full.unsqueeze(2).unsqueeze(3)


class QEDSRHandler(QModel):
    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, scale=4, in_features=3, num_blocks=16,
                 num_features=64, res_scale=0.1, scheduler=None, scheduler_params=None, perceptual=None, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        self.net = A.QEDSR(scale=scale, in_features=in_features, num_features=num_features, num_blocks=num_blocks,
                           res_scale=res_scale, input_para=self.num_metadata, **kwargs)
        self.colorspace = 'augmented_rgb'
        self.im_input = 'unmodified'
        self.activate_device()
        self.model_name = 'qedsr'
        self.criterion = L1Loss()
        self.training_setup(lr, scheduler, scheduler_params, perceptual, device)


HANDLERS = [EDSRHandler, RCANHandler, QRCANHandler, QEDSRHandler]
try:  # HAN / QHAN are registered once their attention kernels are built (han.py)
    from .han import HANHandler, QHANHandler
    HANDLERS += [HANHandler, QHANHandler]
except ImportError:
    pass
try:  # SAN / QSAN (san.py)
    from .san import SANHandler, QSANHandler
    HANDLERS += [SANHandler, QSANHandler]
except ImportError:
    pass
try:  # SRMD (srmd.py)
    from .srmd import SRMDHandler
    HANDLERS += [SRMDHandler]
except ImportError:
    pass
try:  # SFTMD (sftmd.py)
    from .sftmd import SFTMDHandler
    HANDLERS += [SFTMDHandler]
except ImportError:
    pass
try:  # SPARNet / QSPARNet (sparnet.py)
    from .sparnet import SPARNetHandler, QSPARNetHandler
    HANDLERS += [SPARNetHandler, QSPARNetHandler]
except ImportError:
    pass
try:  # SRCNN / VDSR (basic.py)
    from .basic import SRCNNHandler, VDSRHandler
    HANDLERS += [SRCNNHandler, VDSRHandler]
except ImportError:
    pass
try:  # degradation predictor (predictor.py)
    from .predictor import PredictorHandler
    HANDLERS += [PredictorHandler]
except ImportError:
    pass
try:  # IKC's corrector (corrector.py)
    from .corrector import CorrectorHandler
    HANDLERS += [CorrectorHandler]
except ImportError:
    pass
try:  # RRDBNet / QRRDBNet: ESRGAN's generator and its meta-attention form (rrdb.py)
    from .rrdb import RRDBHandler, QRRDBHandler
    HANDLERS += [RRDBHandler, QRRDBHandler]
except ImportError:
    pass
# registry key = class name minus 'Handler', lower-cased (ref: models/__init__.py:26-30)
available_models = {h.__name__.split('Handler')[0].lower(): h for h in HANDLERS}


# ----------------------------------------------------------------------------- client façade
class ModelInterface:
    """ref: Code/SISR/models/__init__.py:33-254"""

    def __init__(self, model_loc, experiment, gpu='off', sp_gpu=0, mode='eval', new_params=None, load_epoch=None,
                 scale=None, save_subdir=None, new_branch=False, ema=False):
        """Same contract as the reference's constructor: experiment folder layout (<model_loc>/<experiment>/{result_outputs,
        saved_models}[/<save_subdir>]), parameters from `new_params` (new model) or the folder's config.toml (load_epoch given,
        a number or 'best' / 'last'), the same refusals with the same messages.  ema: load the checkpoint's averaged weights
        (a run with ema_decay stores them) as the network."""
        self.experiment, self.mode = experiment, mode
        resuming = load_epoch is not None
        self._lay_out(model_loc, experiment, save_subdir, create=mode == 'train')
        if mode == 'train' and new_params is None and not resuming:
            raise RuntimeError('Need to specify model parameters to train a new model.')
        if mode == 'eval' and not resuming:
            raise RuntimeError('Need to specify which model epoch to load.')
        self.metadata = self._stored_parameters() if resuming else new_params
        self.name = {'qpircan': 'qrcan'}.get(self.metadata['name'], self.metadata['name'])  # (a legacy spelling)
        if scale not in (None, self.metadata['internal_params']['scale']):
            raise Exception('The model loaded has been trained for a different scale, '
                            'and cannot produce the requested images.')
        self.device = sp_gpu if (gpu != 'off' and torch.cuda.is_available()) else torch.device('cpu')
        self.model = self.define_model(name=self.name, model_save_dir=self.saved_models, device=self.device,
                                       eval_mode=mode == 'eval', **self.metadata['internal_params'])
        self.model_epoch = self._epoch_number(load_epoch) if resuming else 0
        if resuming:
            self.model.load_model(model_save_name='train_model', model_idx=self.model_epoch, legacy=self.model.legacy_load,
                                  load_override=os.path.dirname(self.saved_models) if new_branch else None,
                                  **({'ema': True} if ema else {}))
        else:
            self.model.pre_training_model_load()
        self.full_name = '%s_%d' % (experiment, self.model_epoch)
        if gpu == 'multi':
            self.model.set_multi_gpu()
        self.configuration = {'input': self.model.im_input, 'colorspace': self.model.colorspace}
        self.print_overview()

    def _lay_out(self, model_loc, experiment, save_subdir, create):
        sub = (save_subdir,) if save_subdir is not None else ()
        self.base_folder = os.path.abspath(os.path.join(model_loc, experiment))
        self.logs = os.path.join(self.base_folder, 'result_outputs', *sub)
        self.saved_models = os.path.join(self.base_folder, 'saved_models', *sub)
        if create:
            create_dir_if_empty(self.base_folder, self.logs, self.saved_models)

    def _stored_parameters(self):
        if not glob.glob(os.path.join(self.base_folder, '*.toml')):
            raise RuntimeError('No config.toml in %s - model structure unknown.' % self.base_folder)
        import tomli
        with open(os.path.join(self.base_folder, 'config.toml'), 'rb') as f:
            return tomli.load(f)['model']

    def _epoch_number(self, load_epoch):
        if load_epoch not in ('best', 'last'):
            return load_epoch
        import pandas as pd
        summary = pd.read_csv(os.path.join(self.logs, 'summary.csv'))
        if getattr(self.model, 'predicts_metadata', False):  # no images, no PSNR: the lowest val-loss
            loss = summary['val-loss']
            return loss.idxmin() if load_epoch == 'best' else len(loss) - 1
        psnr = summary['val-PSNR']
        return psnr.idxmax() if load_epoch == 'best' else len(psnr) - 1

    def train_batch(self, lr, hr, **kwargs):
        return self.model.run_train(x=lr, y=hr, **kwargs)

    def set_epoch(self, epoch):
        self.model_epoch = epoch
        self.model.set_epoch(epoch)

    def net_run_and_process(self, lr=None, hr=None, **kwargs):
        if 'rgb' not in self.configuration['colorspace']:
            out_y, loss, timing = self._run_y(lr, hr, **kwargs)
            return (*self._y_to_images(out_y, lr), loss, timing)
        out_rgb, loss, timing = self.model.run_eval(x=lr, y=hr, **kwargs)
        out_ycbcr = self.colorspace_convert(out_rgb, colorspace='rgb')
        out_rgb = self._standard_image_formatting(out_rgb.numpy())
        return out_rgb, out_ycbcr, loss, timing

    def _run_y(self, lr, hr, **kwargs):
        """The Y-channel models (SRCNN / VDSR; ref: models/__init__.py:146-151): `lr` is the interpolated image in YCbCr, the
        net sees its Y channel only, the loss is taken against the reference's Y channel."""
        f_ref = hr if hr is None else hr[:, 0, :, :].unsqueeze(1)
        return self.model.run_eval(lr[:, 0, :, :].unsqueeze(1), y=f_ref, **kwargs)

    def _y_to_images(self, out_y, lr):
        """ref: models/__init__.py:152-154: the net's Y with the input's Cb / Cr -> (RGB, clipped YCbCr)."""
        out_ycbcr = torch.stack([out_y.cpu().squeeze(1), lr[:, 1, :, :].cpu(), lr[:, 2, :, :].cpu()], 1)
        out_rgb = self.colorspace_convert(out_ycbcr, colorspace='ycbcr')
        return out_rgb, self._standard_image_formatting(out_ycbcr.numpy())

    def net_run_process_and_measure(self, lr=None, hr=None, metrics=(), max_value=1, **kwargs):
        """net_run_and_process plus per-image image-quality metrics of the output against `hr`, measured where the output
        is (on the device, sisr_ssim, when the model runs on one) and outside the `timing` window.
        -> (rgb, ycbcr, loss, timing, {metric: [one value per image]}).  Measured here: 'SSIM' and 'MS-SSIM' (Y channels, data_range
        `max_value`; MS-SSIM with the five default scale weights, so images from 176 x 176); PSNR stays with the callers, on the host."""
        if 'rgb' not in self.configuration['colorspace']:
            out_y, loss, timing = self._run_y(lr, hr, keep_on_device=True, **kwargs)
            measured = {}
            if 'SSIM' in metrics:  # one-channel planes, compared as given (sisr_ssim, channels == 1)
                if hr is None:
                    raise RuntimeError('Need a reference to calculate SSIM.')
                measured['SSIM'] = batch_ssim(out_y.clamp(0, 1), hr[:, :1].to(device=out_y.device).clamp(0, 1),
                                              max_value=max_value)
            if 'MS-SSIM' in metrics:
                if hr is None:
                    raise RuntimeError('Need a reference to calculate MS-SSIM.')
                measured['MS-SSIM'] = batch_ms_ssim(out_y.clamp(0, 1), hr[:, :1].to(device=out_y.device).clamp(0, 1),
                                                    max_value=max_value)
            return (*self._y_to_images(out_y, lr), loss, timing, measured)
        out, loss, timing = self.model.run_eval(x=lr, y=hr, keep_on_device=True, **kwargs)
        measured = {}
        if 'SSIM' in metrics:
            if hr is None:
                raise RuntimeError('Need a reference to calculate SSIM.')
            measured['SSIM'] = batch_ssim(out, hr.to(device=out.device), max_value=max_value)
        if 'MS-SSIM' in metrics:
            if hr is None:
                raise RuntimeError('Need a reference to calculate MS-SSIM.')
            measured['MS-SSIM'] = batch_ms_ssim(out, hr.to(device=out.device), max_value=max_value)
        out_rgb = out.cpu()
        out_ycbcr = self.colorspace_convert(out_rgb, colorspace='rgb')
        out_rgb = self._standard_image_formatting(out_rgb.numpy())
        return out_rgb, out_ycbcr, loss, timing, measured

    def net_run_and_measure(self, lr=None, hr=None, metrics=(), max_value=1, shave=0, want_images=False, **kwargs):
        """The device output stage: the network's output stays where the model runs and only what is asked for leaves it.
        -> ({metric: [one value per image]}, loss, timing, rgb8 or None).
        metrics: any of 'PSNR' (Y-PSNR with `shave` pixels cropped from every border, metrics.eval_output), 'SSIM', 'MS-SSIM'
        (batch_ssim / batch_ms_ssim), all against `hr`, which is sent to the model's device once (a tensor already there is
        used as it is) and also serves the loss.  want_images: the (N, H, W, 3) uint8 numpy images a PNG is written from,
        made by the launch that measures PSNR.  A Y-channel model follows _run_y / _y_to_images: its one output plane against
        plane 0 of `hr`, the bytes from that plane with the Cb / Cr of `lr`, saturated where the host cast of
        net_run_and_process's RGB would wrap.  On a CPU handler everything takes the host forms of metrics.py."""
        y_model = 'rgb' not in self.configuration['colorspace']
        device = self.model.device
        on_device = device != torch.device('cpu')
        need_ref = [m for m in ('PSNR', 'SSIM', 'MS-SSIM') if m in metrics]
        if need_ref and hr is None:
            raise RuntimeError('Need a reference to calculate %s.' % need_ref[0])
        ref = hr.to(device=device) if (hr is not None and on_device) else hr
        if y_model:
            f_ref = None if ref is None else ref[:, :1].contiguous()
            out, loss, timing = self.model.run_eval(lr[:, :1].contiguous(), y=f_ref, keep_on_device=True, **kwargs)
        else:
            out, loss, timing = self.model.run_eval(x=lr, y=ref, keep_on_device=True, **kwargs)
        chroma = None
        if y_model and want_images:
            chroma = lr.to(device=out.device)
        values, rgb8 = eval_output(out, ref, chroma=chroma, max_value=max_value, shave=shave,
                                   want_psnr='PSNR' in metrics, want_rgb8=want_images, hr_form=1 if y_model else 0)
        measured = {}
        if values is not None:
            measured['PSNR'] = values
        if 'SSIM' in metrics or 'MS-SSIM' in metrics:
            a, b = (out.clamp(0, 1), f_ref.clamp(0, 1)) if y_model else (out, ref)
            if 'SSIM' in metrics:
                measured['SSIM'] = batch_ssim(a, b, max_value=max_value)
            if 'MS-SSIM' in metrics:
                measured['MS-SSIM'] = batch_ms_ssim(a, b, max_value=max_value)
        if isinstance(rgb8, torch.Tensor):
            rgb8 = rgb8.cpu().numpy()
        return measured, loss, timing, rgb8

    @staticmethod
    def colorspace_convert(image, colorspace='rgb'):
        if colorspace == 'ycbcr':
            return metrics.batch_ycbcr_to_rgb(image.numpy())
        if colorspace != 'rgb':
            raise NotImplementedError(colorspace)
        return metrics.batch_rgb_to_ycbcr(image.numpy())

    @staticmethod
    def _standard_image_formatting(im, min_value=0, max_value=1):
        return metrics.standard_image_formatting(im, min_value, max_value)

    def save(self, name='train_model', override=False, dry_run=False):
        save_path = os.path.join(self.saved_models, "{}_{}".format(name, str(self.model_epoch)))
        if os.path.isfile(save_path) and not override:
            raise RuntimeError('Saving this model will result in overwriting existing data!  '
                               'Change model location or enable override.')
        if not dry_run:
            self.model.save_model(model_save_name=name, model_idx=self.model_epoch)
        else:
            print('Training cleared to run.')

    def save_metadata(self):
        import pandas as pd
        pd.DataFrame.from_dict({'model_parameters': [self.model.print_parameters()]}).to_csv(
            os.path.join(self.base_folder, 'extra_metadata.csv'), index=False)

    def print_overview(self):
        if self.mode == 'eval':
            pmode, epoch, message = 'eval', self.model_epoch, 'currently evaluating'
        else:
            pmode, message = 'train', 'will start training from'
            epoch = self.model_epoch if self.model_epoch == 0 else self.model_epoch + 1
        print('----------------------------')
        print('Handler for experiment %s initialized successfully.' % self.experiment)
        print('System loaded in %s mode - %s architecture provided.' % (pmode, self.name))
        print('Model has %d trainable parameters.' % self.model.print_parameters())
        device = self.model.device if str(self.model.device) == 'cpu' else 'GPU ' + str(self.model.device)
        print("Using %s as the model's primary device, and %s epoch %d of the model." % (device, message, epoch))
        self.model.extra_diagnostics()
        print('----------------------------')

    @staticmethod
    def define_model(name, **kwargs):
        return available_models[name](**kwargs)

    def epoch_end_calls(self):
        self.model.epoch_end_calls()

    def get_learning_rate(self):
        return self.model.get_learning_rate()
