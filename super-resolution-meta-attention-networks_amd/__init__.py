"""MI355X-native SISR forward/backward engine (gfx950 HIP kernels behind the reference's model API).

Import with ``importlib.import_module("super-resolution-meta-attention-networks_amd")`` or via the
``sisr_amd`` shim at the repository root.  Sub-modules: hip (C-ABI binding), ops (autograd operators: the shared core and
the 64-channel body; its families in ops_chain, ops_sparnet, ops_sftmd, ops_attention, ops_losses, convs, pool),
architectures (drop-in nn.Modules), handlers (model-handler API), parallel (RCCL data parallelism),
metrics (PSNR), basic (SRCNN / VDSR), ensemble (x8 geometric self-ensemble for evaluation),
perceptual (VGG19 feature loss), structural (SSIM loss term), multiscale (MS-SSIM loss term),
frequency (FFT L1 loss term), consistency (degradation-consistency loss term: the output degraded again by the batch's blur
kernel against the LR input), predictor (degradation code from an LR image), corrector (IKC's correction of that code from
an SR image), pool (global mean of a map), convs (every conv of csrc/basic.hip: K x K at stride 1 and 2, Y-channel ends,
pointwise layers).
"""
from . import hip, ops, ops_chain, ops_sparnet, ops_sftmd, ops_attention, ops_losses, optim, architectures, metrics, handlers, parallel, han, san, srmd, sftmd, sparnet, basic, degrade, data, ensemble, perceptual, structural, multiscale, frequency, consistency, pool, convs, predictor, corrector, cli  # noqa: F401
from .handlers import ModelInterface, available_models  # noqa: F401
