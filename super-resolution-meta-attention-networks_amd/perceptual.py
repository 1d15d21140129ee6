"""Perceptual (VGG19 feature) training loss on the HIP path.

Mirrors
  VGGFeatureExtractor   ref: Code/SISR/models/feature_extractors/VGGNets.py:118-131 (torchvision vgg19.features[:35]:
                        sixteen 3x3 convs up to conv5_4 BEFORE its ReLU, four 2x2 max-pools, ImageNet-normalised RGB)
  PerceptualMechanism   ref: Code/sr_tools/loss_functions.py:6-22 (lambda_pixel * L1(sr, y) + lambda_per * L1(phi(sr), phi(y)))
with one intentional difference: the reference builds the extractor with a remote fetch of the published weights; here
nothing is ever fetched -- the weight file is the user's to provide (load_vgg19_weights), as torchvision publishes it or
under the reference's key names.

The extractor's parameters are frozen.  On a HIP device its forward is ops.frozen_features: the convs on the MFMA conv
kernels, the normalisation and the pools on csrc/perceptual.hip, one autograd node whose backward launches input-gradient
kernels only.  The packed weights are built when the weights are first seen on the device and kept by the module.
"""
import torch
from torch import nn

from . import ops

# torchvision's configuration "E" up to conv5_4: output channels per block, a MaxPool2d(2, 2) between blocks
VGG19_54_BLOCKS = ((64, 64), (128, 128), (256, 256, 256, 256), (512, 512, 512, 512), (512, 512, 512, 512))
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _vgg19_54_modules():
    """The first 35 children of torchvision's vgg19().features, positions included (convs at 0, 2, 5, 7, 10, ... 34)."""
    mods, cin = [], 3
    for bi, block in enumerate(VGG19_54_BLOCKS):
        if bi:
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
        for cout in block:
            mods += [nn.Conv2d(cin, cout, kernel_size=3, padding=1), nn.ReLU(inplace=False)]
            cin = cout
    return mods[:-1]  # conv5_4 is taken before its ReLU


class VGGFeatureExtractor(nn.Module):
    def __init__(self, normalise_input=True):
        super().__init__()
        self.vgg19_54 = nn.Sequential(*_vgg19_54_modules())
        assert len(self.vgg19_54) == 35
        for p in self.parameters():
            p.requires_grad_(False)
        # the reference keeps these as plain attributes: they are not part of its state dict, so not of this one either
        self.register_buffer("mean", torch.tensor(IMAGENET_MEAN).view(1, 3, 1, 1), persistent=False)
        self.register_buffer("std", torch.tensor(IMAGENET_STD).view(1, 3, 1, 1), persistent=False)
        self.normalise_input = normalise_input
        self._chain = None
        self._chain_key = None

    def conv_indices(self):
        return [i for i, m in enumerate(self.vgg19_54) if isinstance(m, nn.Conv2d)]

    def _blocks(self):
        blocks, cur = [], []
        for m in self.vgg19_54:
            if isinstance(m, nn.Conv2d):
                cur.append((m.weight, m.bias))
            elif isinstance(m, nn.MaxPool2d):
                blocks.append(cur)
                cur = []
        blocks.append(cur)
        return blocks

    def chain(self):
        """The packed device form of the weights as they are now (ops.FrozenChain).  Built on first use and again only when
        a weight has been moved or written since (load_state_dict, .to(device)): the key is every parameter's address and
        version counter -- host-side values, so looking at it is safe under stream capture."""
        key = tuple((p.data_ptr(), p._version) for p in self.parameters()) + (self.normalise_input, ops.PRECISION)
        if self._chain is None or self._chain_key != key:
            if self.mean.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("the feature extractor's weights must be packed before a hipGraph capture: run the "
                                   "criterion once eagerly first")
            self._chain = ops.FrozenChain(self._blocks(), mean=self.mean if self.normalise_input else None,
                                          std=self.std if self.normalise_input else None)
            self._chain_key = key
        return self._chain

    def forward(self, img):
        """(B, 3, H, W) RGB -> (B, 512, H / 16, W / 16) channels-last feature map."""
        if any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("VGGFeatureExtractor is a frozen feature extractor: its parameters take no gradient")
        return ops.frozen_features(img, self.chain())


def load_vgg19_weights(module, path):
    """Fill a VGGFeatureExtractor from a plain state dict on disk: torchvision's published vgg19 file as it is (keys
    `features.N.weight` / `features.N.bias`; its classifier entries are ignored) or the reference's own naming
    (`vgg19_54.N.*`).  Nothing is downloaded.  A layer that is missing or has another shape raises, naming the key."""
    state = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(state, dict):
        raise TypeError(f"{path}: expected a state dict, got {type(state).__name__}")
    with torch.no_grad():
        for i in module.conv_indices():
            conv = module.vgg19_54[i]
            for leaf, param in (("weight", conv.weight), ("bias", conv.bias)):
                names = (f"vgg19_54.{i}.{leaf}", f"features.{i}.{leaf}")
                found = [n for n in names if n in state]
                if not found:
                    raise KeyError(f"{path}: no entry {names[1]!r} (or {names[0]!r}) for VGG19 layer {i}")
                t = state[found[0]]
                if not torch.is_tensor(t) or tuple(t.shape) != tuple(param.shape):
                    got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
                    raise ValueError(f"{path}: entry {found[0]!r} has shape {got}, VGG19 layer {i} needs {tuple(param.shape)}")
                param.copy_(t.to(dtype=param.dtype))
    return module


class PerceptualMechanism(nn.Module):
    """Drop-in for handlers.L1Loss: lambda_pixel * L1(sr, y) + lambda_per * L1(phi(sr), phi(y)), phi = VGG19 conv5_4 features.
    The target's features are computed without a graph.  Capture-safe once the extractor's weights are packed (the first
    eager call does that): no host synchronisation."""

    def __init__(self, lambda_pixel=1, lambda_per=0.01, normalise_input=True):
        super().__init__()
        self.lambda_pixel = lambda_pixel
        self.lambda_per = lambda_per
        self.vgg_extractor = VGGFeatureExtractor(normalise_input=normalise_input)
        self.vgg_extractor.eval()

    def forward(self, sr, y):
        gen = self.vgg_extractor(sr)
        with torch.no_grad():
            real = self.vgg_extractor(y)
        # both maps are channels-last: seen as (B, h, w, 512) they are contiguous, and a mean over all elements is the same mean
        # Both means are rounded once: the two terms' roundings add up in the sum, and the plain l1_loss's rounded 1 / n alone
        # put this value a whole fp32 unit further from float64 than the stock stack's
        vgg_loss = ops.l1_loss(gen.permute(0, 2, 3, 1), real.permute(0, 2, 3, 1), rounded_once=True)
        return (self.lambda_pixel * ops.l1_loss(sr, y, rounded_once=True)) + (self.lambda_per * vgg_loss)
