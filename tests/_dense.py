"""Dense-block kernels and RRDBNet: sizes, stack builders, float64 budgets and the torch.nn twins (helper module, not collected;
torch only, no HIP import).  The twins are written from the definition of the network (ESRGAN's RRDBNet as BasicSR builds it)
and are never the code under test."""
import torch
import torch.nn.functional as F
from torch import nn

import _exact as E

# (H, W).  All three dense kernels (forward, input gradient, weight gradient) tile the image 8 rows x 32 columns:
#   (1, 1) one pixel; (2, 3) smaller than the 3 x 3 kernel's halo; (9, 21) odd, one partial tile below a full one;
#   (8, 32) exactly one tile; (9, 32) one row over it; (8, 33) one column over it; (37, 70) several ragged tiles.
SIZES = [(1, 1), (2, 3), (9, 21), (8, 32), (9, 32), (8, 33), (37, 70)]
CINS = [64, 96, 128, 160]
BATCHES = [1, 2]
PITCH = 192
SENTINEL = 1234.5
CL = torch.channels_last


def stack(parts, B, H, W, device, pitch=PITCH, fill=SENTINEL):
    """channels-last (B, pitch, H, W) map on `device`: `parts` = [(first channel, (B, c, H, W) tensor)], `fill` elsewhere"""
    s = torch.full((B, pitch, H, W), fill, dtype=torch.float32).contiguous(memory_format=CL)
    for c0, t in parts:
        s[:, c0:c0 + t.shape[1]] = t
    s = s.to(device)
    assert s.is_contiguous(memory_format=CL)
    return s


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def gradient_budgets(x, w, eff, prefill, what):
    """the gradient kernels contract eff = dy or slope * dy: the same contractions on absolute values, on eff's granule"""
    ge = E.granule(eff)
    mx = E.dgrad_ref(eff.double().abs(), w.double().abs())
    if prefill is not None:
        mx = mx + prefill.double().abs()
    E.assert_budget(mx, min(ge * E.granule(w), E.granule(prefill)), what + " input gradient")
    E.assert_budget(E.wgrad_ref(x.double().abs(), eff.double().abs()), ge * E.granule(x), what + " weight gradient")
    E.assert_budget(eff.double().abs().sum(dim=(0, 2, 3)), ge, what + " bias gradient")


# ----------------------------------------------------------------------------- twins (stock torch.nn, any dtype, any device)
SLOPE = 0.2


class RDBTwin(nn.Module):
    def __init__(self, nf=64, gc=32):
        super().__init__()
        self.conv1 = nn.Conv2d(nf, gc, 3, 1, 1)
        self.conv2 = nn.Conv2d(nf + gc, gc, 3, 1, 1)
        self.conv3 = nn.Conv2d(nf + 2 * gc, gc, 3, 1, 1)
        self.conv4 = nn.Conv2d(nf + 3 * gc, gc, 3, 1, 1)
        self.conv5 = nn.Conv2d(nf + 4 * gc, nf, 3, 1, 1)
        for m in self.children():
            nn.init.kaiming_normal_(m.weight)
            m.weight.data *= 0.1
            m.bias.data.zero_()

    def forward(self, x):
        x1 = F.leaky_relu(self.conv1(x), SLOPE)
        x2 = F.leaky_relu(self.conv2(torch.cat((x, x1), 1)), SLOPE)
        x3 = F.leaky_relu(self.conv3(torch.cat((x, x1, x2), 1)), SLOPE)
        x4 = F.leaky_relu(self.conv4(torch.cat((x, x1, x2, x3), 1)), SLOPE)
        x5 = self.conv5(torch.cat((x, x1, x2, x3, x4), 1))
        return x5 * 0.2 + x


class GateTwin(nn.Module):
    """ParaCALayer(64, M): sigmoid(fc2(fc1(md))), two 1 x 1 convs (M <= 15: hidden width 32), no inner non-linearity"""

    def __init__(self, M):
        super().__init__()
        self.attribute_integrator = nn.Sequential(nn.Conv2d(M, 32, 1), nn.Conv2d(32, 64, 1), nn.Sigmoid())

    def forward(self, md):
        return self.attribute_integrator(md)


class RRDBTwin(nn.Module):
    def __init__(self, M=None):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = RDBTwin(), RDBTwin(), RDBTwin()
        if M is not None:
            self.attention_layer = GateTwin(M)

    def forward(self, x, md=None):
        out = self.rdb3(self.rdb2(self.rdb1(x)))
        if md is not None:
            out = out * self.attention_layer(md)
        return out * 0.2 + x


class RRDBNetTwin(nn.Module):
    def __init__(self, num_blocks=23, M=None, in_features=3, out_features=3):
        super().__init__()
        self.conv_first = nn.Conv2d(in_features, 64, 3, 1, 1)
        self.body = nn.Sequential(*[RRDBTwin(M) for _ in range(num_blocks)])
        self.conv_body = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_up1 = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_up2 = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_hr = nn.Conv2d(64, 64, 3, 1, 1)
        self.conv_last = nn.Conv2d(64, out_features, 3, 1, 1)

    def forward(self, x, md=None):
        feat = self.conv_first(x)
        t = feat
        for blk in self.body:
            t = blk(t, md)
        feat = feat + self.conv_body(t)
        feat = F.leaky_relu(self.conv_up1(F.interpolate(feat, scale_factor=2, mode='nearest')), SLOPE)
        feat = F.leaky_relu(self.conv_up2(F.interpolate(feat, scale_factor=2, mode='nearest')), SLOPE)
        return self.conv_last(F.leaky_relu(self.conv_hr(feat), SLOPE))


def randomise_biases(net, seed, scale=0.05):
    """the dense convs start at zero bias: draw every bias non-zero so that a dropped or misplaced bias shows"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * scale)


def as_dtype(twin_cls, sd, dtype, **cfg):
    t = twin_cls(**cfg).to(dtype)
    t.load_state_dict({k: v.detach().cpu().to(dtype) for k, v in sd.items()})
    return t


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu().flatten(), ref.detach().double().cpu().flatten()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def flat_grads(params):
    return torch.cat([p.grad.detach().double().cpu().flatten() for p in params])


def run_twin(twin, inputs, cot):
    """-> (output, input gradient, concatenated parameter gradients) of (twin(*inputs) * cot).sum(); inputs[0] is the leaf"""
    dtype = next(twin.parameters()).dtype
    x = inputs[0].detach().cpu().to(dtype).requires_grad_(True)
    rest = [t.detach().cpu().to(dtype) for t in inputs[1:]]
    out = twin(x, *rest)
    (out * cot.detach().cpu().to(dtype)).sum().backward()
    return out.detach(), x.grad.detach(), flat_grads(twin.parameters())


ACTIVATED = ("conv1", "conv2", "conv3", "conv4", "conv_up1", "conv_up2", "conv_hr")  # the convs a LeakyReLU follows
KINK_MARGIN = 1.2e-7


def smallest_preactivation(twin, inputs):
    """min |z| over every LeakyReLU input of a float64 twin's forward.  A z below fp32 resolution leaves the branch -- and with
    it a whole gradient element, 1 against 0.2 -- undecided for ANY fp32 implementation, the stock one included; with 1.3 M
    activations in a 2-block net most random cases hold one below 1e-7.  The net cases are therefore drawn (by seed) so that the
    float64 twin ALONE keeps every pre-activation KINK_MARGIN away from the kink, and the tests assert that they do."""
    found, hooks = [], []
    for name, m in twin.named_modules():
        if isinstance(m, nn.Conv2d) and name.split(".")[-1] in ACTIVATED:
            hooks.append(m.register_forward_hook(lambda mod, i, o: found.append(float(o.detach().abs().min()))))
    with torch.no_grad():
        twin(*[t.detach().cpu().double() for t in inputs])
    for h in hooks:
        h.remove()
    return min(found)


ULP = 2.0 ** -23


def assert_within_rule(hip_triplet, twin_cls, sd, inputs, cot, what, **cfg):
    """The tolerance rule of the block and net tests: for output, input gradient and concatenated parameter gradients, the
    relative L2 distance of the HIP result from the float64 twin is at most 3 x (the stock fp32 twin's distance on the CPU,
    computed here) + 2^-23.  No element is excluded.  Returns the three (hip, stock) pairs."""
    ref = run_twin(as_dtype(twin_cls, sd, torch.float64, **cfg), inputs, cot)
    stock = run_twin(as_dtype(twin_cls, sd, torch.float32, **cfg), inputs, cot)
    pairs, bad = [], []
    for name, got, st, rf in zip(("output", "input gradient", "parameter gradients"), hip_triplet, stock, ref):
        e_hip, e_stock = rel_l2(got, rf), rel_l2(st, rf)
        pairs.append((e_hip, e_stock))
        if not e_hip <= 3 * e_stock + ULP:
            bad.append("%s: hip %.3g, stock %.3g, ratio %.2f" % (name, e_hip, e_stock, e_hip / max(e_stock, 1e-300)))
    print(what, "relative L2 from float64 (hip, stock fp32):", ["%.3g / %.3g" % p for p in pairs])
    assert not bad, "%s: beyond 3 x stock + 2^-23: %s" % (what, "; ".join(bad))
    return pairs
