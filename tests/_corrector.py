"""IKC's Corrector restated in stock torch.nn (helper module, not collected; torch only, no HIP import).  The twin is the
definition, with a real torch.cat:

    F = x;  for i in range(num_layers): F = LeakyReLU(Conv2d(c_i, nf, K, stride_i, padding=K // 2)(F))
    c = Linear(nf, nf)(LeakyReLU(Linear(M, nf)(codes)))
    t = cat([F, c broadcast over the pixels], dim=1)
    t = LeakyReLU(Conv2d(2nf, 2nf, 1)(t));  t = LeakyReLU(Conv2d(2nf, 2nf, 1)(t));  t = Conv2d(2nf, M, 1)(t)
    output = t.mean(dim=(2, 3))

`fold=True` is the same net with the code half of the first head layer applied to c alone and added as a per-image bias,
the form the HIP net runs.  It runs in float64 as the reference of the tests."""
import torch
import torch.nn.functional as F
from torch import nn

import _predictor as P

IKC_STRIDES = (1, 1, 2, 1, 2)
SITES = 8  # LeakyReLUs of the default net, in forward order: 5 convs, the code layer, 2 head layers


class Twin(nn.Module):
    def __init__(self, in_channels=3, num_codes=12, num_features=64, num_layers=5, kernel_size=5, slope=0.2, strides=None):
        super().__init__()
        nf = num_features
        strides = list(strides or (IKC_STRIDES if num_layers == 5 else [1] * num_layers))
        self.slope, self.depth, self.nf = slope, num_layers, nf
        self.layer_dict, self.code_dict, self.head_dict = nn.ModuleDict(), nn.ModuleDict(), nn.ModuleDict()
        for i in range(num_layers):
            self.layer_dict["conv_%d" % i] = nn.Conv2d(in_channels if i == 0 else nf, nf, kernel_size, stride=strides[i],
                                                       padding=kernel_size // 2)
        self.code_dict["linear_0"], self.code_dict["linear_1"] = nn.Linear(num_codes, nf), nn.Linear(nf, nf)
        for i, width in enumerate([2 * nf, 2 * nf, num_codes]):
            self.head_dict["conv_%d" % i] = nn.Conv2d(2 * nf, width, 1)

    def forward(self, x, codes, fold=False, branches=None):
        """branches (optional): per LeakyReLU site the branch to take for pre-activations inside |z| < KINK (bool maps,
        True = positive), the kink protocol of tests/_predictor.py.  -> output, or (output, elements decided that way)"""
        decided, site = 0, 0

        def act(z):
            nonlocal decided, site
            if branches is None:
                out = F.leaky_relu(z, self.slope)
            else:
                near, own = z.detach().abs() < P.KINK, z.detach() > 0
                decided += int((near & (branches[site] != own)).sum())
                out = P._LeakyAt.apply(z, self.slope, torch.where(near, branches[site], own))
            site += 1
            return out

        t = x
        for i in range(self.depth):
            t = act(self.layer_dict["conv_%d" % i](t))
        c = self.code_dict["linear_1"](act(self.code_dict["linear_0"](codes)))
        h0 = self.head_dict["conv_0"]
        if fold:
            nf = self.nf
            z = F.conv2d(t, h0.weight[:, :nf]) + (h0.bias + c @ h0.weight[:, nf:, 0, 0].t())[:, :, None, None]
        else:
            z = h0(torch.cat([t, c[:, :, None, None].expand(-1, -1, t.shape[2], t.shape[3])], dim=1))
        t = act(z)
        t = act(self.head_dict["conv_1"](t))
        out = self.head_dict["conv_2"](t).mean(dim=(2, 3))
        return out if branches is None else (out, decided)


def kaiming_state(net, seed):
    """tests/_predictor.kaiming_state for a net that also has Linear layers (2-D weights)"""
    import math
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith(".weight"):
            sd[k] = torch.randn(v.shape, generator=g) * math.sqrt(2.0 / (v.numel() // v.shape[0]))
        else:
            sd[k] = (torch.rand(v.shape, generator=g) - 0.5) * 0.2
    return sd


def twin(sd, dtype=torch.float64, **cfg):
    t = Twin(**cfg).to(dtype)
    t.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    return t


def fp32_branches(net, x, codes):
    """the branch every LeakyReLU element takes in a forward of `net` (an fp32 Twin, on the device of x), in the folded form:
    for choosing seeds on the CPU, and for the stock-torch rows of tools/corrector_bench.py"""
    out = []
    with torch.no_grad():
        t = x.float()
        for i in range(net.depth):
            z = net.layer_dict["conv_%d" % i](t)
            out.append(z > 0)
            t = F.leaky_relu(z, net.slope)
        z = net.code_dict["linear_0"](codes.float())
        out.append(z > 0)
        c = net.code_dict["linear_1"](F.leaky_relu(z, net.slope))
        h0, nf = net.head_dict["conv_0"], net.nf
        z = F.conv2d(t, h0.weight[:, :nf]) + (h0.bias + c @ h0.weight[:, nf:, 0, 0].t())[:, :, None, None]
        out.append(z > 0)
        z = net.head_dict["conv_1"](F.leaky_relu(z, net.slope))
        out.append(z > 0)
    return out


def hip_branches(ops, net, x, codes):
    """the branch every LeakyReLU of the HIP forward of a DegradationCorrector took: the same launches again, layer by layer,
    through `ops` (the package's operators, handed in: this module imports no HIP) -> (branches, output)"""
    nf, out = net.num_features, []
    with torch.no_grad():
        t = ops.nchw_to_nhwc_pad(x, cp=32)
        for i in range(net.depth):
            m = net.layer_dict["conv_%d" % i]
            t = ops.conv_kxk(t, m.weight, m.bias, slope=net.slope, stride=net.strides[i])
            out.append(t[:, :nf].cpu() > 0)
        z = net.code_dict["linear_0"](codes)
        out.append(z.cpu() > 0)
        c = net.code_dict["linear_1"](F.leaky_relu(z, net.slope))
        h = [net.head_dict["conv_%d" % i] for i in range(3)]
        t = ops.conv_1x1(t, h[0].weight[:, :nf].contiguous(), h[0].bias, slope=net.slope,
                         image_bias=c @ h[0].weight[:, nf:, 0, 0].t())
        out.append(t[:, :2 * nf].cpu() > 0)
        t = ops.conv_1x1(t, h[1].weight, h[1].bias, slope=net.slope)
        out.append(t[:, :2 * nf].cpu() > 0)
        return out, ops.map_mean(ops.conv_1x1(t, h[2].weight, h[2].bias), net.num_codes)
