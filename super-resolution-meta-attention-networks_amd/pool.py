"""Global mean of a channels-last map, both ways (csrc/basic.hip: sisr_map_mean, sisr_map_mean_bwd): the pooling at the end of
the degradation predictor (predictor.py).  ops.map_mean is this module's map_mean.  The attention gates' global_avg_pool
(64-multiples, fused into their conv launches) is another operator, in ops_attention.py."""
import torch
from torch.autograd import Function

from . import convs, hip, ops


class _MapMean(Function):
    """(B, cp, H, W) channels-last map, cp = 32 / 64 -> (B, channels) means of its real channels.  The gradient is
    materialised as a map (g / (H W) on the real channels, zero on the padded ones): the layer below reads it through its
    own activation mask, like any other dy.  No host synchronisation; the partials live in hip.workspace."""

    @staticmethod
    def forward(ctx, x, channels):
        ops._fp32_only("map_mean")
        B, cp, H, W = x.shape
        x = convs._check_map(x, "map_mean")
        if not 1 <= channels <= cp:
            raise RuntimeError(f"map_mean: {channels} real channels in a map of {cp}")
        L = hip.lib()
        hip.ptr(x)  # (refuses CPU tensors before anything touches a device)
        out = torch.empty((B, channels), device=x.device, dtype=torch.float32)
        nb = L.sisr_map_mean_workspace_bytes(B, H, W, cp)
        ws = hip.workspace(x.device, nb)
        hip.check(L.sisr_map_mean(hip.ptr(x), hip.ptr(out), B, H, W, channels, cp, hip.ptr(ws), nb, hip.stream()),
                  "sisr_map_mean")
        ctx.cfg = (B, cp, H, W, channels)
        return out

    @staticmethod
    def backward(ctx, g):
        B, cp, H, W, channels = ctx.cfg
        g = g.contiguous()
        dx = ops._empty_cl(B, cp, H, W, g.device)
        hip.check(hip.lib().sisr_map_mean_bwd(hip.ptr(g), hip.ptr(dx), B, H, W, channels, cp, hip.stream()),
                  "sisr_map_mean_bwd")
        return dx, None


def map_mean(x, channels):
    return _MapMean.apply(x, int(channels))
