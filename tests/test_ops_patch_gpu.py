"""Nodes that live outside ops.py launch through ops.py's core AT CALL TIME (pytest -m gpu): ops.conv_c64 and ops.wgrad_c64
are replaced by counting wrappers around the originals, as bench.py's KernelTimer and the tools replace them, and a node of
ops_chain.py and one of ops_sftmd.py must be seen making every one of their launches.  A family module that bound the
functions at import time (`from .ops import conv_c64`) would run the originals and count nothing."""
import pytest
import torch

import sisr_amd

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
DEV = "cuda:0"
CL = torch.channels_last


def _counted(run):
    """run() under counting wrappers -> (conv_c64 calls, wgrad_c64 calls); the originals are put back whatever happens"""
    conv0, wgrad0 = ops.conv_c64, ops.wgrad_c64
    calls = {"conv": 0, "wgrad": 0}

    def conv(*a, **k):
        calls["conv"] += 1
        return conv0(*a, **k)

    def wgrad(*a, **k):
        calls["wgrad"] += 1
        return wgrad0(*a, **k)

    ops.conv_c64, ops.wgrad_c64 = conv, wgrad
    try:
        run()
        torch.cuda.synchronize()
    finally:
        ops.conv_c64, ops.wgrad_c64 = conv0, wgrad0
    return calls["conv"], calls["wgrad"]


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def _map(shape, seed):
    return _rand(shape, seed).contiguous(memory_format=CL).requires_grad_(True)


def test_conv_chain_launches_through_the_patched_core():
    x = _map((1, 64, 8, 8), 1)
    layers = [(_rand((64, 64, 3, 3), 2, 0.05).requires_grad_(True), _rand((64,), 3, 0.1).requires_grad_(True), 1),
              (_rand((64, 64, 3, 3), 4, 0.05).requires_grad_(True), _rand((64,), 5, 0.1).requires_grad_(True), 0)]

    def run():
        ops.conv_chain(x, layers).backward(_rand((1, 64, 8, 8), 6).contiguous(memory_format=CL))

    assert _counted(run) == (4, 2)  # 2 forward convs + 2 input gradients; 2 weight gradients
    assert x.grad is not None and all(w.grad is not None and b.grad is not None for w, b, _ in layers)


def test_concat_sft_launches_through_the_patched_core():
    M = 4
    x = _map((1, 64, 8, 8), 11)
    md = ops.nchw_to_nhwc_pad(_rand((1, M, 8, 8), 12), 64)
    w, b = _rand((64, 64 + M, 3, 3), 13, 0.05).requires_grad_(True), _rand((64,), 14, 0.1).requires_grad_(True)

    def run():
        y = sisr_amd.ops_sftmd._ConcatSft.apply(x, md, w, b)
        y.backward(_rand((1, 64, 8, 8), 15).contiguous(memory_format=CL))

    assert _counted(run) == (2, 1)  # the 128 -> 64 conv + the feature half's input gradient; 1 weight gradient
    assert x.grad is not None and w.grad is not None and b.grad is not None
