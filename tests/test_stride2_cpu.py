"""Stride-2 K x K conv: what can be checked without a GPU -- the refusals of the new entry points, the output-size helper,
the argument checks of ops.conv_kxk and the predictor's `strides` parameter."""
import ctypes as C

import pytest
import torch
from torch import nn

import _predictor as P
import _stride2 as S
import sisr_amd

ARG, ALIGN, UNSUPPORTED = -1, -2, -4


def _buf():
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    assert a % 16 == 0
    return buf, a


def test_stride2_entry_points_refuse_bad_arguments_before_any_device_call():
    L = sisr_amd.hip.lib()
    buf, a = _buf()
    nan, inf = float("nan"), float("inf")

    def fwd(x=a, packed=a, K=5, cin_p=64, cout_p=64, slope=0.2, nbias=64, B=1):
        return L.sisr_convk_s2_mfma_leaky(x, packed, a, nbias, a, B, 8, 8, K, cin_p, cout_p, 1, slope, None)

    assert fwd(x=None) == ARG and fwd(packed=None) == ARG and fwd(B=0) == ARG
    assert fwd(slope=nan) == ARG and fwd(slope=inf) == ARG
    assert fwd(K=4) == UNSUPPORTED and fwd(K=11) == UNSUPPORTED
    assert fwd(cin_p=48) == UNSUPPORTED and fwd(cout_p=48) == UNSUPPORTED and fwd(cout_p=128) == UNSUPPORTED
    assert fwd(cout_p=32, nbias=33) == UNSUPPORTED
    assert fwd(x=a + 4) == ALIGN and fwd(packed=a + 4) == ALIGN

    def dgrad(dy=a, mask=a, packed=a, dx=a, K=5, cout_p=64, cin_p=64, slope=0.2, H=8):
        return L.sisr_dgradk_s2_mfma_leaky(dy, mask, packed, dx, 1, H, 8, K, cout_p, cin_p, slope, None)

    assert dgrad(dy=None) == ARG and dgrad(packed=None) == ARG and dgrad(dx=None) == ARG and dgrad(H=0) == ARG
    assert dgrad(slope=nan) == ARG
    assert dgrad(K=2) == UNSUPPORTED and dgrad(cin_p=48) == UNSUPPORTED and dgrad(cout_p=128) == UNSUPPORTED
    assert dgrad(dy=a + 4) == ALIGN and dgrad(mask=a + 4) == ALIGN and dgrad(packed=a + 4) == ALIGN

    def wgrad(x=a, K=5, cop=64, cip=64, cout=64, slope=0.2, nbytes=1 << 30):
        return L.sisr_wgradk_s2_mfma_leaky(x, a, a, a, a, 1, 8, 8, K, cout, 64, cop, cip, a, nbytes, slope, None)

    assert wgrad(x=None) == ARG and wgrad(slope=nan) == ARG and wgrad(cout=0) == ARG
    assert wgrad(nbytes=16) == ARG  # workspace too small
    assert wgrad(K=4) == UNSUPPORTED and wgrad(cip=48) == UNSUPPORTED and wgrad(cop=128) == UNSUPPORTED
    assert wgrad(cop=32, cout=33) == UNSUPPORTED
    assert L.sisr_wgradk_s2_mfma_workspace_bytes(1, 8, 8, 4, 64, 64) == 0
    assert L.sisr_wgradk_s2_mfma_workspace_bytes(1, 8, 8, 5, 64, 128) == 0
    # 8 x 8 input -> 4 output rows: one slice of 64 x 64 x 25 partial weights, then the bias partials
    assert L.sisr_wgradk_s2_mfma_workspace_bytes(1, 8, 8, 5, 64, 64) == 4 * (64 * 64 * 25 + 1024 * 64)
    # the slices follow dy's rows, not x's: 2 x 37 input rows are 38 output rows -> 10 slices; the stride-1 form has 15
    assert L.sisr_wgradk_s2_mfma_workspace_bytes(2, 37, 70, 5, 64, 64) == 4 * (10 * 64 * 64 * 25 + 1024 * 64)
    assert L.sisr_wgradk_mfma_workspace_bytes(2, 37, 70, 5, 64, 64) == 4 * (15 * 64 * 64 * 25 + 1024 * 64)


@pytest.mark.parametrize("K", [1, 3, 5, 7, 9])
def test_output_size_helper_agrees_with_conv2d(K):
    conv = nn.Conv2d(1, 1, K, stride=2, padding=K // 2)
    for n in range(1, 21):
        want = conv(torch.zeros(1, 1, n, 21 - n)).shape
        got = (sisr_amd.ops.conv_s2_out_size(n), sisr_amd.ops.conv_s2_out_size(21 - n))
        assert got == tuple(want[2:]) == (S.out_size(n), S.out_size(21 - n)), (n, K)
    assert sisr_amd.ops.conv_s2_out_size(0) == 0


def test_conv_kxk_refuses_relu_at_stride_2_and_other_strides():
    x, w = torch.zeros(1, 32, 4, 4), torch.zeros(32, 32, 3, 3)
    with pytest.raises(ValueError, match="LeakyReLU family only"):
        sisr_amd.ops.conv_kxk(x, w, None, relu=True, stride=2)
    for stride in (0, 3, 4, (2, 2)):
        with pytest.raises(ValueError, match="strides 1 and 2 only"):
            sisr_amd.ops.conv_kxk(x, w, None, slope=0.2, stride=stride)


def test_predictor_without_strides_is_the_net_it_was():
    net = sisr_amd.predictor.DegradationPredictor(num_outputs=12)
    same = sisr_amd.predictor.DegradationPredictor(num_outputs=12, strides=None)
    ones = sisr_amd.predictor.DegradationPredictor(num_outputs=12, strides=[1] * 6)
    want = {k: tuple(v.shape) for k, v in P.Twin(num_outputs=12).state_dict().items()}
    for n in (net, same, ones):
        assert {k: tuple(v.shape) for k, v in n.state_dict().items()} == want
        assert n.strides == [1] * 6 and all(m.stride == (1, 1) for m in n.layer_dict.children())


def test_predictor_strides_are_checked_and_reach_the_layers():
    ikc = sisr_amd.predictor.DegradationPredictor(num_outputs=12, strides=S.IKC_STRIDES)
    assert [m.stride for m in ikc.layer_dict.children()] == [(s, s) for s in S.IKC_STRIDES]
    assert list(ikc.state_dict()) == list(S.Twin(strides=S.IKC_STRIDES).state_dict())
    for bad in ([1, 1, 2], [1, 1, 1, 3, 1, 1], [1, 1, 1, 0, 1, 1], [1] * 7):
        with pytest.raises(NotImplementedError, match="strides"):
            sisr_amd.predictor.DegradationPredictor(num_outputs=12, strides=bad)


def test_predictor_handler_passes_the_strides_through(tmp_path):
    make = sisr_amd.available_models["predictor"]
    handler = make(device="cpu", model_save_dir=str(tmp_path), eval_mode=True, metadata=list(P.KEYS), strides=S.IKC_STRIDES,
                   num_features=32)
    assert handler.net.strides == S.IKC_STRIDES
    assert make(device="cpu", model_save_dir=str(tmp_path), eval_mode=True, metadata=list(P.KEYS)).net.strides == [1] * 6
