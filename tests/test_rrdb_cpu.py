"""RRDBNet / QRRDBNet, host side (no GPU): registry, parameter count, state-dict compatibility with the torch.nn twin written from
the definition (BasicSR's names), the dense convs' initialisation, the refusals."""
import math

import pytest
import torch

import _dense as D
import sisr_amd

rrdb, handlers, ops = sisr_amd.rrdb, sisr_amd.handlers, sisr_amd.ops


def test_handlers_are_registered_under_their_names():
    assert handlers.available_models['rrdb'] is rrdb.RRDBHandler
    assert handlers.available_models['qrrdb'] is rrdb.QRRDBHandler
    assert issubclass(rrdb.RRDBHandler, handlers.BaseModel) and issubclass(rrdb.QRRDBHandler, handlers.QModel)


def test_default_net_has_the_generator_parameter_count():
    net, twin = rrdb.RRDBNet(), D.RRDBNetTwin()
    n = sum(p.numel() for p in net.parameters())
    assert n == 16697987 == sum(p.numel() for p in twin.parameters())


@pytest.mark.parametrize("M", [None, 11])
def test_state_dict_keys_and_shapes_equal_the_twins(M):
    if M is None:
        net, twin = rrdb.RRDBNet(num_blocks=2), D.RRDBNetTwin(num_blocks=2)
    else:
        net, twin = rrdb.QRRDBNet(num_blocks=2, input_para=M), D.RRDBNetTwin(num_blocks=2, M=M)
    a, b = net.state_dict(), twin.state_dict()
    assert list(a) == list(b)
    assert [tuple(v.shape) for v in a.values()] == [tuple(v.shape) for v in b.values()]
    for name in ("conv_first.weight", "body.1.rdb3.conv5.bias", "conv_body.weight", "conv_up1.weight", "conv_up2.bias",
                 "conv_hr.weight", "conv_last.bias"):
        assert name in a, name
    net.load_state_dict(b, strict=True)  # a checkpoint written by the plain modules loads as it is
    if M is not None:
        assert [id(m) for m in net.meta_gate_layers()] == [id(blk.attention_layer) for blk in net.body]


def test_dense_convs_start_kaiming_normal_times_a_tenth_with_zero_bias():
    torch.manual_seed(3)
    net = rrdb.RRDBNet(num_blocks=1)
    w = net.body[0].rdb1.conv1.weight
    want = 0.1 * math.sqrt(2 / 576)
    assert abs(float(w.detach().std()) / want - 1) < 0.05
    assert not net.body[0].rdb1.conv1.bias.any() and not net.body[0].rdb3.conv5.bias.any()
    assert abs(float(net.body[0].rdb2.conv5.weight.detach().std()) / (0.1 * math.sqrt(2 / (192 * 9))) - 1) < 0.05
    assert net.conv_body.bias.any(), "the other convs keep torch's default initialisation"


@pytest.mark.parametrize("kwargs, word", [(dict(scale=2), "scale"), (dict(scale=1), "scale"), (dict(num_features=48), "num_features"),
                                          (dict(num_grow_ch=16), "num_grow_ch")])
def test_unbuilt_configurations_are_refused_with_a_clear_message(kwargs, word):
    for cls in (rrdb.RRDBNet, rrdb.QRRDBNet):
        with pytest.raises(NotImplementedError, match=word):
            cls(num_blocks=1, **kwargs)


def test_nets_raise_under_another_precision_and_on_the_cpu():
    net = rrdb.RRDBNet(num_blocks=1)
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP device"):
        net(torch.zeros(1, 3, 8, 8))
    blk = net.body[0].rdb1
    ops.set_precision("bf16")
    try:
        with pytest.raises(NotImplementedError, match="fp32"):
            blk(torch.zeros(1, 64, 8, 8))
    finally:
        ops.set_precision("fp32")
    with pytest.raises(RuntimeError, match="metadata"):
        rrdb.QRRDBNet(num_blocks=1, input_para=3)._gates(None)
