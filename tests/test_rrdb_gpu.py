"""Residual Dense Blocks, RRDBNet / QRRDBNet and their handlers on the HIP kernels (pytest -m gpu).

Reference: the torch.nn twins of tests/_dense.py in float64 on the host.  Tolerance rule (D.assert_within_rule): for each of
output, input gradient and concatenated parameter gradients under a fixed random cotangent, the relative L2 distance of the
HIP result from the float64 twin is at most 3 x (the same distance of the stock fp32 twin on the CPU, computed in the test)
+ 2^-23 -- the factor covers another summation order at the same precision, the ulp the `* 0.2 + x` epilogues rounded in
another operation order.  No element is excluded."""
import pytest
import torch

import _dense as D
import sisr_amd

pytestmark = pytest.mark.gpu
ops, hip, rrdb = sisr_amd.ops, sisr_amd.hip, sisr_amd.rrdb
DEV = "cuda:0"
CL = torch.channels_last


def _rdb_case(B, H, W, seed):
    torch.manual_seed(seed)
    twin = D.RDBTwin()
    D.randomise_biases(twin, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    x, cot = torch.randn((B, 64, H, W), generator=g), torch.randn((B, 64, H, W), generator=g)
    return twin.state_dict(), x, cot


def _hip_rdb(sd, x, cot, frozen=()):
    """ops.dense_block on the twin's weights -> (out, dx | None, {name: grad | None}); frozen: names ('x', 'conv2', ...)"""
    params = {k: v.detach().clone().to(DEV).requires_grad_(k.split(".")[0] not in frozen) for k, v in sd.items()}
    xl = x.to(DEV).contiguous(memory_format=CL).requires_grad_("x" not in frozen)
    convs = [(params["conv%d.weight" % j], params["conv%d.bias" % j]) for j in range(1, 6)]
    out = ops.dense_block(xl, convs)
    out.backward(cot.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), xl.grad, {k: p.grad for k, p in params.items()}


@pytest.mark.parametrize("shape", [(2, 9, 21), (1, 37, 70)])
def test_dense_block_matches_the_float64_twin_within_three_times_stock_fp32(shape):
    B, H, W = shape
    sd, x, cot = _rdb_case(B, H, W, 600 + H)
    out, dx, grads = _hip_rdb(sd, x, cot)
    assert out.shape == (B, 64, H, W) and all(g is not None for g in grads.values())
    flat = torch.cat([grads[k].double().cpu().flatten() for k in sd])
    D.assert_within_rule((out, dx, flat), D.RDBTwin, sd, (x,), cot, "dense_block %s" % (shape,))


def test_dense_block_output_opens_the_next_blocks_stack_and_chains_without_a_copy():
    """a block's result is the first 64 channels of a fresh 192-channel stack; the next block fills that stack in place, a
    second consumer of the same map gets a stack of its own, and both compute what a contiguous copy of the map gives"""
    sd, x, _ = _rdb_case(2, 9, 21, 610)
    convs = [(sd["conv%d.weight" % j].to(DEV), sd["conv%d.bias" % j].to(DEV)) for j in range(1, 6)]
    with torch.no_grad():
        y = ops.dense_block(x.to(DEV).contiguous(memory_format=CL), convs)
        assert y.stride() == (9 * 21 * 192, 1, 21 * 192, 192)
        keep = y.clone()
        plain = ops.dense_block(y.contiguous(memory_format=CL), convs)
        first = ops.dense_block(y, convs)   # claims y's stack
        second = ops.dense_block(y, convs)  # the stack is taken: copies
        torch.cuda.synchronize()
    assert torch.equal(y, keep), "filling the stack behind a map must not change the map"
    assert torch.equal(first, plain) and torch.equal(second, plain)


def test_dense_block_saves_exactly_its_stack():
    B, H, W = 2, 9, 21
    sd, x, cot = _rdb_case(B, H, W, 620)
    saved = []

    def pack(t):
        if t.dim() == 4 and t.shape[0] == B and tuple(t.shape[2:]) == (H, W):
            saved.append(t.numel() * t.element_size())
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        params = {k: v.detach().clone().to(DEV).requires_grad_(True) for k, v in sd.items()}
        xl = x.to(DEV).contiguous(memory_format=CL).requires_grad_(True)
        out = ops.dense_block(xl, [(params["conv%d.weight" % j], params["conv%d.bias" % j]) for j in range(1, 6)])
    assert sum(saved) == B * H * W * 192 * 4, saved
    out.backward(cot.to(DEV))
    torch.cuda.synchronize()


def _count_calls(monkeypatch, name):
    L, calls = hip.lib(), []
    orig = getattr(L, name)

    def counted(*args):
        calls.append(args)
        return orig(*args)

    monkeypatch.setattr(L, name, counted)
    return calls


def test_dense_block_skips_the_launches_of_frozen_inputs_and_weights(monkeypatch):
    sd, x, cot = _rdb_case(2, 9, 21, 630)
    dgrads, wgrads = _count_calls(monkeypatch, "sisr_dense3x3_dgrad"), _count_calls(monkeypatch, "sisr_dense3x3_wgrad")
    out, dx, full = _hip_rdb(sd, x, cot)
    assert (len(dgrads), len(wgrads)) == (4, 4) and dx is not None
    del dgrads[:], wgrads[:]
    out_f, dx_f, g = _hip_rdb(sd, x, cot, frozen=("x",))
    assert dx_f is None and len(wgrads) == 4
    assert len(dgrads) == 3 and all(a[8] != 64 for a in dgrads), "no first-layer input gradient into a frozen input"
    assert torch.equal(out_f, out) and all(torch.equal(g[k], full[k]) for k in sd)
    del dgrads[:], wgrads[:]
    out_w, dx_w, g = _hip_rdb(sd, x, cot, frozen=("conv2",))
    assert len(dgrads) == 4 and len(wgrads) == 3 and all(a[2] != 96 for a in wgrads), "no weight gradient for frozen weights"
    assert g["conv2.weight"] is None and g["conv2.bias"] is None
    assert torch.equal(dx_w, dx) and all(torch.equal(g[k], full[k]) for k in sd if not k.startswith("conv2"))
    del dgrads[:], wgrads[:]
    _, dx_a, g = _hip_rdb(sd, x, cot, frozen=("x", "conv1", "conv2"))  # nothing below layer 3 wants a gradient
    assert len(dgrads) == 1 and dgrads[0][8] == 160 and len(wgrads) == 2
    assert all(torch.equal(g[k], full[k]) for k in sd if k[:5] in ("conv3", "conv4", "conv5"))


# ----------------------------------------------------------------------------- the nets
def _net_case(M, seed):
    torch.manual_seed(seed)
    twin = D.RRDBNetTwin(num_blocks=2, M=M)
    D.randomise_biases(twin, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    x, cot = torch.rand((2, 3, 12, 20), generator=g), torch.randn((2, 3, 48, 80), generator=g)
    md = torch.rand((2, M, 1, 1), generator=g) if M else None
    return twin.state_dict(), x, cot, md


# the first seeds from 640 / 651 on at which the float64 twin alone has no LeakyReLU input within D.KINK_MARGIN of zero
NET_SEEDS = {None: 670, 11: 663}


@pytest.mark.parametrize("M", [None, 11])
def test_rrdbnet_and_qrrdbnet_match_the_float64_twin_within_three_times_stock_fp32(M):
    sd, x, cot, md = _net_case(M, NET_SEEDS[M])
    z = D.smallest_preactivation(D.as_dtype(D.RRDBNetTwin, sd, torch.float64, num_blocks=2, M=M), (x,) if M is None else (x, md))
    assert z > D.KINK_MARGIN, "TEST BUG (not a kernel failure): a LeakyReLU input of the float64 twin is %.3g, below fp32 resolution" % z
    net = rrdb.RRDBNet(num_blocks=2) if M is None else rrdb.QRRDBNet(num_blocks=2, input_para=M)
    net.load_state_dict(sd, strict=True)  # the twin's state dict, as it is
    net.to(DEV)
    xl = x.to(DEV).requires_grad_(True)
    out = net(xl) if M is None else net(xl, md.to(DEV))
    assert out.shape == (2, 3, 48, 80)
    out.backward(cot.to(DEV))
    torch.cuda.synchronize()
    named = dict(net.named_parameters())
    names = [k for k, _ in D.RRDBNetTwin(num_blocks=2, M=M).named_parameters()]
    flat = torch.cat([named[k].grad.double().cpu().flatten() for k in names])
    inputs = (x,) if M is None else (x, md)
    D.assert_within_rule((out, xl.grad, flat), D.RRDBNetTwin, sd, inputs, cot, "RRDBNet M=%s" % M, num_blocks=2, M=M)


# ----------------------------------------------------------------------------- the handler
def _handler(tmp_path, eval_mode=False, **extra):
    torch.manual_seed(8)
    return sisr_amd.handlers.available_models["rrdb"](device=0, model_save_dir=str(tmp_path), eval_mode=eval_mode, lr=1e-4,
                                                      num_blocks=2, **extra)


def _batches(n):
    g = torch.Generator().manual_seed(5)
    return [(torch.rand(2, 3, 12, 20, generator=g), torch.rand(2, 3, 48, 80, generator=g)) for _ in range(n)]


def test_rrdb_handler_steps_under_graph_capture_equal_eager_bit_for_bit(tmp_path):
    runs = {}
    for mode in (False, True):
        h = _handler(tmp_path)
        assert h.colorspace == 'rgb' and h.im_input == 'unmodified' and h.model_name == 'rrdb'
        h.use_graph = mode
        losses = [h.train_step(x, y)[0].clone() for x, y in _batches(3)]
        torch.cuda.synchronize()
        runs[mode] = (losses, [p.detach().clone() for p in h.net.parameters()])
    for a, b in zip(runs[False][0], runs[True][0]):
        assert torch.equal(a, b), (float(a), float(b))
    assert runs[False][0][0] != runs[False][0][2], "test bug: the steps do not move the loss"
    for (k, _), a, b in zip(h.net.named_parameters(), runs[False][1], runs[True][1]):
        assert torch.equal(a, b), k


def test_rrdb_handler_first_loss_matches_the_twin_and_a_saved_model_evaluates_bit_for_bit(tmp_path):
    h = _handler(tmp_path)
    sd = {k: v.detach().clone().cpu() for k, v in h.net.state_dict().items()}
    (x, y), = _batches(1)
    loss, _ = h.train_step(x, y)
    with torch.no_grad():
        l64, l32 = [float((D.as_dtype(D.RRDBNetTwin, sd, dt, num_blocks=2)(x.to(dt)) - y.to(dt)).abs().mean())
                    for dt in (torch.float64, torch.float32)]
    e_hip, e_stock = abs(float(loss.double()) - l64) / l64, abs(l32 - l64) / l64
    print("first L1 loss: hip %.9g, float64 twin %.9g; relative distance hip %.3g, stock fp32 %.3g" % (float(loss), l64, e_hip, e_stock))
    assert e_hip <= 3 * e_stock + D.ULP, (e_hip, e_stock)
    h.save_model("m", 0)
    want = h.run_eval(x, keep_on_device=True)[0]
    again = h.run_eval(x, keep_on_device=True, self_ensemble=True)[0]
    assert again.shape == want.shape and torch.isfinite(again).all()
    h2 = _handler(tmp_path, eval_mode=True)
    assert not torch.equal(h2.run_eval(x, keep_on_device=True)[0], want), "test bug: the step did not move the weights"
    h2.load_model("m", 0)
    assert torch.equal(h2.run_eval(x, keep_on_device=True)[0], want)


def test_qrrdb_handler_trains_on_metadata(tmp_path):
    torch.manual_seed(8)
    h = sisr_amd.handlers.available_models["qrrdb"](device=0, model_save_dir=str(tmp_path), eval_mode=False, lr=1e-4, num_blocks=2,
                                                    metadata=["blur_kernel"])
    assert h.colorspace == 'augmented_rgb' and h.im_input == 'unmodified' and h.model_name == 'qrrdb'
    (x, y), = _batches(1)
    md = torch.rand(2, h.num_metadata, 1, 1).to(DEV)
    before = [p.detach().clone() for p in h.net.parameters()]
    loss, out = h.train_step(x, y, extra_channels=md)
    torch.cuda.synchronize()
    assert out.shape == (2, 3, 48, 80) and torch.isfinite(loss)
    moved = [not torch.equal(a, b) for a, b in zip(before, h.net.parameters())]
    assert all(moved), "every parameter, the meta-attention layers' included, takes a gradient"
