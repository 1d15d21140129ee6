"""The autograd contract of convs.py's two nodes (pytest -m gpu), as tests/test_autograd_contract_gpu.py pins it for the nodes
of ops.py: frozen inputs, a `.grad` that already exists, GRAD_SINK registered as the optimiser registers it, a weight applied
twice in one backward pass, and hipGraph capture.  The baseline of each operator (everything trainable, `.grad` None, one
application, no sink) is exact against float64 in tests/test_stride2_gpu.py / test_corrector_gpu.py; everything here is an
EQUALITY against that baseline, because the kernels are deterministic.  Data: tests/_exact.py's, so sums of two gradients
are exact too."""
import itertools

import pytest
import torch

import _exact as E
import sisr_amd

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
DEV = "cuda:0"
CL = torch.channels_last
B, H, W = 3, 9, 21


def _map(t):
    return t.contiguous(memory_format=CL).to(DEV)


def _s2(t):
    return ops.conv_kxk(t["x"], t["w"], t["b"], slope=0.5, stride=2)


def _pw(t):
    return ops.conv_1x1(t["x"], t["w"], t["b"], slope=0.5, image_bias=t["ib"])


def _data(op, k):
    """data set k (0 / 1) over the SAME parameters"""
    if op is _s2:
        return dict(x=_map(E.ints((B, 64, H, W), 300 + k)), w=E.weights((48, 64, 5, 5), 310).to(DEV), b=E.biases(48, 311).to(DEV),
                    cot=_map(E.ints((B, 64, 5, 11), 320 + k)))
    return dict(x=_map(E.ints((B, 64, H, W), 330 + k)), w=E.weights((128, 64, 1, 1), 340).to(DEV), b=E.biases(128, 341).to(DEV),
                ib=(E.ints((B, 128), 350 + k, -8, 8) / 8).to(DEV), cot=_map(E.ints((B, 128, H, W), 360 + k)))


OPS = [pytest.param(_s2, ("x", "w", "b"), id="conv_kxk_s2"), pytest.param(_pw, ("x", "w", "b", "ib"), id="conv_1x1")]


def _leaves(td, req, share=None):
    return {n: (v if n == "cot" else share[n] if share and n in share else v.detach().clone().requires_grad_(n in req))
            for n, v in td.items()}


def _run(op, lv):
    out = op(lv)
    if out.requires_grad:
        out.backward(lv["cot"])
    return out.detach()


@pytest.fixture
def sinks(monkeypatch):
    monkeypatch.setattr(ops, "GRAD_SINK", {})
    return ops.GRAD_SINK


def _baseline(op, diff, k):
    lv = _leaves(_data(op, k), diff)
    out = _run(op, lv)
    return out, {n: lv[n].grad.clone() for n in diff}


@pytest.mark.parametrize("op, diff", OPS)
def test_requires_grad_subsets(op, diff, sinks):
    bout, bg = _baseline(op, diff, 0)
    for r in range(len(diff) + 1):
        for S in itertools.combinations(diff, r):
            lv = _leaves(_data(op, 0), S)
            assert torch.equal(_run(op, lv), bout), S
            for n in diff:
                if n in S:
                    assert torch.equal(lv[n].grad, bg[n]), (S, n)
                else:
                    assert lv[n].grad is None, (S, n)


@pytest.mark.parametrize("op, diff", OPS)
@pytest.mark.parametrize("with_sink", [False, True])
def test_kept_gradients_and_the_sink(op, diff, with_sink, sinks):
    """two passes without clearing .grad: the fp32 sum of the single-pass gradients; with a sink registered the first pass is
    written where the sink is (autograd adopts it: zero copy) and the second is added to it.  A pass into a zeroed .grad equals
    the single pass."""
    g = [_baseline(op, diff, k)[1] for k in (0, 1)]
    lv = _leaves(_data(op, 0), diff)
    params = {n: lv[n] for n in ("w", "b")}
    views = {}
    if with_sink:
        for n, p in params.items():
            views[n] = sinks[p.data_ptr()] = torch.zeros_like(p)
    _run(op, lv)
    for n, p in params.items():
        assert torch.equal(p.grad, g[0][n])
        if with_sink:
            assert p.grad.data_ptr() == views[n].data_ptr(), "d%s did not land in its sink" % n
    _run(op, _leaves(_data(op, 1), diff, share=params))
    for n, p in params.items():
        assert torch.equal(p.grad, g[0][n] + g[1][n]), n
    sinks.clear()
    lv = _leaves(_data(op, 0), diff)
    for n in ("w", "b"):
        lv[n].grad = torch.zeros_like(lv[n])
    _run(op, lv)
    for n in ("w", "b"):
        assert torch.equal(lv[n].grad, g[0][n]), n


@pytest.mark.parametrize("op, diff", OPS)
@pytest.mark.parametrize("with_sink", [False, True])
def test_weights_applied_twice_in_one_pass(op, diff, with_sink, sinks):
    g = [_baseline(op, diff, k)[1] for k in (0, 1)]
    a = _leaves(_data(op, 0), diff)
    params = {n: a[n] for n in ("w", "b")}
    b = _leaves(_data(op, 1), diff, share=params)
    if with_sink:
        for p in params.values():
            sinks[p.data_ptr()] = torch.zeros_like(p)
    outs = [op(a), op(b)]
    torch.autograd.backward(outs, [a["cot"], b["cot"]])
    for n, p in params.items():
        assert torch.equal(p.grad, g[0][n] + g[1][n]), n
    for k, lv in enumerate((a, b)):
        for n in set(diff) - set(params):
            assert torch.equal(lv[n].grad, g[k][n]), (k, n)


@pytest.mark.parametrize("op, diff", OPS)
def test_forward_and_backward_under_graph_capture_equal_eager(op, diff, sinks):
    """workspaces come from hip.workspace and nothing synchronises with the host: the pass captures, and its replay on new
    data in the captured buffers gives the eager bits"""
    want_out, want = _baseline(op, diff, 1)
    lv = _leaves(_data(op, 0), diff)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):  # warm-up outside the capture: allocator pools, the library's once-only attributes
        _run(op, lv)
    torch.cuda.current_stream().wait_stream(stream)
    grads = {}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(lv)
        got = torch.autograd.grad(out, [lv[n] for n in diff], lv["cot"])
        grads = dict(zip(diff, got))
    new = _data(op, 1)
    with torch.no_grad():
        for n in ("x", "ib"):
            if n in lv:
                lv[n].copy_(new[n])
        lv["cot"].copy_(new["cot"])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), want_out)
    for n in diff:
        assert torch.equal(grads[n], want[n]), n
