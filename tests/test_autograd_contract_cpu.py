"""The case table of the autograd contract (tests/_contract.py) against the package, on the host: every `Function` subclass
defined in any of its modules (found by walking the package, not listed by hand) has a case or a stated exclusion, every builder / float64 restatement runs, and every exact-data case fits
the significand budget at every size it is run at (so a budget failure can never be met on the GPU first).  The policy of
ops._grad_buf / ops._side_ok for a tensor that gets two gradients in one backward pass is host code and is pinned here too."""
import importlib
import importlib.machinery
import inspect
import os
import pkgutil

import pytest
import torch

import _contract as C
import sisr_amd

ops = sisr_amd.ops


def _defined_nodes(m):
    return {n: o for n, o in vars(m).items()
            if inspect.isclass(o) and issubclass(o, torch.autograd.Function) and o.__module__ == m.__name__}


def _discover():
    """every module of the package, imported on the host, that defines a torch.autograd.Function subclass: a new family module
    is seen without anybody listing it (the built HIP libraries lie in the package directory and are no Python modules)"""
    found = []
    for info in pkgutil.walk_packages(sisr_amd.__path__, sisr_amd.__name__ + "."):
        spec = info.module_finder.find_spec(info.name)
        if not isinstance(spec.loader, importlib.machinery.SourceFileLoader):
            continue
        m = importlib.import_module(info.name)
        if _defined_nodes(m):
            found.append(m)
    return tuple(found)


MODULES = _discover()
FLOOR = 52  # the nodes the package defines today: a discovery that went blind (an import that stopped finding modules) shows


def _nodes():
    nodes = {}
    for m in MODULES:
        for n, o in _defined_nodes(m).items():
            assert n not in nodes, f"two autograd nodes named {n}: {nodes[n].__module__} and {m.__name__} (the table goes by name)"
            nodes[n] = o
    return nodes


def _functions():
    return sorted(_nodes())


def test_discovery_finds_the_family_modules_and_those_beside_them():
    short = {m.__name__.rsplit(".", 1)[-1] for m in MODULES}
    assert {"ops", "ops_chain", "ops_sparnet", "ops_sftmd", "ops_attention", "ops_losses", "convs"} <= short, "the former hand-written list"
    assert {"ops_dense", "pool", "degrade"} <= short, short


def test_every_function_of_ops_has_a_case_or_an_exclusion_reason():
    covered = {f for c in C.CASES for f in c.functions}
    names = _functions()
    assert len(names) >= FLOOR
    missing = [n for n in names if n not in covered and n not in C.EXCLUDED]
    assert not missing, f"autograd operators without a contract case (tests/_contract.py) or an exclusion reason: {missing}"
    stale = sorted((covered | set(C.EXCLUDED)) - set(names))
    assert not stale, f"the table names operators ops.py no longer defines: {stale}"
    both = sorted(covered & set(C.EXCLUDED))
    assert not both, f"excluded AND covered: {both}"
    assert all(isinstance(r, str) and len(r) > 20 for r in C.EXCLUDED.values())


def test_every_user_of_grad_buf_is_in_the_table():
    """the shared-weight test runs every case with a `sink`; that list must keep up with the callers of _grad_buf"""
    src = inspect.getsource(ops)
    users, elsewhere = set(), set()
    for name, node in _nodes().items():
        body = inspect.getsource(node)
        if "_grad_buf(" in body or "_grad_buf_or(" in body or "_wb_grad_bufs(" in body:
            (elsewhere if name in C.EXCLUDED else users).add(name)
    assert "_grad_buf" in src and users == set(C.GRAD_BUF_USERS), sorted(users ^ set(C.GRAD_BUF_USERS))
    # an excluded node that takes buffers is named with the file that runs its sink and shared-weight cases; that file exists,
    # registers sinks, and the node's exclusion reason points to it
    assert elsewhere == set(C.GRAD_BUF_USERS_ELSEWHERE), sorted(elsewhere ^ set(C.GRAD_BUF_USERS_ELSEWHERE))
    for name, path in C.GRAD_BUF_USERS_ELSEWHERE.items():
        assert path in C.EXCLUDED[name], (name, path)
        with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), path)) as f:
            text = f.read()
        assert "GRAD_SINK" in text and "applied_twice" in text, path
    with_sink = {f for c in C.CASES if c.sink for f in c.functions}
    assert set(C.GRAD_BUF_USERS) | {"_MetaGateMany"} == with_sink, sorted(with_sink ^ set(C.GRAD_BUF_USERS))


@pytest.mark.parametrize("case", C.CASES, ids=repr)
def test_builder_restatement_and_budget(case):
    for H, W in case.sizes:
        a, b = case.build(H, W, 0), case.build(H, W, 1)
        assert set(a) == set(b) and "cot" in a and set(case.diff) <= set(a)
        for n in case.params:
            assert torch.equal(a[n], b[n]), f"{n}: parameters must not depend on the data set"
        for n in set(a) - set(case.params):
            assert not torch.equal(a[n], b[n]) or a[n].numel() <= 1, f"{n}: the two data sets must differ"
        del C.PROBE[:]
        out, grads = C.reference(case, a)
        C.reference(case, b)
        if not case.exact:  # no rectified pre-activation may sit where fp32 rounding decides its mask
            assert not C.PROBE or min(C.PROBE) > C.PROBE_FLOOR, f"{case.name} {H}x{W}: |pre-activation| {min(C.PROBE):.2e}"
        assert tuple(out.shape) == tuple(a["cot"].shape)
        for n in case.diff:
            assert tuple(grads[n].shape) == tuple(a[n].shape) and float(grads[n].abs().max()) > 0, n
        if case.exact:
            C.budget(case, a)
            C.budget(case, b)
            if (H, W) == case.main:  # where two gradients are added: kept gradients, a weight applied twice
                C.budget(case, a, b)


def test_subset_policy():
    small, large = C.by_name("conv3x3_c64"), C.by_name("gated_group_ca")
    assert len(C.subsets(small)) == 16
    s = C.subsets(large)
    n = len(large.diff)
    assert tuple(large.diff) in s and tuple(large.params) in s and ("x", "m0") in s
    assert all((d,) in s and tuple(x for x in large.diff if x != d) in s for d in large.diff) and len(s) == 2 * n + 3
    for name in ("conv3x3_c64", "conv3x3_cin3", "conv_f2y", "conv_kxk", "res_block_convs", "refl_conv"):
        c = C.by_name(name)  # the pair the deferred_wgrads docstring used to assume away
        assert ("w",) in C.subsets(c) or ("w1",) in C.subsets(c)


# ----------------------------------------------------------------------------- two gradients of one tensor in one pass
class _TwoBuffers(torch.autograd.Function):
    """a stand-in node: asks _side_ok, then _grad_buf, as the conv nodes do, and fills the buffer with its input"""
    log = []

    @staticmethod
    def forward(ctx, x, w):
        ctx.w = w
        ctx.save_for_backward(x)
        return x * w

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        side = ops._side_ok(ctx.w)
        dw = ops._grad_buf(ctx.w)
        _TwoBuffers.log.append((side, dw.data_ptr()))
        dw.copy_(dy * x)
        return dy * ctx.w, dw


@pytest.fixture
def clean_sink(monkeypatch):
    monkeypatch.setattr(ops, "GRAD_SINK", {})
    monkeypatch.setattr(ops, "WGRAD_SIDE_STREAM", False)  # host tensors: _side_ok's own answer is not under test here
    _TwoBuffers.log = []


def test_second_gradient_of_a_parameter_does_not_get_the_sink_again(clean_sink):
    """a stand-in node on the host: with the sink registered the weight used to end up with twice the second contribution
    ([2, 20] where [101, 1010] is due)"""
    w = torch.tensor([1.0, 10.0], requires_grad=True)
    sink = torch.zeros(2)
    ops.GRAD_SINK[w.data_ptr()] = sink
    x1, x2 = torch.tensor([1.0, 1.0]), torch.tensor([100.0, 100.0])
    y = _TwoBuffers.apply(x1, w) + _TwoBuffers.apply(x2, w)
    y.backward(torch.tensor([1.0, 10.0]))
    assert torch.equal(w.grad, torch.tensor([101.0, 1010.0]))
    ptrs = [p for _, p in _TwoBuffers.log]
    assert ptrs.count(sink.data_ptr()) == 1 and len(set(ptrs)) == 2, "first request: the sink; second: a private buffer"
    assert w.grad.data_ptr() == sink.data_ptr() and torch.equal(sink, torch.tensor([101.0, 1010.0])), "the sum ends in the sink"
    # the next pass starts afresh: one use, the zero-copy path
    w.grad = None
    _TwoBuffers.log = []
    _TwoBuffers.apply(x1, w).backward(torch.tensor([1.0, 10.0]))
    assert w.grad.data_ptr() == sink.data_ptr() and torch.equal(w.grad, torch.tensor([1.0, 10.0]))
    # ... and an existing .grad keeps its rule: a private buffer, added by autograd
    _TwoBuffers.log = []
    _TwoBuffers.apply(x2, w).backward(torch.tensor([1.0, 10.0]))
    assert _TwoBuffers.log[0][1] != sink.data_ptr() and torch.equal(w.grad, torch.tensor([101.0, 1010.0]))
    assert w.grad.data_ptr() == sink.data_ptr()


def test_a_pass_that_died_leaves_no_claim_behind(clean_sink):
    w = torch.tensor([1.0, 10.0], requires_grad=True)
    sink = torch.zeros(2)
    ops.GRAD_SINK[w.data_ptr()] = sink

    class Boom(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, g):
            raise KeyError("the pass dies after the weight's node has run")

    x = torch.ones(2, requires_grad=True)
    with pytest.raises(KeyError):
        _TwoBuffers.apply(Boom.apply(x), w).sum().backward()
    w.grad = None  # (the weight's own gradient had arrived before the pass died)
    _TwoBuffers.log = []
    _TwoBuffers.apply(torch.ones(2), w).sum().backward()
    assert _TwoBuffers.log[0][1] == sink.data_ptr() and w.grad.data_ptr() == sink.data_ptr()


def test_a_pass_that_died_with_the_sum_pending_does_not_touch_a_later_pass(clean_sink):
    """the hook that moves the sum of two contributions into the sink belongs to ONE pass: left behind by a pass that died
    between the second request and the sum, it must not overwrite a .grad that lives in the sink in a later pass"""
    w = torch.tensor([1.0, 10.0], requires_grad=True)
    sink = torch.zeros(2)
    ops.GRAD_SINK[w.data_ptr()] = sink

    class DiesWithItsBuffer(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, v):
            ctx.v = v
            return x * v

        @staticmethod
        def backward(ctx, g):
            ops._grad_buf(ctx.v)
            raise KeyError("the pass dies after the second buffer was handed out")

    x1, x2 = torch.tensor([1.0, 1.0]), torch.tensor([100.0, 100.0])
    with pytest.raises(KeyError):  # (the engine runs the later node first: the stand-in takes the sink, then the other dies)
        (DiesWithItsBuffer.apply(x2, w) + _TwoBuffers.apply(x1, w)).sum().backward()
    assert w.grad is None and [s for s, _ in _TwoBuffers.log] == [False] and _TwoBuffers.log[0][1] == sink.data_ptr()
    sink.copy_(torch.tensor([5.0, 5.0]))
    w.grad = sink.detach()
    _TwoBuffers.apply(x2, w).sum().backward()
    assert w.grad.data_ptr() == sink.data_ptr() and torch.equal(w.grad, torch.tensor([105.0, 105.0]))
    w.grad = None
    _TwoBuffers.apply(x1, w).backward(torch.tensor([1.0, 10.0]))
    assert w.grad.data_ptr() == sink.data_ptr() and torch.equal(w.grad, torch.tensor([1.0, 10.0]))


def test_outside_a_backward_pass_nothing_is_recorded(clean_sink):
    w = torch.ones(2, requires_grad=True)
    sink = torch.zeros(2)
    ops.GRAD_SINK[w.data_ptr()] = sink
    assert ops._grad_buf(w).data_ptr() == sink.data_ptr() and ops._grad_buf(w).data_ptr() == sink.data_ptr()


def test_side_stream_answer_for_first_and_second_contributions(clean_sink, monkeypatch):
    """_side_ok on the stand-in node (it asks BEFORE it takes its buffer, the order every node of ops.py keeps): a weight
    applied once may go to the side stream, pass after pass; applied twice, its first gradient may and its second may not.
    A node that took its buffer first would be refused on every ordinary pass -- shown here by asking again afterwards."""
    monkeypatch.setattr(ops, "WGRAD_SIDE_STREAM", True)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    w = torch.tensor([1.0, 10.0], requires_grad=True)
    x1, x2 = torch.tensor([1.0, 1.0]), torch.tensor([100.0, 100.0])
    for _ in range(2):
        w.grad = None
        _TwoBuffers.log = []
        _TwoBuffers.apply(x1, w).sum().backward()
        assert [s for s, _ in _TwoBuffers.log] == [True], "an unshared weight lost the side stream"
    w.grad = None
    _TwoBuffers.log = []
    (_TwoBuffers.apply(x1, w) + _TwoBuffers.apply(x2, w)).sum().backward()
    assert [s for s, _ in _TwoBuffers.log] == [True, False]
    assert torch.equal(w.grad, torch.tensor([101.0, 101.0]))
    w.grad = None  # kept gradients keep their rule: no side stream into an existing .grad
    _TwoBuffers.apply(x1, w).sum().backward()
    _TwoBuffers.log = []
    _TwoBuffers.apply(x2, w).sum().backward()
    assert [s for s, _ in _TwoBuffers.log] == [False]

    late = []

    class BufferFirst(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, v):
            ctx.v = v
            return x * v

        @staticmethod
        def backward(ctx, dy):
            dv = ops._grad_buf(ctx.v)
            late.append(ops._side_ok(ctx.v))
            return None, dv.copy_(dy)

    v = torch.ones(2, requires_grad=True)
    BufferFirst.apply(x1, v).sum().backward()
    assert late == [False], "the order rule of _side_ok / _grad_buf changed: update the nodes of ops.py and this test"


def test_every_node_of_ops_asks_side_ok_before_it_takes_buffers():
    for name, node in _nodes().items():
        body = inspect.getsource(node)
        if "_side_ok(" in body:
            first_buf = min(i for i in (body.find("_grad_buf("), body.find("_grad_buf_or(")) if i >= 0)
            assert body.find("_side_ok(") < first_buf, f"{name} requests a gradient buffer before it asks _side_ok"
