"""The autograd contract of ops_dense.py's two nodes (pytest -m gpu), as tests/test_convs_contract_gpu.py pins it for convs.py:
frozen inputs, bias=None, a `.grad` that already exists, GRAD_SINK registered as the optimiser registers it, one block
applied twice in one backward pass, deferred_wgrads(), inputs and cotangents of other layouts, two consumers of one output,
retain_graph, in-place edits of a saved stack, and a foreign 192-channel tensor where an open stack used to be.

dense_block: the baseline (everything trainable, `.grad` None, one application, no sink, channels-last) is compared ONCE with
the float64 twin under the project's own rule (tests/_dense.py assert_within_rule: at most 3 x the stock fp32 twin's distance
+ 2^-23; a block is five convs deep, outside the exact-data budget).  Everything else is an EQUALITY of bits against that
baseline, because the kernels are deterministic (tests/test_dense_gpu.py asserts repeatability).  Where autograd adds two
gradients the expectation is the fp32 sum of the two separately computed ones: one commutative fp32 add is what it performs.
dense_skip: dyadic data of tests/_exact.py, so every expectation is the float64 value itself, bit for bit.

One shape, (B, H, W) = (2, 9, 21): two images, one partial 8 x 32 tile below a full one -- the shape of tests/test_rrdb_gpu.py."""
import itertools

import pytest
import torch

import _dense as D
import _exact as E
import sisr_amd

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
DEV = "cuda:0"
CL = torch.channels_last
B, H, W = 2, 9, 21
NAMES = tuple("conv%d.%s" % (j, p) for j in range(1, 6) for p in ("weight", "bias"))
DIFF = ("x",) + NAMES  # the 11 differentiable inputs of a block
SENT = D.SENTINEL

# Chosen on the host, by the float64 twin ALONE: of the seeds 700 .. 704 (all of which keep every LeakyReLU input of BOTH data
# sets D.KINK_MARGIN away from zero) the one with the widest margin, 2.7e-6 and 1.0e-5.
# test_baseline_matches_the_float64_twin asserts the margin.
SEED = 702


def _state(seed):
    torch.manual_seed(seed)
    twin = D.RDBTwin()
    D.randomise_biases(twin, seed + 1)
    return {k: v.detach().clone() for k, v in twin.state_dict().items()}


def _maps(seed):
    """two data sets (input, cotangent) over the same parameters"""
    g = torch.Generator().manual_seed(seed + 2)
    xs = [torch.randn((B, 64, H, W), generator=g) for _ in range(2)]
    cots = [torch.randn((B, 64, H, W), generator=g) for _ in range(2)]
    return xs, cots


SD = _state(SEED)
X, COT = _maps(SEED)


def _dev(t):
    """a device copy that shares nothing with the host tensor it is made from"""
    return t.detach().clone().to(DEV)


def _map(t):
    return _dev(t).contiguous(memory_format=CL)


def _params(sd=SD, frozen=()):
    return {n: sd[n].detach().clone().to(DEV).requires_grad_(n not in frozen) for n in NAMES}


def _input(k, frozen=()):
    return _map(X[k]).requires_grad_("x" not in frozen)


def _block(x, P, none=()):
    return ops.dense_block(x, [(P["conv%d.weight" % j], None if "conv%d.bias" % j in none else P["conv%d.bias" % j])
                               for j in range(1, 6)])


def _grads(x, P):
    return {"x": x.grad, **{n: P[n].grad for n in NAMES}}


def _pass(k, P=None, x=None, cot=None, frozen=(), none=()):
    """one forward and backward pass -> (output, {name: gradient | None}, x, P)"""
    P = _params(frozen=frozen) if P is None else P
    x = _input(k, frozen) if x is None else x
    out = _block(x, P, none)
    out.backward(_map(COT[k]) if cot is None else cot)
    return out.detach(), _grads(x, P), x, P


def same(got, want, what):
    assert got is not None, f"{what}: no gradient"
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert D.same_bits(got, want), (f"{what}: {int((got != want).sum())} of {want.numel()} elements differ from the expected bits, "
                                    f"max |difference| {float((got.double() - want.double()).abs().max()):.3e}")


@pytest.fixture(scope="module")
def base():
    """[(output, {name: gradient})] of the two data sets: computed once, cloned, never written again"""
    runs = []
    for k in (0, 1):
        out, g, _, _ = _pass(k)
        runs.append((out.clone(), {n: v.detach().clone() for n, v in g.items()}))
    torch.cuda.synchronize()
    return runs


@pytest.fixture(autouse=True)
def sinks(monkeypatch):
    """every test starts without a registered sink, whatever earlier modules left behind"""
    monkeypatch.setattr(ops, "GRAD_SINK", {})
    return ops.GRAD_SINK


def _arena(P, gap=64):
    """GRAD_SINK as the flat Adam fills it -- every parameter's slice of one flat arena -- but sentinel-filled and with `gap`
    floats between the slices -> (arena, {name: view}, mask of the floats outside every slice)"""
    offs, off = {}, gap
    for n in NAMES:
        offs[n] = off
        off += (P[n].numel() + 63) // 64 * 64 + gap
    flat = torch.full((off,), SENT, device=DEV)
    outside = torch.ones(off, dtype=torch.bool, device=DEV)
    views = {}
    for n in NAMES:
        views[n] = flat[offs[n]:offs[n] + P[n].numel()].view_as(P[n])
        outside[offs[n]:offs[n] + P[n].numel()] = False
        ops.GRAD_SINK[P[n].data_ptr()] = views[n]
    return flat, views, outside


# ============================================================================ dense_block
def test_baseline_matches_the_float64_twin(base):
    for k in (0, 1):
        z = D.smallest_preactivation(D.as_dtype(D.RDBTwin, SD, torch.float64), (X[k],))
        assert z > D.KINK_MARGIN, ("TEST BUG (not a kernel failure): a LeakyReLU input of the float64 twin is %.3g, below fp32 "
                                   "resolution (data set %d)" % (z, k))
        out, g = base[k]
        flat = torch.cat([g[n].double().cpu().flatten() for n in NAMES])
        D.assert_within_rule((out, g["x"], flat), D.RDBTwin, SD, (X[k],), COT[k], "dense_block, data set %d" % k)


def _frozen_sets():
    """each of the 11 inputs alone frozen (x alone frozen; a weight frozen beside its trainable bias and the reverse, on the
    growth layers and on conv5), each alone trainable (x alone trainable = all parameters frozen)"""
    sets = [(n,) for n in DIFF] + [tuple(m for m in DIFF if m != n) for n in DIFF]
    assert ("x",) in sets and NAMES in sets and ("conv2.weight",) in sets and ("conv5.bias",) in sets and len(set(sets)) == 22
    return sets


def test_frozen_subsets(base, sinks):
    bout, bg = base[0]
    for frozen in _frozen_sets():
        out, g, _, _ = _pass(0, frozen=frozen)
        what = "frozen %s" % (frozen,)
        same(out, bout, what + " output")
        for n in DIFF:
            if n in frozen:
                assert g[n] is None, f"{what}: frozen {n} received a gradient"
            else:
                same(g[n], bg[n], f"{what} d{n}")


def test_bias_none_equals_a_zero_bias():
    none = ("conv2.bias", "conv5.bias")
    sd = {n: (torch.zeros_like(v) if n in none else v) for n, v in SD.items()}
    zout, zg, _, _ = _pass(0, P=_params(sd))
    out, g, _, P = _pass(0, P=_params(sd), none=none)
    same(out, zout, "bias=None output")
    for n in DIFF:
        if n in none:
            assert P[n].grad is None, n
        else:
            same(g[n], zg[n], "bias=None d%s" % n)


def test_second_pass_adds_to_the_existing_grad(base):
    _, g, x, P = _pass(0)
    kept = dict(g)
    for n in DIFF:
        same(g[n], base[0][1][n], "first pass d%s" % n)
    with torch.no_grad():
        x.copy_(_map(X[1]))
    _, g, _, _ = _pass(1, P=P, x=x)
    for n in DIFF:
        assert g[n] is kept[n], f"{n}: .grad was replaced, not added to"
        same(g[n], base[0][1][n] + base[1][1][n], "kept d%s" % n)


def test_gradients_land_in_registered_sinks_and_nowhere_else(base, sinks):
    P = _params()
    flat, views, outside = _arena(P)
    out, g, _, _ = _pass(0, P=P)
    same(out, base[0][0], "sink output")
    for n in NAMES:
        assert g[n].data_ptr() == views[n].data_ptr(), f"d{n} did not land in its sink"
        same(g[n], base[0][1][n], "sink d%s" % n)
        same(views[n], base[0][1][n], "sink slice of %s" % n)
    same(g["x"], base[0][1]["x"], "sink dx")
    assert bool((flat[outside] == SENT).all()), "something wrote between the slices of the arena"


@pytest.mark.parametrize("with_sink", [False, True])
def test_one_block_applied_twice_in_one_pass(with_sink, sinks, monkeypatch):
    """blk(blk(x)): every parameter gets two gradients in one pass, ten parameters at once through _wb_grad_bufs.  Expected:
    the fp32 sum of the two applications run apart -- the second on the detached intermediate, the first under the dx the
    second produced."""
    cot = _map(COT[0])
    x1, P1, P2 = _input(0), _params(), _params()
    y1 = _block(x1, P1)
    y1d = y1.detach().requires_grad_(True)
    out2 = _block(y1d, P2)
    out2.backward(cot)
    y1.backward(y1d.grad)
    want_out, want_dx = out2.detach().clone(), x1.grad.clone()
    want = {n: P1[n].grad + P2[n].grad for n in NAMES}

    x, P = _input(0), _params()
    views = _arena(P)[1] if with_sink else {}
    log = []
    orig = ops._grad_buf

    def logged(w, gid=None):
        buf = orig(w, gid)
        log.append((w.data_ptr(), buf.data_ptr()))
        return buf

    monkeypatch.setattr(ops, "_grad_buf", logged)
    out = _block(_block(x, P), P)
    out.backward(cot)
    same(out.detach(), want_out, "blk(blk(x))")
    same(x.grad, want_dx, "blk(blk(x)) dx")
    for n in NAMES:
        same(P[n].grad, want[n], "blk(blk(x)) d%s" % n)
        bufs = [b for w, b in log if w == P[n].data_ptr()]
        assert len(bufs) == 2 and bufs[0] != bufs[1], (n, bufs)
        if with_sink:
            assert bufs[0] == views[n].data_ptr(), f"{n}: the first contribution did not land in the sink"
            assert P[n].grad.data_ptr() == views[n].data_ptr(), f"{n}: .grad did not end in the sink"


def test_deferred_wgrads_open_or_closed_give_the_same_bits(base, sinks):
    """conv5 (192 -> 64, alpha 0.2) is never queued today; queued or not, the block must leave the baseline's bits"""
    x, P = _input(0), _params()
    out = _block(x, P)
    with ops.deferred_wgrads():
        out.backward(_map(COT[0]))
    for n, v in _grads(x, P).items():
        same(v, base[0][1][n], "deferred d%s" % n)


def _offset_slice(t):
    buf = torch.full((B + 1, 64, H, W), SENT, device=DEV).contiguous(memory_format=CL)
    buf[1:] = t
    return buf[1:]


def _wide_slice(t):
    buf = torch.full((B, 128, H, W), SENT, device=DEV).contiguous(memory_format=CL)
    buf[:, 64:] = t
    return buf[:, 64:]


def _stack_view(t, c0=0):
    return D.stack([(c0, t)], B, H, W, DEV)[:, c0:c0 + 64]


LAYOUTS = {
    "nchw": lambda t: _dev(t).contiguous(),
    "offset slice": lambda t: _offset_slice(_dev(t)),          # channels-last behind a nonzero storage offset
    "pitch 128 slice": lambda t: _wide_slice(_dev(t)),         # a pitch the kernels do not read: copied
    "pitch 192 view": lambda t: _stack_view(t),                  # read in place (_pitched)
    "pitch 192 view at channel 64": lambda t: _stack_view(t, 64),
}


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_layouts_of_input_and_cotangent(layout, base):
    make = LAYOUTS[layout]
    cot = make(COT[0])
    assert layout == "nchw" or cot.storage_offset() or cot.stride(3) == 192
    keep = cot.clone()
    out, g, _, _ = _pass(0, cot=cot)
    assert torch.equal(cot, keep), "the backward pass wrote into its cotangent"
    same(out, base[0][0], "cot %s: output" % layout)
    for n in DIFF:
        same(g[n], base[0][1][n], "cot %s: d%s" % (layout, n))
    x = make(X[0]).requires_grad_(True)
    out, g, _, _ = _pass(0, x=x, cot=cot)
    same(out, base[0][0], "x and cot %s: output" % layout)
    for n in DIFF:
        same(g[n], base[0][1][n], "x and cot %s: d%s" % (layout, n))


def test_two_consumers_of_one_output():
    """y = blk1(x) feeds blk2, which fills y's stack in place, and blk3, which copies: the same graph over two copies of y"""
    sds = [SD, _state(SEED + 10), _state(SEED + 20)]
    cots = [_map(COT[0]), _map(COT[1])]
    runs = []
    for copies in (False, True):
        x, Ps = _input(0), [_params(sd) for sd in sds]
        y = _block(x, Ps[0])
        keep = y.detach().clone()
        feed = (lambda: y.contiguous(memory_format=CL)) if copies else (lambda: y)
        a, b = _block(feed(), Ps[1]), _block(feed(), Ps[2])
        torch.autograd.backward([a, b], cots)
        assert torch.equal(y.detach(), keep), "filling the stack behind y, or a backward pass, changed y"
        runs.append((a.detach(), b.detach(), x.grad, Ps))
    (a, b, dx, Ps), (wa, wb, wdx, wPs) = runs
    same(a, wa, "first consumer")
    same(b, wb, "second consumer")
    same(dx, wdx, "dx")
    for i in range(3):
        for n in NAMES:
            same(Ps[i][n].grad, wPs[i][n].grad, "block %d d%s" % (i + 1, n))


def test_retain_graph_backward_twice_gives_twice_the_gradient(base):
    x, P = _input(0), _params()
    out = _block(x, P)
    cot = _map(COT[0])
    out.backward(cot, retain_graph=True)
    out.backward(cot)
    for n, v in _grads(x, P).items():
        same(v, base[0][1][n] + base[0][1][n], "twice d%s" % n)


@pytest.mark.parametrize("how", ["detached alias", "under no_grad"])
def test_editing_an_output_whose_stack_a_later_block_saved_is_refused(how):
    """blk2 keeps y's own stack (an as_strided view of y) for its backward: an edit of y afterwards must be noticed by
    autograd's version check (a Python error raised on the host), never answered with gradients of the edited stack"""
    x, P1, P2 = _input(0), _params(), _params(_state(SEED + 10))
    y = _block(x, P1)
    b = _block(y, P2)
    if how == "detached alias":
        y.detach().add_(1)
    else:
        with torch.no_grad():
            y.add_(1)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        b.backward(_map(COT[0]))
    assert all(p.grad is None for p in P2.values()) and x.grad is None


def test_a_foreign_192_channel_tensor_is_never_filled_in_place():
    """a stack that died unclaimed (the trunk's last dense_skip) must leave no claim behind: the allocator hands its block to the
    next (2, 192, 9, 21) tensor, whose channels 64.. are the caller's data"""
    convs = [(SD["conv%d.weight" % j].to(DEV), SD["conv%d.bias" % j].to(DEV)) for j in range(1, 6)]
    t, x = _map(X[0]), _map(X[1])
    g = (E.scales((B, 64), 5)).to(DEV)
    reused = 0
    with torch.no_grad():
        for r in range(4):
            y = ops.dense_skip(t, g, x)
            was = y.data_ptr()
            del y
            Z = ops._empty_cl(B, 192, H, W, DEV)
            Z.fill_(SENT)
            Z[:, :64] = x
            reused += Z.data_ptr() == was
            head = Z[:, :64]
            plain = head.contiguous(memory_format=CL)
            out = ops.dense_block(head, convs)
            assert bool((Z[:, 64:] == SENT).all()), "round %d: dense_block filled a tensor that is not its stack" % r
            same(out, ops.dense_block(plain, convs), "round %d: block on a foreign view" % r)
            y = ops.dense_skip(t, g, x)
            del y
            Z = ops._empty_cl(B, 192, H, W, DEV)
            Z.fill_(SENT)
            Z[:, :64] = x
            head = Z[:, :64]
            plain = head.contiguous(memory_format=CL)
            out = ops.dense_skip(head, g, head)
            assert bool((Z[:, 64:] == SENT).all()) and torch.equal(Z[:, :64], plain)
            same(out, ops.dense_skip(plain, g, plain), "round %d: skip on a foreign view" % r)
            nxt = ops.dense_block(out, convs)  # ... while the genuine output still opens the next block's stack
            assert nxt.shape == out.shape
    print("the allocator reused the dead stack's block in %d of 4 rounds" % reused)


# ============================================================================ dense_skip
def _skip_data(k, gshape=(B, 64)):
    s = 40 + 10 * k
    return dict(t=E.ints((B, 64, H, W), s), g=E.scales(gshape, s + 1), x=E.ints((B, 64, H, W), s + 2), cot=E.ints((B, 64, H, W), s + 3))


def _skip_ref(d):
    """float64 output and gradients of t * g + x under the cotangent (no mask: any data is exact data here)"""
    t, g, x, cot = (d[n].double() for n in ("t", "g", "x", "cot"))
    gb = g.reshape(B, 64, 1, 1)
    return t * gb + x, dict(t=cot * gb, g=(cot * t).sum(dim=(2, 3)).reshape(g.shape), x=cot)


def _skip_leaves(d, trainable=("t", "g", "x")):
    return {n: (_map(v) if v.dim() == 4 and v.shape[-1] > 1 else _dev(v)).requires_grad_(n in trainable)
            for n, v in d.items() if n != "cot"}


@pytest.mark.parametrize("gshape", [(B, 64), (B, 64, 1, 1)])
def test_skip_frozen_subsets_and_the_gates_shape(gshape):
    d = _skip_data(0, gshape)
    want_out, want = _skip_ref(d)
    for r in range(4):
        for S in itertools.combinations(("t", "g", "x"), r):
            lv = _skip_leaves(d, S)
            out = ops.dense_skip(lv["t"], lv["g"], lv["x"])
            E.assert_exact(out, want_out, "dense_skip output, trainable %s" % (S,))
            assert out.requires_grad == bool(S)
            if S:
                out.backward(_map(d["cot"]))
            for n in ("t", "g", "x"):
                if n in S:
                    assert lv[n].grad.shape == lv[n].shape, (n, lv[n].grad.shape)
                    E.assert_exact(lv[n].grad, want[n], "dense_skip d%s, trainable %s" % (n, S))
                else:
                    assert lv[n].grad is None, (S, n)


def test_skip_of_a_map_with_itself_adds_both_gradients():
    d = _skip_data(0)
    lv = _skip_leaves(d)
    out = ops.dense_skip(lv["x"], lv["g"], lv["x"])
    out.backward(_map(d["cot"]))
    ref = dict(d, t=d["x"])
    want_out, want = _skip_ref(ref)
    E.assert_exact(out, want_out, "dense_skip(x, g, x)")
    E.assert_exact(lv["x"].grad, want["t"] + want["x"], "dense_skip(x, g, x) dx")
    E.assert_exact(lv["g"].grad, want["g"], "dense_skip(x, g, x) dg")


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_skip_layouts_of_inputs_and_cotangent(layout):
    make = LAYOUTS[layout]
    d = _skip_data(0)
    want_out, want = _skip_ref(d)
    for inputs_too in (False, True):
        lv = _skip_leaves(d)
        if inputs_too:
            lv["t"], lv["x"] = make(d["t"]).requires_grad_(True), make(d["x"]).requires_grad_(True)
        cot = make(d["cot"])
        keep = cot.clone()
        out = ops.dense_skip(lv["t"], lv["g"], lv["x"])
        out.backward(cot)
        assert torch.equal(cot, keep)
        E.assert_exact(out, want_out, "dense_skip output (%s)" % layout)
        for n in ("t", "g", "x"):
            E.assert_exact(lv[n].grad, want[n], "dense_skip d%s (%s, inputs too: %s)" % (n, layout, inputs_too))


def test_skip_second_pass_adds_to_the_existing_grad():
    d = [_skip_data(0), _skip_data(1)]
    want = [_skip_ref(v)[1] for v in d]
    lv = _skip_leaves(d[0])
    ops.dense_skip(lv["t"], lv["g"], lv["x"]).backward(_map(d[0]["cot"]))
    kept = {n: lv[n].grad for n in lv}
    with torch.no_grad():
        for n in lv:
            lv[n].copy_(d[1][n])
    ops.dense_skip(lv["t"], lv["g"], lv["x"]).backward(_map(d[1]["cot"]))
    for n in lv:
        assert lv[n].grad is kept[n], n
        E.assert_exact(lv[n].grad, want[0][n] + want[1][n], "dense_skip kept d%s" % n)
