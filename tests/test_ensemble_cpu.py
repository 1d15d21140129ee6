"""Geometric self-ensemble (ensemble.py) on the host: the host form of dihedral_fan / dihedral_merge, which is the
specification the kernels are tested against (tests/test_ensemble_gpu.py), the handler helper around a stand-in forward,
the metadata handling, and the host-side argument checks of the device entry points (no GPU needed)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import sisr_amd

E = sisr_amd.ensemble


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def test_host_merge_of_fan_is_the_identity_bit_for_bit():
    """eight equal values summed pairwise are x * 8 exactly, and * 0.125 is exact"""
    for shape in ((2, 3, 5, 7), (1, 1, 1, 9), (1, 2, 6, 1), (3, 5, 33, 31)):
        x = _rand(shape, 11)
        up, tu = E.dihedral_fan(x)
        n, c, h, w = shape
        assert up.shape == (4 * n, c, h, w) and tu.shape == (4 * n, c, w, h) and up.is_contiguous() and tu.is_contiguous()
        assert torch.equal(E.dihedral_merge(up, tu), x)


def test_host_fan_variant_order():
    x = _rand((2, 3, 5, 7), 12)
    up, tu = E.dihedral_fan(x)
    xt = x.transpose(-1, -2)
    want_up = [x, x.flip(-1), x.flip(-2), x.flip(-2, -1)]
    want_tu = [xt, xt.flip(-1), xt.flip(-2), xt.flip(-2, -1)]
    for k in range(4):  # variant-major: image i of variant k is entry k * n + i
        assert torch.equal(up[2 * k:2 * k + 2], want_up[k]), k
        assert torch.equal(tu[2 * k:2 * k + 2], want_tu[k]), k
        for i in range(2):
            assert torch.equal(up[k * 2 + i], want_up[k][i]) and torch.equal(tu[k * 2 + i], want_tu[k][i])


def test_host_merge_inverts_each_variant_and_sums_in_the_documented_order():
    """eight independent maps: variant k of the inputs holds map k under operation k, so the merge must see the maps"""
    n, c, H, W = 2, 3, 5, 7
    maps = [_rand((n, c, H, W), 20 + k) * 10 ** (k - 4) for k in range(8)]  # spread magnitudes: the order of the adds shows
    ops = [lambda t: t, lambda t: t.flip(-1), lambda t: t.flip(-2), lambda t: t.flip(-2, -1)]
    up = torch.cat([ops[k](maps[k]) for k in range(4)]).contiguous()
    tu = torch.cat([ops[k](maps[4 + k].transpose(-1, -2)) for k in range(4)]).contiguous()
    u, t = maps[:4], maps[4:]
    want = (((u[0] + u[1]) + (u[2] + u[3])) + ((t[0] + t[1]) + (t[2] + t[3]))) * 0.125
    assert torch.equal(E.dihedral_merge(up, tu), want)
    other = ((((((u[0] + u[1]) + u[2]) + u[3]) + t[0]) + t[1]) + t[2] + t[3]) * 0.125
    assert not torch.equal(other, want)  # (the data does tell the orders apart)


def test_operators_refuse_gradients_and_wrong_shapes():
    x = _rand((1, 3, 4, 6), 13)
    with pytest.raises(RuntimeError, match="requires grad"):
        E.dihedral_fan(x.clone().requires_grad_(True))
    up, tu = E.dihedral_fan(x)
    with pytest.raises(RuntimeError, match="requires grad"):
        E.dihedral_merge(up.clone().requires_grad_(True), tu)
    with pytest.raises(ValueError):
        E.dihedral_merge(up, up)            # the turned batch must be (4n, c, W, H)
    with pytest.raises(ValueError):
        E.dihedral_merge(up[:3], tu[:3])    # not a multiple of four
    with pytest.raises(ValueError):
        E.dihedral_fan(x.double())


def test_entry_points_refuse_bad_arguments_before_any_device_call():
    """sisr_dihedral_fan / _merge validate on the host and return SISR_ERR_ARG without a launch (this runs with no GPU)."""
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)  # a non-null stand-in: every call below must fail before it is dereferenced
    ERR_ARG = -1

    def fan(x=p, n=1, c=3, h=4, w=5, up=p, tu=p):
        return L.sisr_dihedral_fan(x, n, c, h, w, up, tu, None)

    def merge(up=p, tu=p, n=1, c=3, h=4, w=5, out=p):
        return L.sisr_dihedral_merge(up, tu, n, c, h, w, out, None)
    assert fan(x=None) == ERR_ARG and fan(up=None) == ERR_ARG and fan(tu=None) == ERR_ARG
    assert merge(up=None) == ERR_ARG and merge(tu=None) == ERR_ARG and merge(out=None) == ERR_ARG
    for call in (fan, merge):
        for name in ("n", "c", "h", "w"):
            for bad in (0, -1, -(2 ** 31)):
                assert call(**{name: bad}) == ERR_ARG, (call.__name__, name, bad)


def _nearest(scale):
    """a pointwise stand-in network: nearest-neighbour x scale commutes with every flip and transpose"""
    return lambda t, e=None: F.interpolate(t, scale_factor=scale, mode="nearest")


@pytest.mark.parametrize("shape", [(1, 3, 6, 9), (2, 1, 7, 4)])
def test_helper_around_a_pointwise_forward_returns_its_plain_output(shape):
    x = _rand(shape, 14)
    seen = []

    def forward(t, e):
        assert e is None
        seen.append(tuple(t.shape))
        return _nearest(3)(t)
    out = E.self_ensemble(forward, x)
    n, c, h, w = shape
    assert seen == [(4 * n, c, h, w), (4 * n, c, w, h)]  # two forwards at batch 4n
    assert torch.equal(out, _nearest(3)(x))


def test_extra_channels_follow_the_input():
    x = _rand((2, 3, 6, 9), 15)
    vec = _rand((2, 10, 1, 1), 16)
    a, b = E.fan_extra_channels(vec, x)
    assert a.shape == (8, 10, 1, 1) and torch.equal(a, b)
    for k in range(4):
        assert torch.equal(a[2 * k:2 * k + 2], vec)  # variant-major repeat: entry k * n + i is image i's vector
    maps = _rand((2, 4, 6, 9), 17)
    a, b = E.fan_extra_channels(maps, x)
    want = E.dihedral_fan(maps)
    assert torch.equal(a, want[0]) and torch.equal(b, want[1]) and b.shape == (8, 4, 9, 6)
    assert E.fan_extra_channels(None, x) == (None, None)
    with pytest.raises(NotImplementedError):
        E.fan_extra_channels(_rand((2, 4, 2, 2), 18), x)
    # ... and reach the forward in step with the image batch
    got = []

    def forward(t, e):
        got.append((tuple(t.shape), tuple(e.shape)))
        return t * e[:, :1]
    E.self_ensemble(forward, x, vec)
    E.self_ensemble(forward, x, maps)
    assert got == [((8, 3, 6, 9), (8, 10, 1, 1)), ((8, 3, 9, 6), (8, 10, 1, 1)),
                   ((8, 3, 6, 9), (8, 4, 6, 9)), ((8, 3, 9, 6), (8, 4, 9, 6))]
    with pytest.raises(NotImplementedError):
        E.self_ensemble(forward, x, _rand((2, 4, 2, 2), 18))


def test_run_eval_takes_the_keyword_on_every_path():
    """BaseModel.run_eval and the chopped run_eval of SAN / QSAN (the overrides that do not end in BaseModel.run_eval)"""
    import inspect
    H, S = sisr_amd.handlers, sisr_amd.san
    for fn in (H.BaseModel.run_eval, S.SANHandler.run_eval, S.QSANHandler.run_eval):
        p = inspect.signature(fn).parameters["self_ensemble"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__qualname__


def test_handler_on_the_host_with_a_stand_in_forward(tmp_path):
    """run_eval(self_ensemble=True) end to end on a CPU handler whose run_model is the stand-in: the plain result, and the
    loss of the merged output"""
    h = sisr_amd.handlers.EDSRHandler(device=torch.device("cpu"), model_save_dir=str(tmp_path), eval_mode=True,
                                      num_features=16, num_blocks=1)
    h.run_model = lambda t, *a, **k: _nearest(4)(t)
    h.criterion = torch.nn.L1Loss()  # (the handler's own is the device kernel)
    x, y = _rand((2, 3, 6, 9), 19), _rand((2, 3, 24, 36), 20)
    plain, loss0, _ = h.run_eval(x, y, request_loss=True)
    plus, loss1, _ = h.run_eval(x, y, request_loss=True, self_ensemble=True)
    assert torch.equal(plain, plus) and float(loss0) == float(loss1)
