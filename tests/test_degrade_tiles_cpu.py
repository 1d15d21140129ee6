"""Tile-level online degradation (`[data] degrade_tiles = true`), the parts that need no GPU: tile geometry, the split of
OnlineDegrader into draws and pixel work, the Philox words of the noise field's numpy mirror, argument refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sisr_amd
from conftest import GOLDEN
from _degrade_tiles import FLIPS, PHILOX_KAT, D, data, draw_for_origin, gather_on_host


@pytest.mark.parametrize("hf,vf,rot", FLIPS)
def test_tile_source_box_is_the_origin_of_what_the_index_map_reads(hf, vf, rot):
    h, w, c = 9, 13, 4
    img = (torch.arange(h).view(h, 1) * 100 + torch.arange(w).view(1, w))[None]  # value = 100 row + column
    ah, aw = (w, h) if rot else (h, w)
    for top in (0, 2, ah - c):          # origins at 0, inside and at the far edge of the augmented image
        for left in (0, 3, aw - c):
            got = gather_on_host(img, (h, w, top, left, hf, vf, rot), c)[0]
            sy, sx = got // 100, got % 100
            ty, tx = data.tile_source_box(h, w, c, top, left, hf, vf, rot)
            assert (ty, tx) == (int(sy.min()), int(sx.min()))
            assert int(sy.max()) == ty + c - 1 and int(sx.max()) == tx + c - 1          # a c x c square
            assert draw_for_origin(h, w, c, ty, tx, hf, vf, rot) == (top, left)
            # the tile-local map the kernels store through (include/sisr_hip.h, sisr_degrade_tile.flips)
            i = torch.arange(c).view(c, 1).expand(c, c)
            j = torch.arange(c).view(1, c).expand(c, c)
            a, b = (j, i) if rot else (i, j)
            ry, rx = (c - 1 - a if vf else a), (c - 1 - b if hf else b)
            assert torch.equal(sy, ty + ry) and torch.equal(sx, tx + rx)
    with pytest.raises(ValueError):
        data.tile_source_box(h, w, c, ah - c + 1, 0, hf, vf, rot)


def _old_call_draws(deg, shape):
    """The draws of OnlineDegrader.__call__ as it stood before the split, in its order (degrade.py: kernel, noise level and
    mask, the host field, the quality)."""
    kernel = deg.draw_kernel()
    code = D.encode_kernel(kernel, deg.pca)
    field = q = None
    if deg.noise:
        level = torch.FloatTensor(D.random_batch_noise(1, deg.noise_high, deg.rate_cln))
        field = torch.FloatTensor(np.random.normal(loc=0.0, scale=1.0, size=(1,) + shape))
        code = torch.cat([code, (level * 10).view(-1)])
    if deg.jpeg:
        q = int(np.random.randint(deg.jpeg_lo, deg.jpeg_hi + 1))
        a, b = deg.jpeg_norm
        code = torch.cat([code, torch.tensor([(q - a) / (b - a)], dtype=torch.float32)])
    return kernel, code, field, q


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("jpeg", [False, True])
def test_draw_consumes_numpy_as_the_call_did(noise, jpeg, monkeypatch):
    pca = torch.linspace(-1, 1, 441 * 10).view(441, 10)
    deg = D.OnlineDegrader(scale=4, pca=pca, noise=noise, jpeg=jpeg, rate_cln=0.5)
    shape = (3, 12, 10)
    np.random.seed(31)
    want = [_old_call_draws(deg, shape) for _ in range(3)]
    want_state = np.random.get_state()
    np.random.seed(31)
    got = [deg.draw(field_shape=shape) for _ in range(3)]
    state = np.random.get_state()
    assert state[0] == want_state[0] and np.array_equal(state[1], want_state[1]) and state[2:] == want_state[2:]
    for (kernel, code, field, q), d in zip(want, got):
        assert torch.equal(kernel, d.kernel) and torch.equal(code, d.code) and q == d.quality and d.seed is None
        assert (field is None and d.field is None) or torch.equal(field, d.field)
        assert (d.level is not None) == noise and (not noise or abs(d.level * 10 - float(code[10])) < 1e-6)
    # __call__ = draw + apply: the same stream with the pixel work stubbed out (it draws nothing)
    seen = []
    monkeypatch.setattr(deg, "apply", lambda hr, d: (seen.append(d), ("lr", (0, 0, 12, 8)))[1])
    np.random.seed(31)
    outs = [deg(torch.zeros(shape)) for _ in range(3)]
    state = np.random.get_state()
    assert np.array_equal(state[1], want_state[1]) and state[2:] == want_state[2:]
    for (kernel, code, field, q), out, d in zip(want, outs, seen):
        assert torch.equal(out[1], code) and torch.equal(out[2], kernel) and d.quality == q
    # the tile-level draw: the field is replaced by ONE randint (the seed), right after random_batch_noise's two draws
    np.random.seed(31)
    d = deg.draw()
    np.random.seed(31)
    kernel = deg.draw_kernel()
    if noise:
        D.random_batch_noise(1, deg.noise_high, deg.rate_cln)
        seed = int(np.random.randint(0, 1 << 32, dtype=np.int64))
        assert d.seed == seed and 0 <= seed < 1 << 32 and d.field is None
    if jpeg:
        assert d.quality == int(np.random.randint(deg.jpeg_lo, deg.jpeg_hi + 1))
    assert torch.equal(d.kernel, kernel) and np.random.random() == (np.random.seed(31), deg.draw(), np.random.random())[2]


def test_philox_known_answers():
    for ctr, key, want in PHILOX_KAT:
        got = D.philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert [int(v) for v in got] == list(want), [hex(int(v)) for v in got]
    # batched, and as the field uses it: counter = (column >> 2, row, channel, 0), key = (seed, 0)
    words = D.normal_field_words_host(0xa4093822, 2, 3, 10)
    assert words.shape == (2, 3, 3, 4) and words.dtype == np.uint32
    one = D.philox4x32_10(np.array([2, 1, 1, 0], np.uint32), np.array([0xa4093822, 0], np.uint32))
    assert np.array_equal(words[1, 1, 2], one)
    assert np.array_equal(D.normal_field_words_host(0, 1, 1, 1)[0, 0, 0], np.array(PHILOX_KAT[0][2], np.uint32))


def test_normal_field_host_maps_words_to_pixels_as_documented():
    seed, Cn, H, W = 12345, 2, 3, 7
    words = D.normal_field_words_host(seed, Cn, H, W)
    f = D.normal_field_host(seed, Cn, H, W)
    assert f.shape == (Cn, H, W) and f.dtype == np.float64
    for (c, y, x) in [(0, 0, 0), (1, 2, 1), (0, 1, 2), (1, 0, 3), (0, 2, 6), (1, 1, 5)]:
        w = words[c, y, x >> 2]
        pair = (x >> 1) & 1
        u = [np.float64((np.float32(int(v) >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)) for v in (w[2 * pair], w[2 * pair + 1])]
        r, a = np.sqrt(-2 * np.log(u[0])), 2 * np.pi * u[1]
        assert f[c, y, x] == (r * np.sin(a) if x & 1 else r * np.cos(a))
    big = D.normal_field_host(7, 3, 64, 64)
    assert np.isfinite(big).all() and abs(big.mean()) < 0.05 and abs(big.var() - 1) < 0.07  # 5 standard errors at n = 12 288
    assert not np.array_equal(big, D.normal_field_host(8, 3, 64, 64))


def _rec(hip, a, **kw):
    """A valid record of a 38 x 47 image at x 4 (crop box offset (1, 2), LR 9 x 11) with stand-in pointers."""
    r = hip.DegradeTile()
    for f in ("image", "bounds_h", "coef_h", "bounds_v", "coef_v"):
        setattr(r, f, a)
    r.H, r.W, r.t0, r.l0, r.rh, r.rw, r.ty, r.tx, r.ksize_h, r.ksize_v = 38, 47, 1, 2, 36, 44, 1, 3, 17, 17
    r.sigma = 0.03
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_tile_entries_refuse_bad_arguments_before_any_device_call():
    """In the style of test_abi.py::test_round4_entry_points_refuse_bad_arguments_before_any_device_call: everything below
    must fail on the host, before a pointer is dereferenced or a kernel launched (this runs without a GPU)."""
    hip = sisr_amd.hip
    L = hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    ERR_ARG, ERR_UNSUPPORTED = -1, -4
    assert L.sisr_degrade_tile_bytes() == C.sizeof(hip.DegradeTile)

    def run(rec, B=1, Cn=3, c=8, l=21, scale=4, to_float=1, host=True, dev=a, k=a, out=a):
        recs = (hip.DegradeTile * 1)(rec)
        return L.sisr_degrade_tiles(C.addressof(recs) if host else None, dev, k, out, B, Cn, c, l, scale, to_float, None)

    assert run(_rec(hip, a), host=False) == ERR_ARG and run(_rec(hip, a), dev=None) == ERR_ARG       # null record arrays
    assert run(_rec(hip, a), k=None) == ERR_ARG and run(_rec(hip, a), out=None) == ERR_ARG
    assert run(_rec(hip, a), B=0) == ERR_ARG and run(_rec(hip, a), c=0) == ERR_ARG and run(_rec(hip, a), to_float=2) == ERR_ARG
    assert run(_rec(hip, a, image=None)) == ERR_ARG
    for f in ("bounds_h", "coef_h", "bounds_v", "coef_v"):
        assert run(_rec(hip, a, **{f: None})) == ERR_ARG                                             # tables not supplied
    assert run(_rec(hip, a, rh=27, rw=33, ksize_h=13, ksize_v=13), scale=4) == ERR_ARG                # x 3's tables at x 4
    assert run(_rec(hip, a), c=9) == ERR_ARG                                                         # ty + c > h = 9
    assert run(_rec(hip, a, ty=0), c=10) == ERR_ARG and run(_rec(hip, a, tx=4)) == ERR_ARG           # c > h; tx + c > w = 11
    assert run(_rec(hip, a, ty=-1)) == ERR_ARG and run(_rec(hip, a, flips=8)) == ERR_ARG
    assert run(_rec(hip, a, t0=3)) == ERR_ARG and run(_rec(hip, a, rh=35)) == ERR_ARG                # box outside / not 4 k
    assert run(_rec(hip, a, sigma=-0.1)) == ERR_ARG
    assert run(_rec(hip, a), l=22) == ERR_UNSUPPORTED and run(_rec(hip, a), l=0) == ERR_ARG
    assert run(_rec(hip, a, H=10, t0=0, rh=8, ty=0), c=2) == ERR_UNSUPPORTED                         # l / 2 = 10 >= H
    assert run(_rec(hip, a), scale=5) == ERR_UNSUPPORTED and run(_rec(hip, a), scale=1) == ERR_UNSUPPORTED
    big = _rec(hip, a, H=4000, W=4000, t0=0, l0=0, rh=4000, rw=4000, ty=0, tx=0)
    assert run(big, c=512) == ERR_UNSUPPORTED                                                        # window beyond the LDS

    jp = L.sisr_jpeg_roundtrip_batch
    b2 = C.addressof((C.c_float * 64)())
    assert jp(None, b2, a, a, 1, 3, 8, 1, None) == ERR_ARG and jp(a, None, a, a, 1, 3, 8, 1, None) == ERR_ARG
    assert jp(a, b2, None, a, 1, 3, 8, 1, None) == ERR_ARG and jp(a, a, a, a, 1, 3, 8, 1, None) == ERR_ARG    # in place
    assert jp(a, b2, a, a, 0, 3, 8, 1, None) == ERR_ARG and jp(a, b2, a, a, 1, 2, 8, 1, None) == ERR_ARG
    assert jp(a, b2, a, a, 1, 3, 0, 1, None) == ERR_ARG and jp(a, b2, a, a, 1, 3, 8, 2, None) == ERR_ARG
    assert jp(a, b2, a, a, 70000, 3, 8, 1, None) == ERR_UNSUPPORTED

    nf = L.sisr_normal_field
    assert nf(1, None, None, 3, 8, 8, None) == ERR_ARG and nf(1, a, None, 0, 8, 8, None) == ERR_ARG
    assert nf(1, a, None, 3, 0, 8, None) == ERR_ARG and nf(1, a, None, 3, 8, -1, None) == ERR_ARG

    cs = L.sisr_crop_augment_strided
    prm = (C.c_int * 12)(36, 44, 0, 0, 0, 0, 0, 38, 47, 1, 2, 0)
    p = C.addressof(prm)
    assert cs(None, p, a, a, 1, 3, 32, None) == ERR_ARG and cs(a, None, a, a, 1, 3, 32, None) == ERR_ARG
    assert cs(a, p, None, a, 1, 3, 32, None) == ERR_ARG and cs(a, p, a, None, 1, 3, 32, None) == ERR_ARG
    assert cs(a, p, a, a, 1, 3, 40, None) == ERR_ARG                                                 # 40 > rh = 36
    prm[9] = 3
    assert cs(a, p, a, a, 1, 3, 32, None) == ERR_ARG                                                 # box leaves the image

    # the Python entry: qualities are device values for the kernel, so they are refused here, before the upload
    img = [torch.zeros(3, 38, 47)]
    for q in (0, 101, 50.5, True):
        with pytest.raises(ValueError):
            D.degrade_tiles(img, np.zeros((1, 21, 21), np.float32), [(0, 0)], 8, 4, qualities=[q])
    with pytest.raises(ValueError):
        D.degrade_tiles(img, np.zeros((1, 21, 21), np.float32), [(0, 0)], 8, 4, sigmas=[0.1])       # noise without seeds
    with pytest.raises(RuntimeError, match="HIP device"):
        D.degrade_tiles(img, np.zeros((1, 21, 21), np.float32), [(0, 0)], 8, 4)                      # no CPU path
    with pytest.raises(RuntimeError, match="HIP device"):
        D.normal_field(1, 3, 8, 8, "cpu")
    with pytest.raises(ValueError):
        D.normal_field(1 << 32, 3, 8, 8, "cuda:0")


def test_degrade_tiles_needs_device_tiles_and_online_degradations():
    d = os.path.join(GOLDEN, "set5")
    sets = {"a": {"lr": os.path.join(d, "lr_random_blur"), "hr": os.path.join(d, "hr"), "crop": 24}}
    online = {"a": {"lr": None, "hr": os.path.join(d, "hr"), "crop": 24, "online_degradations": True}}
    with pytest.raises(ValueError, match="degrade_tiles"):
        data.sisr_data_setup(online, online, degrade_tiles=True, device_tiles=False, scale=4)
    with pytest.raises(ValueError, match="degrade_tiles"):
        data.sisr_data_setup(sets, sets, degrade_tiles=True, device_tiles=True, device="cuda:0", scale=4)
    ds = data.SuperResImages(lr_dir=sets["a"]["lr"], hr_dir=sets["a"]["hr"], split="all", scale=4, random_crop=24)
    with pytest.raises(ValueError, match="degrade_tiles"):
        data.DeviceTileLoader([ds], 2, "cpu", degrade_tiles=True)
