"""Online degradation for interpolated-input and Y-channel models, the parts that need no GPU: the constructor's rules, the
LR window behind a tile, the tap arithmetic of the tile kernel restated in numpy against Pillow, and the entry points' checks of
their records (which launch nothing, so they run here)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sisr_amd
from conftest import GOLDEN
from _interp_online import D, data, origin_pairs, pillow_upsample, window_upsample_host

HR_DIR = os.path.join(GOLDEN, "set5", "hr")


@pytest.fixture
def small_pca(monkeypatch):
    real = D.pca_matrix
    monkeypatch.setattr(D, "pca_matrix", lambda batch=2000, k=10: real(batch=2000, k=k))


def _dataset(**kw):
    return data.SuperResImages(hr_dir=HR_DIR, online_degradations=True, split="all", **kw)


def test_constructor_accepts_interp_and_ycbcr_with_online_degradations(small_pca):
    """Both raised NotImplementedError before this feature."""
    params = {"degradation_scale": 4}
    ds = _dataset(input="interp", scale=1, online_degradation_params=params)
    assert ds.degrader.interp and ds.degrader.scale == 4 and ds.scale == 1 and ds.degrader.lr_form() == "rgb"
    ds = _dataset(input="interp", scale=1, colorspace="ycbcr", online_degradation_params=params)
    assert ds.degrader.interp and ds.degrader.scale == 4 and ds.degrader.lr_form() == "y"
    ds = _dataset(input="interp", scale=1, colorspace="ycbcr", y_only=False, online_degradation_params=params)
    assert ds.degrader.lr_form() == "ycbcr"
    ds = _dataset(input="unmodified", scale=4, colorspace="ycbcr")
    assert not ds.degrader.interp and ds.degrader.scale == 4 and ds.degrader.lr_form() == "y"
    ds = _dataset(input="interp", scale=3)  # default factor: the data set's scale when that is above 1
    assert ds.degrader.interp and ds.degrader.scale == 3
    assert ds.metadata_keys == ["blur_kernel"] * 10  # metadata keys are unchanged


def test_constructor_refusals(small_pca):
    with pytest.raises(ValueError, match="degradation_scale"):
        _dataset(input="interp", scale=1)
    with pytest.raises(ValueError, match="degradation_scale"):
        _dataset(input="interp", scale=1, online_degradation_params={"degradation_scale": 2.5})
    with pytest.raises(ValueError, match="degradation_scale"):  # LR / HR crops are paired by `scale`
        _dataset(input="unmodified", scale=4, online_degradation_params={"degradation_scale": 2})
    with pytest.raises(NotImplementedError, match="conv_type"):
        _dataset(input="interp", scale=1, colorspace="ycbcr", conv_type="png", online_degradation_params={"degradation_scale": 4})
    with pytest.raises(NotImplementedError, match="conv_type"):
        _dataset(input="unmodified", scale=4, colorspace="ycbcr", conv_type="png")


def test_interp_window_covers_every_tap_inside_the_image():
    """LR sides 5..40, factors 2, 3, 4, tile edges 8 and 20, every tile origin."""
    seen = refused = 0
    for s in (2, 3, 4):
        for c in (8, 20):
            edge = D.interp_window_edge(c, s)
            assert edge == (c - 1) // s + 5 <= -(-c // s) + 5
            for h in range(5, 41):
                if h * s < c:
                    with pytest.raises(ValueError, match="leaves"):
                        D.interp_window(h, s, c, 0)
                    continue
                if h < edge:  # refused as an LR image smaller than the tile is
                    with pytest.raises(ValueError, match="smaller"):
                        D.interp_window(h, s, c, 0)
                    refused += 1
                    continue
                bounds = D.pil_bicubic_table(h, h * s)[0]
                for T in range(h * s - c + 1):
                    w0, e = D.interp_window(h, s, c, T)
                    assert e == edge and 0 <= w0 and w0 + e <= h
                    first = bounds[T:T + c, 0]
                    assert first.min() >= w0 and (first + bounds[T:T + c, 1]).max() <= w0 + e, (s, c, h, T)
                    seen += 1
                with pytest.raises(ValueError, match="leaves"):
                    D.interp_window(h, s, c, h * s - c + 1)
    assert seen > 10000 and refused > 0
    assert D.interp_window(9, 4, 20, 16) == (0, 9)  # the 9-row LR image of the GPU tests is the window itself


@pytest.mark.parametrize("h,w", [(9, 11), (31, 20), (25, 17)])
def test_two_passes_on_a_window_with_whole_image_tables_equal_pillow_cropped(h, w):
    """The arithmetic of sisr_upsample_tiles in numpy: whole-image tables indexed at the tile's absolute rows and columns, tap
    addresses relative to the window -- against a crop of Pillow's resize of the whole LR image."""
    lr = np.random.default_rng(h * w).integers(0, 256, (3, h, w), dtype=np.uint8)
    cases = 0
    for s in (2, 3, 4):
        up = pillow_upsample(lr, s)
        for c in (8, 20):
            if min(h, w) < D.interp_window_edge(c, s):
                continue
            for ty, tx in origin_pairs(h * s, w * s, c, s):
                (wy, e), (wx, _) = D.interp_window(h, s, c, ty), D.interp_window(w, s, c, tx)
                got = window_upsample_host(lr[:, wy:wy + e, wx:wx + e], h, w, s, wy, wx, ty, tx, c)
                np.testing.assert_array_equal(got, up[:, ty:ty + c, tx:tx + c], err_msg=str((s, c, ty, tx)))
                cases += 1
    assert cases >= 100


def test_byte_over_255_times_255_truncates_back_to_the_byte():
    """Why the fp32 LR image may stand in for its bytes: ToPILImage's `mul(255).byte()` of ToTensor's b / 255 is b."""
    b = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(b.float().div(255).mul(255).byte(), b)


def _rec(hip, a, **kw):
    """A valid record: LR 9 x 11 at x 4, window 6 x 6 at (0, 2), an 8-pixel tile at (3, 16)."""
    r = hip.UpsampleTile()
    for f in ("bounds_h", "coef_h", "bounds_v", "coef_v"):
        setattr(r, f, a)
    r.h, r.w, r.H, r.W, r.wy, r.wx, r.ty, r.tx, r.flips = 9, 11, 36, 44, 0, 2, 3, 16, 5
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_upsample_tiles_refuses_bad_records_before_any_device_call():
    """In the style of test_degrade_tiles_cpu.py: everything below must fail on the host copy of the records, before a pointer
    is dereferenced or a kernel launched -- there is no GPU here to launch on."""
    hip = sisr_amd.hip
    L = hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    ERR_ARG, ERR_UNSUPPORTED = -1, -4
    assert L.sisr_upsample_tile_bytes() == C.sizeof(hip.UpsampleTile)
    assert (D.interp_window(9, 4, 8, 3), D.interp_window(11, 4, 8, 16)) == ((0, 6), (2, 6))  # the valid record's window

    def run(rec, host=True, dev=a, win=a, out=a, ks=5, B=1, Cn=3, c=8, cw=6, form=0):
        recs = (hip.UpsampleTile * 1)(rec)
        return L.sisr_upsample_tiles(C.addressof(recs) if host else None, dev, win, out, ks, B, Cn, c, cw, form, None)

    assert run(_rec(hip, a), host=False) == ERR_ARG and run(_rec(hip, a), dev=None) == ERR_ARG
    assert run(_rec(hip, a), win=None) == ERR_ARG and run(_rec(hip, a), out=None) == ERR_ARG
    for f in ("bounds_h", "coef_h", "bounds_v", "coef_v"):
        assert run(_rec(hip, a, **{f: None})) == ERR_ARG
    assert run(_rec(hip, a), B=0) == ERR_ARG and run(_rec(hip, a), c=0) == ERR_ARG and run(_rec(hip, a), cw=0) == ERR_ARG
    assert run(_rec(hip, a, h=0)) == ERR_ARG and run(_rec(hip, a, W=-44)) == ERR_ARG
    assert run(_rec(hip, a, ty=29)) == ERR_ARG and run(_rec(hip, a, tx=37)) == ERR_ARG      # the tile leaves the 36 x 44 image
    assert run(_rec(hip, a, ty=-1)) == ERR_ARG
    assert run(_rec(hip, a, wy=4)) == ERR_ARG and run(_rec(hip, a, wx=-1)) == ERR_ARG       # the window leaves the LR image
    assert run(_rec(hip, a, wy=1)) == ERR_ARG                                               # row 3's first tap is LR row 0
    assert run(_rec(hip, a, wx=0)) == ERR_ARG and run(_rec(hip, a, wx=3)) == ERR_ARG        # columns 16..23 read LR columns 2..7
    assert run(_rec(hip, a), cw=5) == ERR_ARG                                               # six columns of taps
    assert run(_rec(hip, a, flips=8)) == ERR_ARG and run(_rec(hip, a, flips=-1)) == ERR_ARG
    assert run(_rec(hip, a), form=3) == ERR_ARG and run(_rec(hip, a), form=-1) == ERR_ARG
    assert run(_rec(hip, a), ks=17) == ERR_UNSUPPORTED and run(_rec(hip, a), ks=0) == ERR_ARG
    assert run(_rec(hip, a), Cn=1, form=2) == ERR_UNSUPPORTED and run(_rec(hip, a), Cn=1, form=1) == ERR_UNSUPPORTED
    assert run(_rec(hip, a), B=65536) == ERR_UNSUPPORTED
    assert run(_rec(hip, a, H=37)) == ERR_UNSUPPORTED and run(_rec(hip, a, W=33)) == ERR_UNSUPPORTED  # no one integer factor

    cv = L.sisr_rgb_to_ycbcr
    b2 = C.addressof((C.c_float * 64)())
    assert cv(None, b2, 1, 8, 1, None) == ERR_ARG and cv(a, None, 1, 8, 1, None) == ERR_ARG and cv(a, a, 1, 8, 1, None) == ERR_ARG
    assert cv(a, b2, 0, 8, 1, None) == ERR_ARG and cv(a, b2, 1, 0, 1, None) == ERR_ARG and cv(a, b2, 1, 8, 2, None) == ERR_ARG
    assert cv(a, b2, 65536, 8, 0, None) == ERR_UNSUPPORTED

    # the Python entries
    with pytest.raises(RuntimeError, match="HIP device"):
        D.upsample_tiles(torch.zeros(1, 3, 6, 6, dtype=torch.uint8), [(9, 11)], 4, [(0, 2)], [(3, 16)], 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        D.rgb_to_ycbcr(torch.zeros(3, 4, 4))
    with pytest.raises(ValueError, match="form"):
        D.upsample_tiles(torch.zeros(1, 3, 6, 6, dtype=torch.uint8), [(9, 11)], 4, [(0, 2)], [(3, 16)], 8, form="lab")


def test_tile_mode_refuses_a_factor_above_four(small_pca):
    ds = _dataset(input="interp", scale=1, random_crop=24, random_augments=True, online_degradation_params={"degradation_scale": 8})
    assert ds.degrader.scale == 8  # the whole-image modes take it
    loader = data.DeviceTileLoader.__new__(data.DeviceTileLoader)  # no device here: only the batch routine's own check is run
    loader.degraders = [ds.degrader]
    loader.sampler = type("S", (), {"crop": 24, "scale": 1, "hr": [torch.zeros(3, 64, 72)]})()
    with pytest.raises(ValueError, match="degradation_scale = 8"):
        loader._degraded_tile_batch([0])
