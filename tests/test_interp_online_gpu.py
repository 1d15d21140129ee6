"""Online degradation for interpolated-input and Y-channel models on a real MI355X (pytest -m gpu).  Every comparison is
exact.  The oracle is Pillow on the host: the interpolated image is `resize(BICUBIC)` of the LR bytes the EXISTING entry points
make, its colour forms are data.rgb_to_ycbcr on the host, a tile is cut out of them with gather_on_host (helpers:
tests/_interp_online.py)."""
import functools
import os
import random
import shutil

import numpy as np
import pytest
import torch

import sisr_amd
from conftest import GOLDEN
from _degrade_tiles import FLIPS, random_image, random_kernel, woman
from _interp_online import (D, data, expected_tile, host_form, origin_pairs, pillow_upsample, to_tensor_u8, window_upsample_host,
                            with_flips)

pytestmark = pytest.mark.gpu

FORMS = ("rgb", "y", "ycbcr")
WHOLE = [("r38x47", 4), ("r93x61", 3), ("r50x34", 2), ("r64x72", 8)]
SMALL = {4: "r38x47", 3: "r93x61", 2: "r50x34"}


@functools.lru_cache(maxsize=None)
def source(key):
    if key == "woman":
        return woman().cuda()
    H, W = (int(v) for v in key[1:].split("x"))
    return random_image(H, W, seed=H).cuda()


@functools.lru_cache(maxsize=None)
def noise_field(key):
    g = torch.Generator().manual_seed(91)
    return torch.randn((1,) + tuple(source(key).shape), generator=g)


def draw_of(key, l, noisy):
    """A degrader's draws with a fixed kernel and, with noise, a fixed level and host field."""
    return D.DegraderDraw(random_kernel(l, l), None, 0.03 if noisy else None, None, noise_field(key) if noisy else None, None)


def degrader(scale, noisy, form="rgb", interp=True):
    return D.OnlineDegrader(scale=scale, pca=torch.zeros(441, 10), noise=noisy, interp=interp, ycbcr=form != "rgb",
                            y_only=form == "y")


@functools.lru_cache(maxsize=None)
def lr_bytes(key, scale, l, noisy):
    """The existing path's LR bytes, stage by stage from the existing entry points -> (3, h, w) uint8 on the host."""
    hr, d = source(key), draw_of(key, l, noisy)
    if noisy:
        _, blurred = D.blur_quant(hr, d.kernel, want_float=True, want_u8=False)
        u8 = D.noise_quant(blurred, d.level, field=d.field)
    else:
        u8 = D.blur_quant(hr, d.kernel)
    top, left, rh, rw = D.center_crop_box(hr.shape[1], hr.shape[2], scale)
    return D.pil_bicubic_downsample(u8[:, top:top + rh, left:left + rw].contiguous(), scale, to_float=False).cpu()


@functools.lru_cache(maxsize=None)
def interpolated(key, scale, l, noisy):
    """Pillow's resize(BICUBIC) of those bytes through ToTensor: the whole interpolated image, on the host, computed once."""
    return to_tensor_u8(pillow_upsample(lr_bytes(key, scale, l, noisy).numpy(), scale))


@pytest.mark.parametrize("noisy", [False, True])
@pytest.mark.parametrize("l", [21, 7])
@pytest.mark.parametrize("key,scale", WHOLE)
def test_whole_image_path_equals_pillow_and_the_data_sets_colour_conversion(key, scale, l, noisy):
    hr, d = source(key), draw_of(key, l, noisy)
    want = interpolated(key, scale, l, noisy)
    box = D.center_crop_box(hr.shape[1], hr.shape[2], scale)
    assert tuple(want.shape[1:]) == box[2:]
    for form in FORMS:
        got, got_box = degrader(scale, noisy, form).apply(hr, d)
        assert got_box == box
        assert torch.equal(got.cpu(), host_form(want, form)), form
    # input = 'unmodified' under 'ycbcr': the LR image itself, converted
    lr = to_tensor_u8(lr_bytes(key, scale, l, noisy))
    for form in FORMS:
        got, _ = degrader(scale, noisy, form, interp=False).apply(hr, d)
        assert torch.equal(got.cpu(), host_form(lr, form)), form


def test_device_colour_conversion_equals_the_data_sets_on_every_byte_triple_that_matters():
    """sisr_rgb_to_ycbcr against data.rgb_to_ycbcr on byte images: every (R, G) pair with a B that sweeps all 256 values, and
    a random fp32 batch."""
    r, g = torch.meshgrid(torch.arange(256), torch.arange(256), indexing="ij")
    b = (r * 7 + g * 13) % 256
    img = torch.stack([r, g, b]).float().div(255)
    for y_only in (True, False):
        assert torch.equal(D.rgb_to_ycbcr(img.cuda(), y_only).cpu(), data.rgb_to_ycbcr(img, y_only=y_only))
    batch = torch.rand(3, 3, 17, 23, generator=torch.Generator().manual_seed(2))
    got = D.rgb_to_ycbcr(batch.cuda(), False).cpu()
    assert torch.equal(got, torch.stack([data.rgb_to_ycbcr(im, y_only=False) for im in batch]))


def tile_samples(scale, c):
    """One batch: the small source of this factor (its LR window clamps on every side) and woman.png, every origin class,
    all eight flips."""
    out = []
    for key in (SMALL[scale], "woman"):
        _, H, W = interpolated(key, scale, 21, False).shape
        out += [(key, o, fl) for o, fl in with_flips(origin_pairs(H, W, c, scale))]
    return out


@pytest.mark.parametrize("c", [8, 20])
@pytest.mark.parametrize("scale", [2, 3, 4])
def test_tiles_equal_crops_of_the_whole_interpolated_image(scale, c):
    samples = tile_samples(scale, c)
    assert {s[2] for s in samples} == set(FLIPS) and len({s[0] for s in samples}) == 2
    wins, sizes, w_or, t_or, flips = [], [], [], [], []
    for key, (ty, tx), fl in samples:
        lr = lr_bytes(key, scale, 21, False)
        _, h, w = lr.shape
        (wy, e), (wx, _) = D.interp_window(h, scale, c, ty), D.interp_window(w, scale, c, tx)
        wins.append(lr[:, wy:wy + e, wx:wx + e])
        sizes.append((h, w)), w_or.append((wy, wx)), t_or.append((ty, tx)), flips.append(fl)
    win = torch.stack(wins).cuda()
    if scale == 4:
        assert lr_bytes("r38x47", 4, 21, False).shape == (3, 9, 11)
    for form in FORMS:
        got = D.upsample_tiles(win, sizes, scale, w_or, t_or, c, flips=flips, form=form)
        want = torch.stack([expected_tile(host_form(interpolated(key, scale, 21, False), form), ty, tx, c, fl)
                            for key, (ty, tx), fl in samples])
        assert got.shape == want.shape and torch.equal(got.cpu(), want), form
        assert torch.equal(D.upsample_tiles(win, sizes, scale, w_or, t_or, c, flips=flips, form=form), got)  # a repeat call
    one = D.upsample_tiles(win[3:4], sizes[3:4], scale, w_or[3:4], t_or[3:4], c, flips=flips[3:4])   # B = 1
    assert torch.equal(one.cpu(), expected_tile(interpolated(samples[3][0], scale, 21, False), *samples[3][1], c, samples[3][2])[None])


def test_tile_edges_that_are_no_multiple_of_four_or_of_the_block_and_grey_sources():
    """c = 70 spans three 32-pixel blocks and c = 13 is no multiple of 4 (the scalar stores); a grey (C = 1) window is
    written as it is."""
    lr = lr_bytes("woman", 4, 21, False)
    _, h, w = lr.shape
    up = interpolated("woman", 4, 21, False)
    for c in (70, 13):
        samples = [(o, fl) for o, fl in with_flips(origin_pairs(h * 4, w * 4, c, 4))][:24]
        win_o = [(D.interp_window(h, 4, c, ty)[0], D.interp_window(w, 4, c, tx)[0]) for (ty, tx), _ in samples]
        e = D.interp_window_edge(c, 4)
        win = torch.stack([lr[:, wy:wy + e, wx:wx + e] for wy, wx in win_o]).cuda()
        args = ([(h, w)] * len(samples), 4, win_o, [s[0] for s in samples], c)
        for form in FORMS:
            got = D.upsample_tiles(win, *args, flips=[s[1] for s in samples], form=form)
            want = torch.stack([expected_tile(host_form(up, form), ty, tx, c, fl) for (ty, tx), fl in samples])
            assert torch.equal(got.cpu(), want), (c, form)
        grey = D.upsample_tiles(win[:, 1:2].contiguous(), *args, flips=[s[1] for s in samples])
        assert grey.shape[1] == 1
        assert torch.equal(grey.cpu(), torch.stack([expected_tile(up[1:2], ty, tx, c, fl) for (ty, tx), fl in samples]))


# ------------------------------------------------------------------------------------------------ the three loaders
@pytest.fixture
def two_images(tmp_path):
    d = tmp_path / "hr"
    d.mkdir()
    for f in ("butterfly.png", "woman.png"):
        shutil.copy(os.path.join(GOLDEN, "set5", "hr", f), d / f)
    return str(d)


def _dataset(monkeypatch, hr_dir, **kw):
    real = D.pca_matrix
    monkeypatch.setattr(D, "pca_matrix", lambda batch=2000, k=10: real(batch=2000, k=k))
    np.random.seed(5)
    kw.setdefault("scale", 1)
    kw.setdefault("input", "interp")
    params = dict(kw.pop("params", {}))
    if kw["input"] == "interp":
        params.setdefault("degradation_scale", 4)
    return data.SuperResImages(hr_dir=hr_dir, online_degradations=True, split="all", random_crop=24, random_augments=True,
                               online_degradation_params=params, **kw)


def _seed():
    torch.manual_seed(3)
    np.random.seed(6)
    random.seed(7)


def _streams():
    return np.random.random(), random.random(), float(torch.rand(1))


def _same(a, b, lr_too=True):
    assert set(a) == set(b)
    assert list(a["tag"]) == list(b["tag"]) and list(a["hr_tag"]) == list(b["hr_tag"])
    assert torch.equal(a["hr"].cpu(), b["hr"].cpu()) and (not lr_too or torch.equal(a["lr"].cpu(), b["lr"].cpu()))
    assert a["lr"].shape == b["lr"].shape and a["lr"].dtype == b["lr"].dtype == torch.float32
    assert torch.equal(a["metadata"], b["metadata"]) and a["metadata"].dtype == b["metadata"].dtype
    assert torch.equal(a["blur_kernels"], b["blur_kernels"])
    assert [tuple(k) for k in a["metadata_keys"]] == [tuple(k) for k in b["metadata_keys"]]
    assert torch.equal(torch.as_tensor(a["mask"]), b["mask"]) and torch.equal(torch.as_tensor(a["halfway_data"]), b["halfway_data"])


def _three_loaders(monkeypatch, hr_dir, **kw):
    from torch.utils.data import DataLoader
    dev = torch.device("cuda:0")
    host = DataLoader(dataset=_dataset(monkeypatch, hr_dir, **kw), batch_size=2, shuffle=True, num_workers=0)
    whole = data.DeviceTileLoader([_dataset(monkeypatch, hr_dir, **kw)], 2, dev)
    tiles = data.DeviceTileLoader([_dataset(monkeypatch, hr_dir, **kw)], 2, dev, degrade_tiles=True)
    out, streams = [], []
    for loader in (host, whole, tiles):
        _seed()
        out.append(list(loader))
        streams.append(_streams())
    assert streams[0] == streams[1] == streams[2]  # the same draws were consumed
    assert len(out[0]) == len(out[1]) == len(out[2]) == 1
    return out, tiles


@pytest.mark.parametrize("colorspace,input", [("rgb", "interp"), ("ycbcr", "interp"), ("ycbcr", "unmodified")])
def test_three_loaders_give_the_same_epoch(monkeypatch, two_images, colorspace, input):
    kw = dict(colorspace=colorspace, input=input)
    if input == "unmodified":
        kw["scale"] = 4
    (host, whole, tiles), _ = _three_loaders(monkeypatch, two_images, **kw)
    ch, hr_edge = (1 if colorspace == "ycbcr" else 3), (96 if input == "unmodified" else 24)
    for a, b, c in zip(host, whole, tiles):
        _same(a, b)
        _same(a, c)
        assert tuple(c["lr"].shape) == (2, ch, 24, 24) and tuple(c["hr"].shape) == (2, ch, hr_edge, hr_edge)
        assert c["lr"].is_cuda and c["hr"].is_cuda
        assert tuple(c["metadata"].shape) == (2, 10)


def test_three_loaders_with_jpeg(monkeypatch, two_images):
    """The two whole-image modes agree; the tile mode's `lr` is the host composition on the WINDOW: interp_window, the JPEG round
    trip of its bytes (block grid at the window's origin), Pillow's two passes with whole-image tables, the colour form, the flips."""
    params = {"jpeg": True, "jpeg_quality": [30, 95]}
    (host, whole, got), tiles = _three_loaders(monkeypatch, two_images, colorspace="ycbcr", params=params)
    _same(host[0], whole[0])
    _same(host[0], got[0], lr_too=False)
    assert tuple(got[0]["metadata"].shape) == (2, 11)
    # replay the draws by hand
    _seed()
    torch.empty((), dtype=torch.int64).random_()
    g = torch.Generator()
    g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
    idx = torch.randperm(2, generator=g).tolist()
    ds = [tiles.degraders[i].draw() for i in idx]
    crops = []
    for i in idx:
        hr = tiles.sampler.hr[i]
        _, _, rh, rw = D.center_crop_box(hr.shape[1], hr.shape[2], 4)
        crops.append(tiles.sampler.draw_for(torch.empty(0, rh, rw)))
    for k, (i, d, (top, left, hf, vf, rot)) in enumerate(zip(idx, ds, crops)):
        hr = tiles.sampler.hr[i]
        t0, l0, rh, rw = D.center_crop_box(hr.shape[1], hr.shape[2], 4)
        h, w = rh // 4, rw // 4
        ty, tx = data.tile_source_box(rh, rw, 24, top, left, hf, vf, rot)
        (wy, e), (wx, _) = D.interp_window(h, 4, 24, ty), D.interp_window(w, 4, 24, tx)
        u8 = D.blur_quant(hr, d.kernel)[:, t0:t0 + rh, l0:l0 + rw].contiguous()
        lr = D.pil_bicubic_downsample(u8, 4, to_float=False).cpu().numpy()
        win = D.jpeg_roundtrip_host(lr[:, wy:wy + e, wx:wx + e], d.quality)
        tile = host_form(to_tensor_u8(window_upsample_host(win, h, w, 4, wy, wx, ty, tx, 24)), "y")
        want = expected_tile(tile, 0, 0, 24, (hf, vf, rot))
        assert torch.equal(got[0]["lr"][k].cpu(), want), (i, d.quality)
        assert torch.equal(d.kernel, got[0]["blur_kernels"][k]) and torch.equal(d.code, got[0]["metadata"][k])


# ------------------------------------------------------------------------------------------------ one epoch of train_sisr
def _train_config(tmp_path, hr_dir, model, crop):
    sets = {"name": None, "lr": None, "hr": hr_dir, "cutoff": 2, "online_degradations": True,  # (a cutoff keeps the split's name,
            "online_degradation_params": {"degradation_scale": 4}}                           # which decides Y alone or YCbCr)
    ev = tmp_path / "eval_hr"  # small validation images: 32 x 32 corners of the two training images
    ev.mkdir()
    from PIL import Image
    for f in sorted(os.listdir(hr_dir)):
        Image.open(os.path.join(hr_dir, f)).convert("RGB").crop((0, 0, 32, 32)).save(ev / f)
    return {"experiment": "interp_online", "experiment_save_loc": str(tmp_path),
            "data": {"batch_size": 2, "dataloader_threads": 0, "device_tiles": True, "degrade_tiles": True,
                     "training_sets": {"data_1": dict(sets, crop=crop, random_augment=True)},
                     "eval_sets": {"data_1": dict(sets, hr=str(ev))}},
            "model": model,
            "training": {"gpu": "single", "sp_gpu": 0, "seed": 8, "num_epochs": 1, "metrics": ["PSNR"], "logging": "text",
                         "save_samples": False}}


@pytest.fixture
def small_pca(monkeypatch):
    real = D.pca_matrix
    monkeypatch.setattr(D, "pca_matrix", lambda batch=2000, k=10: real(batch=2000, k=k))


def test_one_epoch_of_a_reduced_vdsr_on_tile_level_y_batches(tmp_path, two_images, small_pca, monkeypatch):
    model = {"name": "vdsr", "internal_params": {"scale": 1, "lr": 1e-4, "kernel_pattern": [3] * 4,
                                                 "channel_pattern": [1, 64, 64, 64, 1]}}
    shapes = []
    real = data.DeviceTileLoader._degraded_tile_batch

    def spy(self, idx):
        b = real(self, idx)
        shapes.append((tuple(b["lr"].shape), tuple(b["hr"].shape)))
        return b
    monkeypatch.setattr(data.DeviceTileLoader, "_degraded_tile_batch", spy)
    total = sisr_amd.cli.train_sisr(_train_config(tmp_path, two_images, model, 24))
    assert shapes == [((2, 1, 24, 24), (2, 1, 24, 24))]
    assert list(total["epoch"]) == [0]
    for key in ("train-loss", "val-loss", "val-PSNR"):
        assert len(total[key]) == 1 and np.isfinite(total[key]).all(), (key, total[key])


def test_one_epoch_of_a_reduced_qsparnet_gets_the_degraders_codes(tmp_path, two_images, small_pca, monkeypatch):
    cfg = dict(min_ch=32, max_ch=128, in_size=32, out_size=32, min_feat_size=8, res_depth=1, bottleneck_size=16)
    model = {"name": "qsparnet", "internal_params": dict(cfg, scale=1, lr=1e-4, metadata=["blur_kernel"])}
    codes, seen = [], []
    real_draw = D.OnlineDegrader.draw

    def draw(self, field_shape=None):
        d = real_draw(self, field_shape)
        if field_shape is None:  # the tile mode's draws (validation goes through the whole-image path)
            codes.append(d.code.clone())
        return d
    monkeypatch.setattr(D.OnlineDegrader, "draw", draw)
    real_train = sisr_amd.sparnet.QSPARNetHandler.run_train

    def run_train(self, x, y, metadata=None, **kw):
        seen.append((tuple(x.shape), torch.as_tensor(metadata).clone()))
        return real_train(self, x, y, metadata=metadata, **kw)
    monkeypatch.setattr(sisr_amd.sparnet.QSPARNetHandler, "run_train", run_train)
    total = sisr_amd.cli.train_sisr(_train_config(tmp_path, two_images, model, 32))
    assert len(seen) == 1 and seen[0][0] == (2, 3, 32, 32) and len(codes) == 2
    assert torch.equal(seen[0][1].float().cpu().reshape(2, -1), torch.stack(codes))
    for key in ("train-loss", "val-loss", "val-PSNR"):
        assert len(total[key]) == 1 and np.isfinite(total[key]).all(), (key, total[key])
