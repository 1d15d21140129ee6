"""Tile-level online degradation on a real MI355X (pytest -m gpu): every tile equals, bit for bit, what the EXISTING
whole-image entry points give at its position (helpers and expectations: tests/_degrade_tiles.py)."""
import functools
import os
import random

import numpy as np
import pytest
import torch

import sisr_amd
from conftest import GOLDEN
from _degrade_tiles import (FLIPS, D, data, draw_for_origin, gather_on_host, origins_for, random_image, random_kernel,
                            whole_image_lr, woman)

pytestmark = pytest.mark.gpu

# case -> (source image, scale, tile edge).  38 x 47 at x 4 has its crop box at (1, 2) and an LR image of 9 x 11: the halo exceeds
# the image on every side; every case lies within one halo of a border, where a tile kernel goes wrong
CASES = {"r38x47": ("r38x47", 4, 8), "r93x61": ("r93x61", 3, 8), "r50x34": ("r50x34", 2, 8), "woman": ("woman", 4, 24),
         "woman8": ("woman", 4, 8), "woman20": ("woman", 4, 20), "grey8": ("grey", 4, 8), "grey24": ("grey", 4, 24),
         "grey20": ("grey", 4, 20)}


@functools.lru_cache(maxsize=None)
def source(key):
    if key == "woman":
        return woman().cuda()
    if key == "grey":
        return woman()[1:2].contiguous().cuda()
    H, W = (int(v) for v in key[1:].split("x"))
    return random_image(H, W, seed=H).cuda()


def image(name):
    return source(CASES[name][0])


def kernel(l):
    """l: the kernel's edge, or (edge, seed) for another kernel of that size."""
    return random_kernel(*l) if isinstance(l, tuple) else random_kernel(l, l)


@functools.lru_cache(maxsize=None)
def _reference(key, scale, l, sigma, seed):
    return whole_image_lr(source(key), kernel(l), scale, sigma, seed, to_float=False).cpu()


def reference(name, l, sigma, seed):
    """The whole-image LR image (uint8, on the host), computed once per (image, kernel, noise) and shared."""
    return _reference(CASES[name][0], CASES[name][1], l, sigma, seed)


def expected_tiles(samples, to_float, jpeg=None):
    """samples: (name, l, sigma, seed, (ty, tx), flips) -> the tiles cut from the whole-image references with the index map.
    jpeg: per-sample qualities -- jpeg_roundtrip of the un-augmented tile's bytes, then the gather."""
    out = []
    for n, (name, l, sigma, seed, (ty, tx), fl) in enumerate(samples):
        c = CASES[name][2]
        lr = reference(name, l, sigma, seed)
        _, h, w = lr.shape
        if jpeg is not None:
            tile = D.jpeg_roundtrip(lr[:, ty:ty + c, tx:tx + c].contiguous().cuda(), jpeg[n], to_float=False).cpu()
            t = gather_on_host(tile, (c, c) + draw_for_origin(c, c, c, 0, 0, *fl) + fl, c)
        else:
            top, left = draw_for_origin(h, w, c, ty, tx, *fl)
            t = gather_on_host(lr, (h, w, top, left) + fl, c)
        out.append(t.float().div(255) if to_float else t)
    return torch.stack(out)


def run(samples, to_float, jpeg=None):
    _, scale, c = CASES[samples[0][0]]
    noise = samples[0][2] is not None
    return D.degrade_tiles([image(s[0]) for s in samples], torch.stack([kernel(s[1]) for s in samples]),
                           [s[4] for s in samples], c, scale, flips=[s[5] for s in samples],
                           sigmas=[s[2] for s in samples] if noise else None, seeds=[s[3] for s in samples] if noise else None,
                           qualities=jpeg, to_float=to_float).cpu()


def lr_size(name):
    scale = CASES[name][1]
    _, _, rh, rw = D.center_crop_box(image(name).shape[1], image(name).shape[2], scale)
    return rh // scale, rw // scale


def all_samples(name, l, sigma, seed):
    """Every origin of origins_for x every flip / transpose combination, as one batch."""
    h, w = lr_size(name)
    return [(name, l, sigma, seed, o, fl) for o in origins_for(h, w, CASES[name][2]) for fl in FLIPS]


IMAGE_KERNEL = [("r38x47", 21), ("r38x47", 15), ("r38x47", 8), ("r93x61", 21), ("r93x61", 8), ("r50x34", 21), ("r50x34", 15),
                ("woman", 21), ("woman", 8)]


@pytest.mark.parametrize("to_float", [False, True])
@pytest.mark.parametrize("name,l", IMAGE_KERNEL)
def test_blur_and_resample_tiles_equal_the_whole_image_path(name, l, to_float):
    assert D.center_crop_box(38, 47, 4)[:2] == (1, 2) and lr_size("r38x47") == (9, 11)
    samples = all_samples(name, l, None, None)
    assert torch.equal(run(samples, to_float), expected_tiles(samples, to_float))            # B = 48
    assert torch.equal(run(samples[5:6], to_float), expected_tiles(samples[5:6], to_float))  # B = 1


@pytest.mark.parametrize("to_float", [False, True])
def test_a_batch_mixes_image_sizes_and_kernels(to_float):
    """B = 7 over two images of different size (both x 4, c = 8) and three different kernels."""
    samples = []
    for n in range(7):
        name = ("r38x47", "woman8")[n & 1]
        h, w = lr_size(name)
        samples.append((name, (15, n % 3), None, None, origins_for(h, w, 8)[n % 6], FLIPS[n]))
    assert torch.equal(run(samples, to_float), expected_tiles(samples, to_float))


@pytest.mark.parametrize("to_float", [False, True])
@pytest.mark.parametrize("sigma", [0.0, 0.03])
@pytest.mark.parametrize("name,l", IMAGE_KERNEL)
def test_noisy_tiles_equal_the_whole_image_chain_fed_the_same_field(name, l, sigma, to_float):
    samples = all_samples(name, l, sigma, 77 + l)
    got = run(samples, to_float)
    assert torch.equal(got, expected_tiles(samples, to_float))
    assert torch.equal(run(samples, to_float), got)  # the same call twice
    if sigma:
        assert not torch.equal(reference(name, l, sigma, 77 + l), reference(name, l, None, None))  # the noise did something


def test_seeds_are_per_sample():
    a = ("r38x47", 21, 0.03, 5, (1, 2), FLIPS[0])
    b = ("r38x47", 21, 0.03, 6, (1, 2), FLIPS[0])
    got = run([a, b, a], False)
    assert not torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    assert torch.equal(got, expected_tiles([a, b, a], False))


def test_noise_field_against_the_host_mirror():
    Cn, H, W = 3, 272, 272
    field, words = D.normal_field(20261, Cn, H, W, "cuda:0", words=True)
    field = field.cpu().numpy().astype(np.float64)
    assert np.array_equal(words.cpu().numpy().view(np.uint32), D.normal_field_words_host(20261, Cn, H, W))
    host = D.normal_field_host(20261, Cn, H, W)
    err = np.abs(field - host).max()
    print(f"normal_field: max |device - host mirror| = {err:.3e}, mean = {field.mean():.5f}, var = {field.var():.5f}")
    assert err < 2e-5
    assert abs(field.mean()) < 0.011 and abs(field.var() - 1) < 0.015
    # a width that is no multiple of 4, and a field read back twice
    f2, w2 = D.normal_field(3, 2, 5, 7, "cuda:0", words=True)
    assert np.array_equal(w2.cpu().numpy().view(np.uint32), D.normal_field_words_host(3, 2, 5, 7))
    assert np.abs(f2.cpu().numpy() - D.normal_field_host(3, 2, 5, 7)).max() < 2e-5
    assert torch.equal(f2, D.normal_field(3, 2, 5, 7, "cuda:0"))


@pytest.mark.parametrize("to_float", [False, True])
@pytest.mark.parametrize("c", [8, 24, 20])
@pytest.mark.parametrize("grey", [False, True])
def test_jpeg_tiles_equal_the_round_trip_of_the_tiles_bytes(c, grey, to_float):
    """One quality per sample, {1, 30, 95, 100} mixed in the batch; c = 20 is not a block multiple (edge replication)."""
    name = ("grey%d" if grey else "woman%d") % c if (grey or c != 24) else "woman"
    h, w = lr_size(name)
    samples = [(name, 21, None, None, origins_for(h, w, c)[n % 6], FLIPS[n]) for n in range(8)]
    q = [1, 30, 95, 100, 95, 1, 100, 30]
    assert torch.equal(run(samples, to_float, jpeg=q), expected_tiles(samples, to_float, jpeg=q))


def test_hr_tiles_equal_the_samplers_on_the_same_draws():
    """The strided gather from the full images against sample_pairs on contiguous copies of the centre crops, including the
    38 x 47 image whose crop box is offset by (1, 2)."""
    names = ["r38x47", "woman8", "r38x47", "woman8", "r38x47"]
    sm = data.DeviceTileSampler(None, [image(n) for n in names], scale=4, crop=8, device="cuda:0")
    boxes = [D.center_crop_box(image(n).shape[1], image(n).shape[2], 4) for n in names]
    pairs = []
    for n, (t0, l0, rh, rw) in zip(names, boxes):
        hr_c = image(n)[:, t0:t0 + rh, l0:l0 + rw].contiguous()
        pairs.append((torch.zeros(3, rh // 4, rw // 4, device="cuda:0"), hr_c))
    random.seed(4)
    _, want = sm.sample_pairs(pairs)
    random.seed(4)
    draws = [sm.draw_for(p[0]) for p in pairs]
    got = sm.gather_hr_strided([image(n) for n in names], boxes, draws)
    assert got.shape == (5, 3, 32, 32) and torch.equal(got, want)
    assert boxes[0][:2] == (1, 2)


def _set5_dataset(monkeypatch, meta_file=None, **params):
    real = D.pca_matrix
    monkeypatch.setattr(D, "pca_matrix", lambda batch=2000, k=10: real(batch=2000, k=k))
    np.random.seed(5)
    return data.SuperResImages(hr_dir=os.path.join(GOLDEN, "set5", "hr"), online_degradations=True, split="all", scale=4,
                               random_crop=24, random_augments=True, degradation_metadata_file=meta_file,
                               online_degradation_params=params or None)


def _seed():
    torch.manual_seed(3)
    np.random.seed(6)
    random.seed(7)


def _streams():
    return np.random.random(), random.random(), float(torch.rand(1))


def _same_batches(a, b, lr_too=True):
    assert list(a["tag"]) == list(b["tag"]) and list(a["hr_tag"]) == list(b["hr_tag"])
    assert torch.equal(a["hr"], b["hr"]) and (not lr_too or torch.equal(a["lr"], b["lr"]))
    assert torch.equal(a["metadata"], b["metadata"]) and a["metadata"].dtype == b["metadata"].dtype
    assert torch.equal(a["blur_kernels"], b["blur_kernels"]) and a["metadata_keys"] == b["metadata_keys"]
    assert torch.equal(a["mask"], b["mask"]) and torch.equal(a["halfway_data"], b["halfway_data"])
    assert set(a) == set(b)


@pytest.mark.parametrize("with_meta", [False, True])
def test_loader_in_tile_mode_equals_the_whole_image_mode(monkeypatch, tmp_path, with_meta):
    """The seeds of test_degrade_gpu.py::test_device_tile_loader_with_online_degradations_equals_the_dataloader_path."""
    meta_file = None
    if with_meta:
        import pandas as pd
        names = sorted(os.listdir(os.path.join(GOLDEN, "set5", "hr")))
        meta_file = str(tmp_path / "meta.csv")
        pd.DataFrame({"QPI": [20 + 4 * i for i in range(len(names))]}, index=names).to_csv(meta_file)
    dev = torch.device("cuda:0")
    whole = data.DeviceTileLoader([_set5_dataset(monkeypatch, meta_file)], 2, dev)
    tiles = data.DeviceTileLoader([_set5_dataset(monkeypatch, meta_file)], 2, dev, degrade_tiles=True)
    _seed()
    want = list(whole)
    want_streams = _streams()
    _seed()
    got = list(tiles)
    assert _streams() == want_streams
    assert len(got) == len(want) == 3
    for a, b in zip(want, got):
        _same_batches(a, b)
        assert b["lr"].shape[1:] == (3, 24, 24) and b["hr"].shape[1:] == (3, 96, 96) and b["lr"].dtype == torch.float32


def test_loader_in_tile_mode_with_jpeg(monkeypatch):
    """Same draws, metadata and kernels as the whole-image mode; `lr` is the round trip of the TILE (block grid at the tile's
    origin), computed here from the whole-image path without its JPEG stage + jpeg_roundtrip of the tile + the gather."""
    dev = torch.device("cuda:0")
    params = {"jpeg": True, "jpeg_quality": [30, 95]}
    whole = data.DeviceTileLoader([_set5_dataset(monkeypatch, **params)], 2, dev)
    tiles = data.DeviceTileLoader([_set5_dataset(monkeypatch, **params)], 2, dev, degrade_tiles=True)
    _seed()
    want = list(whole)
    want_streams = _streams()
    _seed()
    got = list(tiles)
    assert _streams() == want_streams
    # replay the draws by hand for the expectation
    _seed()
    torch.empty((), dtype=torch.int64).random_()
    g = torch.Generator()
    g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
    order = torch.randperm(5, generator=g).tolist()
    n = 0
    for a, b in zip(want, got):
        _same_batches(a, b, lr_too=False)
        idx = order[n:n + 2]
        n += 2
        ds = [tiles.degraders[i].draw() for i in idx]
        for k, (i, d) in enumerate(zip(idx, ds)):
            hr = tiles.sampler.hr[i]
            t0, l0, rh, rw = D.center_crop_box(hr.shape[1], hr.shape[2], 4)
            h, w = rh // 4, rw // 4
            top, left, hf, vf, rot = tiles.sampler.draw_for(torch.empty(0, h, w))
            ty, tx = data.tile_source_box(h, w, 24, top, left, hf, vf, rot)
            lr = whole_image_lr(hr, d.kernel, 4, to_float=False)
            tile = D.jpeg_roundtrip(lr[:, ty:ty + 24, tx:tx + 24].contiguous(), d.quality, to_float=False).cpu()
            exp = gather_on_host(tile, (24, 24) + draw_for_origin(24, 24, 24, 0, 0, hf, vf, rot) + (hf, vf, rot), 24)
            assert torch.equal(b["lr"][k].cpu(), exp.float().div(255)), (i, d.quality)
            assert torch.equal(d.kernel, a["blur_kernels"][k])


def test_loader_in_tile_mode_with_noise_keeps_codes_and_sets_a_seeded_field(monkeypatch):
    """With `noise` the tile mode draws one seed where the whole-image mode draws its host field: the same kernel, level and
    code, and an LR tile equal to the whole-image chain fed normal_field(seed)."""
    dev = torch.device("cuda:0")
    params = {"noise": True, "noise_high": 0.08, "rate_cln": 0.2}
    tiles = data.DeviceTileLoader([_set5_dataset(monkeypatch, **params)], 2, dev, degrade_tiles=True)
    _seed()
    b = next(iter(tiles))
    _seed()
    torch.empty((), dtype=torch.int64).random_()
    g = torch.Generator()
    g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
    idx = torch.randperm(5, generator=g).tolist()[:2]
    ds = [tiles.degraders[i].draw() for i in idx]
    assert tuple(b["metadata"].shape) == (2, 11)
    for k, (i, d) in enumerate(zip(idx, ds)):
        hr = tiles.sampler.hr[i]
        _, _, rh, rw = D.center_crop_box(hr.shape[1], hr.shape[2], 4)
        h, w = rh // 4, rw // 4
        draw = tiles.sampler.draw_for(torch.empty(0, h, w))
        lr = whole_image_lr(hr, d.kernel, 4, d.level, d.seed).cpu()
        assert torch.equal(b["lr"][k].cpu(), gather_on_host(lr, (h, w) + draw, 24))
        assert torch.equal(b["metadata"][k], d.code) and abs(float(d.code[10]) - 10 * d.level) < 1e-6


def test_training_step_from_a_tile_mode_batch(monkeypatch):
    """QEDSR fed a degrade_tiles batch reports the loss of the step fed the whole-image loader's batch."""
    dev = torch.device("cuda:0")
    losses = []
    for mode in (False, True):
        loader = data.DeviceTileLoader([_set5_dataset(monkeypatch)], 4, dev, degrade_tiles=mode)
        _seed()
        batch = next(iter(loader))
        torch.manual_seed(8)
        h = sisr_amd.available_models["qedsr"](device=0, model_save_dir="/tmp", eval_mode=False, scale=4, num_blocks=2,
                                               metadata=["blur_kernel"])
        loss, _ = h.train_step(batch["lr"], batch["hr"], metadata=batch["metadata"], metadata_keys=batch["metadata_keys"])
        losses.append(float(loss))
    assert losses[0] == losses[1], losses
