"""The JPEG degradation stage without a GPU: the numpy statement of libjpeg's arithmetic (degrade.jpeg_roundtrip_host) against
Pillow byte for byte, the quantisation tables, the C ABI's refusals, the degrader's random draws, keys and code length, and
tools/make_jpeg_set.py (ref: sr_tools/data_converter.py:178-194 jpeg_compress)."""
import ctypes
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

import sisr_amd
from conftest import GOLDEN, ROOT
import _jpeg as J

D = sisr_amd.degrade


@pytest.mark.parametrize("C", [3, 1])
def test_host_form_is_byte_identical_to_pillow(C):
    """... and its int32 run equals its int64 run on every input: 32 bits are enough for the kernel."""
    for label, img, q in J.cases(C):
        got = D.jpeg_roundtrip_host(img, q)
        want = J.pil_roundtrip(img, q)
        assert got.dtype == np.uint8 and got.shape == want.shape == img.shape
        assert np.array_equal(got, want), (label, C, q, int((got != want).sum()))
        assert np.array_equal(D.jpeg_roundtrip_host(img, q, acc=np.int32), got), (label, C, q)


@pytest.mark.parametrize("q", [1, 2, 10, 49, 50, 51, 75, 95, 100])
def test_tables_equal_the_ones_pillow_reports(q):
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(J.random_image(3, (16, 16)).transpose(1, 2, 0).copy()).save(buf, "JPEG", subsampling=0, quality=q)
    buf.seek(0)
    reported = PIL.Image.open(buf).quantization  # {table id: 64 entries}; Pillow >= 8.3 has undone the file's zig-zag order
    luma, chroma = D.jpeg_tables(q)
    assert luma.shape == chroma.shape == (8, 8)
    assert list(reported[0]) == luma.ravel().tolist() and list(reported[1]) == chroma.ravel().tolist()


def test_host_form_and_tables_refuse_bad_arguments():
    img = np.zeros((3, 8, 8), np.uint8)
    for q in (0, 101, 50.5, True):
        with pytest.raises(ValueError):
            D.jpeg_tables(q)
        with pytest.raises(ValueError):
            D.jpeg_roundtrip_host(img, q)
    for bad in (np.zeros((2, 8, 8), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((3, 8, 8), np.float32), np.zeros((3, 0, 8), np.uint8)):
        with pytest.raises(ValueError):
            D.jpeg_roundtrip_host(bad, 50)


def test_abi_refusals_need_no_gpu():
    L = sisr_amd.hip.lib()
    buf = (ctypes.c_ubyte * 256)()
    a = ctypes.addressof(buf)  # a non-null stand-in: every call below must return before it is dereferenced
    ERR_ARG = -1
    f = L.sisr_jpeg_roundtrip
    assert f(None, a, 3, 8, 8, 50, 0, None) == ERR_ARG and f(a, None, 3, 8, 8, 50, 0, None) == ERR_ARG
    for C in (0, 2, 4, -1):
        assert f(a, a, C, 8, 8, 50, 0, None) == ERR_ARG
    assert f(a, a, 3, 0, 8, 50, 0, None) == ERR_ARG and f(a, a, 3, 8, 0, 50, 0, None) == ERR_ARG
    assert f(a, a, 3, -8, 8, 50, 0, None) == ERR_ARG
    for q in (0, 101, -5):
        assert f(a, a, 3, 8, 8, q, 0, None) == ERR_ARG
    for tf in (2, -1):
        assert f(a, a, 3, 8, 8, 50, tf, None) == ERR_ARG


def test_device_call_has_no_cpu_path():
    with pytest.raises(RuntimeError, match="HIP device"):
        D.jpeg_roundtrip(torch.zeros(3, 8, 8, dtype=torch.uint8), 50)


# ----------------------------------------------------------------------------- the degrader's host side
class _NoKernels:
    """Stands in for the device: the launches return success and touch nothing, so that OnlineDegrader's host side -- the
    random draws, the code, the keys -- runs on CPU tensors."""

    def __init__(self, monkeypatch):
        self.qualities = []
        hip = sisr_amd.hip

        class Lib:
            def __getattr__(self, name):
                return lambda *a: 0
        monkeypatch.setattr(hip, "lib", lambda: Lib())
        monkeypatch.setattr(hip, "ptr", lambda t: 0)
        monkeypatch.setattr(hip, "stream", lambda: None)

        def blur_quant(hr, kernel, want_float=False, want_u8=True):
            u8 = torch.zeros(hr.shape, dtype=torch.uint8)
            return (u8 if want_u8 else None, torch.zeros(hr.shape)) if want_float else u8

        def jpeg_roundtrip(u8, quality, to_float=True):
            self.qualities.append(quality)
            return torch.zeros(u8.shape, dtype=torch.float32 if to_float else torch.uint8)
        monkeypatch.setattr(D, "blur_quant", blur_quant)
        monkeypatch.setattr(D, "pil_bicubic_downsample", lambda u8, scale, to_float=True: torch.zeros(
            (u8.shape[0], u8.shape[1] // scale, u8.shape[2] // scale), dtype=torch.float32 if to_float else torch.uint8))
        monkeypatch.setattr(D, "jpeg_roundtrip", jpeg_roundtrip)


def _draws_before_this_stage(noise, hw):
    """The np.random calls one OnlineDegrader access made before the JPEG stage existed (random isotropic kernels; ref:
    gaussian_utils.py:278-282, :299-312), written out."""
    np.random.random()  # isotropic or not
    np.random.random()  # sigma
    if noise:
        np.random.uniform(size=(1, 1))  # level
        np.random.uniform(size=(1, 1))  # clean mask
        np.random.normal(loc=0.0, scale=1.0, size=(1, 3) + hw)  # the field


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("noise", [False, True])
def test_degrader_without_jpeg_consumes_the_numpy_stream_as_before(monkeypatch, noise):
    _NoKernels(monkeypatch)
    pca = torch.zeros(441, 10)
    hw = (24, 32)
    deg = D.OnlineDegrader(scale=4, pca=pca, noise=noise)
    np.random.seed(11)
    for _ in range(3):
        lr, code, kernel, box = deg(torch.zeros((3,) + hw))
        assert code.shape == (11 if noise else 10,) and lr.dtype == torch.float32
    got = np.random.get_state()
    np.random.seed(11)
    for _ in range(3):
        _draws_before_this_stage(noise, hw)
    assert _same_state(got, np.random.get_state())
    assert deg.metadata_keys() == ["blur_kernel"] * 10


@pytest.mark.parametrize("noise", [False, True])
def test_degrader_with_jpeg_draws_the_quality_last_and_appends_it(monkeypatch, noise):
    stub = _NoKernels(monkeypatch)
    hw = (24, 32)
    deg = D.OnlineDegrader(scale=4, pca=torch.zeros(441, 10), noise=noise, jpeg=True, jpeg_quality=[30, 90])
    np.random.seed(12)
    codes = [deg(torch.zeros((3,) + hw))[1] for _ in range(4)]
    got = np.random.get_state()
    np.random.seed(12)
    want_q = []
    for _ in range(4):
        _draws_before_this_stage(noise, hw)
        want_q.append(int(np.random.randint(30, 91)))
    assert _same_state(got, np.random.get_state()) and stub.qualities == want_q and len(set(want_q)) > 1
    n = 12 if noise else 11
    for code, q in zip(codes, want_q):
        assert code.shape == (n,) and code.dtype == torch.float32
        assert code[-1].item() == np.float32((q - 30) / 60)
    assert deg.metadata_keys() == ["blur_kernel"] * 10 + (["noise"] if noise else []) + ["jpeg_quality"]
    assert len(deg.metadata_keys()) == n


def test_degrader_jpeg_options():
    pca = torch.zeros(441, 10)
    d = D.OnlineDegrader(pca=pca, jpeg=True)
    assert (d.jpeg_lo, d.jpeg_hi, d.jpeg_norm) == (30, 95, (30.0, 95.0))
    d = D.OnlineDegrader(pca=pca, jpeg=True, jpeg_quality=60)
    assert (d.jpeg_lo, d.jpeg_hi, d.jpeg_norm) == (60, 60, (0.0, 100.0))
    d = D.OnlineDegrader(pca=pca, jpeg=True, jpeg_quality=[10, 60], jpeg_norm=[0, 100])
    assert d.jpeg_norm == (0.0, 100.0)
    for kw in (dict(jpeg_quality=[60, 10]), dict(jpeg_quality=[0, 50]), dict(jpeg_quality=[50, 101]), dict(jpeg_norm=[50, 50])):
        with pytest.raises(ValueError):
            D.OnlineDegrader(pca=pca, jpeg=True, **kw)
    assert not D.OnlineDegrader(pca=pca).jpeg and not D.OnlineDegrader(pca=pca, jpeg_quality=[60, 10]).jpeg  # off: options unread


@pytest.mark.parametrize("noise", [False, True])
def test_dataset_keys_with_jpeg_in_both_forms(monkeypatch, tmp_path, noise):
    """One key per value, flat and -- next to file metadata -- as the nested list the reference appends; a Q-model that selects
    ['blur_kernel', 'jpeg_quality'] counts 11 values."""
    import pandas as pd
    monkeypatch.setattr(D, "pca_matrix", lambda batch=30000, k=10: torch.zeros(441, k))
    hr_dir = os.path.join(GOLDEN, "set5", "hr")
    params = dict(jpeg=True, jpeg_quality=[30, 90], noise=noise)
    keys = ["blur_kernel"] * 10 + (["noise"] if noise else []) + ["jpeg_quality"]
    ds = sisr_amd.data.SuperResImages(hr_dir=hr_dir, online_degradations=True, online_degradation_params=params, split="all", scale=4)
    assert ds.metadata_keys == keys
    names = sorted(os.listdir(hr_dir))
    meta_file = tmp_path / "meta.csv"
    pd.DataFrame({"QPI": [20 + 4 * i for i in range(len(names))]}, index=names).to_csv(meta_file)
    ds = sisr_amd.data.SuperResImages(hr_dir=hr_dir, online_degradations=True, online_degradation_params=params, split="all", scale=4,
                                      degradation_metadata_file=str(meta_file))
    assert ds.metadata_keys == ["qpi", keys]
    ds = sisr_amd.data.SuperResImages(hr_dir=hr_dir, online_degradations=True, online_degradation_params=dict(noise=noise),
                                      split="all", scale=4)
    assert ds.metadata_keys == ["blur_kernel"] * 10  # jpeg off: the reference's list
    model = sisr_amd.handlers.QModel.__new__(sisr_amd.handlers.QModel)
    model.metadata, model.num_metadata, model.style = ["blur_kernel", "jpeg_quality"], 11, "standard"
    md = torch.arange(2 * len(keys), dtype=torch.float64).reshape(2, len(keys))
    got = model.generate_channels(torch.zeros(2, 3, 4, 4), md, [(k, k) for k in keys])
    pick = [i for i, k in enumerate(keys) if k != "noise"]
    assert got.shape == (2, 11, 1, 1) and torch.equal(got[:, :, 0, 0], md[:, pick].float())


# ----------------------------------------------------------------------------- the fixed evaluation set
def _tool():
    spec = importlib.util.spec_from_file_location("make_jpeg_set", os.path.join(ROOT, "tools", "make_jpeg_set.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_make_jpeg_set_writes_pillows_round_trips_and_a_readable_metadata_file(tmp_path):
    import PIL.Image
    lr_dir = os.path.join(GOLDEN, "set5", "lr_random_blur")
    out = tmp_path / "set5_jpeg"
    rows = _tool().make_jpeg_set(lr_dir, str(out), [10, 60], host=True)
    names = sorted(n for n in os.listdir(lr_dir) if n.endswith(".png"))
    assert [r[0] for r in rows] == [f"{n[:-4]}_q{i}.png" for n in names for i in range(2)]
    assert sorted(os.listdir(out)) == sorted([r[0] for r in rows] + ["degradation_metadata.csv"])
    for n in names:
        src = np.asarray(PIL.Image.open(os.path.join(lr_dir, n)).convert("RGB")).transpose(2, 0, 1)
        for i, q in enumerate((10, 60)):
            got = np.asarray(PIL.Image.open(out / f"{n[:-4]}_q{i}.png")).transpose(2, 0, 1)
            assert np.array_equal(got, J.pil_roundtrip(src, q)), (n, q)
    with open(out / "degradation_metadata.csv") as f:
        lines = f.read().split()
    assert lines[0] == "image,jpeg_quality" and lines[1] == f"{names[0][:-4]}_q0.png,10" and len(lines) == 1 + 2 * len(names)
    ds = sisr_amd.data.SuperResImages(lr_dir=str(out), hr_dir=os.path.join(GOLDEN, "set5", "hr"), split="all", scale=4,
                                      degradation_metadata_file=str(out / "degradation_metadata.csv"))
    assert ds.metadata_keys == ["jpeg_quality"] and len(ds) == 2 * len(names)
    for i in range(len(ds)):
        it = ds[i]
        want = 0.0 if it["tag"].endswith("_q0.png") else 1.0
        assert it["metadata"].tolist() == [want] and it["hr_tag"] == it["tag"][:-7] + ".png"
        assert it["hr"].shape[1] == 4 * it["lr"].shape[1]
    # a single quality keeps the plain names
    rows = _tool().make_jpeg_set(lr_dir, str(tmp_path / "single"), [75], host=True)
    assert [r[0] for r in rows] == names and {r[1] for r in rows} == {75}
