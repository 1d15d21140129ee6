"""The device output stage (csrc/eval_output.hip, sisr_eval_output): its float64 MSE against an exactly rounded sum of the
host's Y planes, Y-PSNR against the host metrics.psnr, its bytes against the host cast, and the device_outputs /
device_metrics switches of eval_sisr / train_sisr against the default host path.  numpy only on the reference side."""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

import _basic as R
import sisr_amd
from _ssim_common import set5_rgb_pairs
from conftest import GOLDEN, golden_json

pytestmark = pytest.mark.gpu
M = sisr_amd.metrics
hip = sisr_amd.hip

# (n, h, w): one pixel; h * w odd, planes unaligned (element-by-element form); odd sides; the 16-byte form; two images whose
# planes are unaligned; a tail group (61 * 130 = 7930, not a multiple of 4: the last group holds two pixels); several blocks of
# 2048 pixels with h * w odd; the partial-sum order at full size (1351 blocks)
SHAPES = [(1, 1, 1), (2, 3, 5), (1, 7, 9), (3, 16, 16), (2, 33, 47), (1, 61, 130), (1, 255, 257), (1, 1356, 2040)]
SIGMAS = (1e-4, 1e-2, 0.2)
SHAVES = (0, 1, 4)
ids = lambda s: "x".join(map(str, s))  # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(shape, sigma):
    """(sr, hr, Y of sr, Y of hr): HR uniform in [0, 1], the output HR + sigma * noise (it overshoots [0, 1]); the Y planes as
    the host forms them (metrics.batch_rgb_to_ycbcr).  Made once per (shape, sigma) and left unchanged."""
    n, h, w = shape
    g = np.random.default_rng(1000 * h + w + int(sigma * 1e4))
    hr = g.random((n, 3, h, w), dtype=np.float32)
    sr = hr + np.float32(sigma) * g.standard_normal((n, 3, h, w)).astype(np.float32)
    ys, yh = M.batch_rgb_to_ycbcr(sr)[:, 0], M.batch_rgb_to_ycbcr(hr)[:, 0]
    for t in (sr, hr, ys, yh):
        t.setflags(write=False)
    return sr, hr, ys, yh


def _exact_mse(ys, yh, shave):
    """math.fsum over the float64 squares of the fp32 differences, divided by the count: the correctly rounded sum"""
    h, w = ys.shape
    d = (ys[shave:h - shave, shave:w - shave] - yh[shave:h - shave, shave:w - shave]).astype(np.float64)
    return math.fsum((d * d).ravel().tolist()) / d.size


def _device(sr, hr=None, chroma=None, hr_form=0, shave=0, want_mse=True, want_rgb8=False):
    """one raw sisr_eval_output call on numpy batches -> (n float64 mse or None, (n, h, w, 3) uint8 or None)"""
    n, c, h, w = sr.shape
    up = lambda t: None if t is None else torch.from_numpy(np.ascontiguousarray(t)).cuda()  # noqa: E731
    a, b, ch = up(sr), up(hr), up(chroma)
    L = hip.lib()
    nbytes = L.sisr_eval_output_workspace_bytes(n, h, w)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mse = torch.full((n,), -1.0, dtype=torch.float64, device="cuda") if want_mse else None
    rgb8 = torch.full((n, h, w, 3), 77, dtype=torch.uint8, device="cuda") if want_rgb8 else None
    hip.check(L.sisr_eval_output(a.data_ptr(), c, None if ch is None else ch.data_ptr(), None if b is None else b.data_ptr(),
                                 hr_form, 1 if b is None else b.shape[1], n, h, w, shave,
                                 None if mse is None else mse.data_ptr(), None if rgb8 is None else rgb8.data_ptr(),
                                 ws.data_ptr(), nbytes, hip.stream()), "sisr_eval_output")
    torch.cuda.synchronize()
    return (None if mse is None else mse.cpu().numpy()), (None if rgb8 is None else rgb8.cpu().numpy())


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_mse_is_the_exact_sum_of_the_hosts_y_planes(shape):
    """rtol 1e-12: the terms are positive, so every partial sum has relative error <= (chain length) * 2^-53, and the longest
    chain of sequential additions is 31 at the largest shape (csrc/eval_output.hip) -- about 3.4e-15; the bound allows
    chains of about 4,000"""
    n, h, w = shape
    for sigma in SIGMAS:
        sr, hr, ys, yh = _case(shape, sigma)
        for shave in SHAVES:
            if 2 * shave >= min(h, w):
                continue
            got, _ = _device(sr, hr, shave=shave)
            want = [_exact_mse(ys[i], yh[i], shave) for i in range(n)]
            print(shape, sigma, shave, got, want)
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=str((sigma, shave)))
            if shave == 0:  # with the bytes made by the same launch the sums are the same bits
                both, _ = _device(sr, hr, want_rgb8=True)
                assert both.tobytes() == got.tobytes()
    sr, hr, _, _ = _case(shape, SIGMAS[-1])
    first, _ = _device(sr, hr, shave=0)
    again, _ = _device(sr, hr, shave=0)
    assert first.tobytes() == again.tobytes()  # a repeat launch is bit-identical
    zero, _ = _device(hr, hr)
    assert (zero == 0).all()
    assert M.batch_psnr(torch.from_numpy(hr).cuda(), torch.from_numpy(hr)) == [100] * n  # mse == 0 gives exactly 100


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_batch_psnr_on_the_device_against_the_host_psnr(shape):
    """1e-4 dB: the host takes an fp32 pairwise mean of fp32 squares over at most 2.8 M terms -- relative error of a few
    2^-24 in the mse, 10 / ln 10 * that in dB, about 1e-6 dB worst case short of systematic rounding; the largest gap measured
    between metrics.psnr and the float64 form over these shapes was 1.6e-5 dB"""
    n, h, w = shape
    for sigma in SIGMAS:
        sr, hr, ys, yh = _case(shape, sigma)
        for shave in SHAVES:
            if 2 * shave >= min(h, w):
                continue
            got = M.batch_psnr(torch.from_numpy(sr).cuda(), torch.from_numpy(hr), shave=shave)  # the host batch follows
            want = [M.psnr(ys[i, shave:h - shave, shave:w - shave], yh[i, shave:h - shave, shave:w - shave], 1)
                    for i in range(n)]
            print(shape, sigma, shave, got, want)
            assert len(got) == n and all(isinstance(v, (int, float)) for v in got)
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-4, err_msg=str((sigma, shave)))
            if shave == 0:
                assert M.batch_psnr(sr, hr) == want  # the host form is the host expression itself


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_bytes_of_an_rgb_output_equal_the_host_cast(shape):
    for sigma in SIGMAS:
        sr, hr, _, _ = _case(shape, sigma)
        want = (np.clip(sr, 0, 1) * 255).round().astype(np.uint8).transpose(0, 2, 3, 1)
        _, got = _device(sr, want_mse=False, want_rgb8=True)
        np.testing.assert_array_equal(got, want)
        _, both = _device(sr, hr, want_rgb8=True)
        np.testing.assert_array_equal(both, want)
    sr, _, _, _ = _case(shape, 0.2)
    assert (sr < 0).any() and (sr > 1).any() or shape == (1, 1, 1)
    dev = M.batch_rgb8(torch.from_numpy(sr).cuda())
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == (shape[0], shape[1], shape[2], 3)
    np.testing.assert_array_equal(dev.cpu().numpy(), M.batch_rgb8(sr))


def test_bytes_round_half_to_even():
    """float32((k + 0.5) / 255) * 255 is k + 0.5 exactly in fp32 for every k in 0 .. 255: all 256 are ties"""
    ties = ((np.arange(256, dtype=np.float64) + 0.5) / 255).astype(np.float32)
    assert ((ties * np.float32(255)) == np.arange(256, dtype=np.float32) + np.float32(0.5)).all()
    k = np.arange(256)
    even = np.minimum(np.where(k % 2 == 0, k, k + 1), 255).astype(np.uint8)
    for shape in ((2, 3, 16, 16), (1, 3, 1, 256), (1, 3, 3, 255)):  # the 16-byte form, and two element-by-element ones
        n, _, h, w = shape
        count = h * w
        batch = np.stack([np.stack([np.roll(np.resize(ties, count), c + 5 * i) for c in range(3)]) for i in range(n)])
        batch = batch.reshape(n, 3, h, w)
        want = (np.clip(batch, 0, 1) * 255).round().astype(np.uint8).transpose(0, 2, 3, 1)
        if count >= 256:
            np.testing.assert_array_equal(want[0, :, :, 0].reshape(-1)[:256], even)
        _, got = _device(batch, want_mse=False, want_rgb8=True)
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_one_plane_form(shape):
    """Y, Cb, Cr in [-0.1, 1.1]: bytes equal the host's batch_ycbcr_to_rgb + cast wherever the host's rounded value lies in
    0 .. 255 and saturate elsewhere; the mse with hr_form = 1 is that of the clipped planes"""
    n, h, w = shape
    g = np.random.default_rng(7 + h * w)
    ycc = g.random((n, 3, h, w), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    ref = g.random((n, 3, h, w), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)  # a YCbCr reference: plane 0 counts
    chroma = ycc.copy()
    chroma[:, 0] = np.nan  # plane 0 of chroma is never read
    v = (M.batch_ycbcr_to_rgb(ycc) * 255).round().transpose(0, 2, 3, 1)
    inside = (v >= 0) & (v <= 255)
    if h * w >= 63:
        assert inside.any() and (v < 0).any() and (v > 255).any()  # both kinds of pixel
    want = np.clip(v, 0, 255).astype(np.uint8)
    host_cast = v.astype(np.int64).astype(np.uint8)
    assert (want[inside] == host_cast[inside]).all()
    mse, got = _device(ycc[:, :1], ref, chroma=chroma, hr_form=1, want_rgb8=True)
    np.testing.assert_array_equal(got[inside], host_cast[inside])
    assert (got[v < 0] == 0).all() and (got[v > 255] == 255).all()
    np.testing.assert_array_equal(got, M.batch_rgb8(ycc[:, :1], chroma=ycc))  # the host form saturates the same way
    ys, yh = np.clip(ycc[:, 0], 0, 1), np.clip(ref[:, 0], 0, 1)
    np.testing.assert_allclose(mse, [_exact_mse(ys[i], yh[i], 0) for i in range(n)], rtol=1e-12, atol=0)
    if min(h, w) > 2:
        mse1, _ = _device(ycc[:, :1], ref[:, :1], hr_form=1, shave=1)  # an HR batch of one plane
        np.testing.assert_allclose(mse1, [_exact_mse(ys[i], yh[i], 1) for i in range(n)], rtol=1e-12, atol=0)


@pytest.mark.parametrize("shape", [(2, 33, 47), (3, 16, 16)], ids=ids)
def test_one_plane_mse_equals_the_three_plane_reference_built_from_plane_0(shape):
    n = shape[0]
    sr, hr, ys, yh = _case(shape, 0.2)
    want = [_exact_mse(ys[i], yh[i], 0) for i in range(n)]
    ycc_hr = M.batch_rgb_to_ycbcr(hr)
    got, _ = _device(np.ascontiguousarray(ys[:, None]), ycc_hr, hr_form=1)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    rgb_ref, _ = _device(np.ascontiguousarray(ys[:, None]), hr, hr_form=0)  # a Y output against an RGB reference
    np.testing.assert_allclose(rgb_ref, want, rtol=1e-12, atol=0)
    three, _ = _device(sr, hr)
    assert three.tobytes() == got.tobytes() == rgb_ref.tobytes()


def test_set5_psnr_on_the_device_against_y_psnr():
    for name, hr, lr in set5_rgb_pairs():
        got = M.batch_psnr(torch.from_numpy(lr[None]).cuda(), torch.from_numpy(hr[None]).cuda())[0]
        assert abs(got - M.y_psnr(lr, hr)) <= 1e-4, name


def test_capture_and_unaligned_views():
    """a batch that starts 4 bytes into an allocation takes the element-by-element form and gives the same results; the call
    neither allocates nor synchronises, so it can be captured and replayed"""
    sr, hr, _, _ = _case((3, 16, 16), 0.2)
    want_mse, want_rgb8 = _device(sr, hr, want_rgb8=True)
    n, c, h, w = sr.shape
    L = hip.lib()
    nbytes = L.sisr_eval_output_workspace_bytes(n, h, w)
    pad = torch.zeros(sr.size + 1, dtype=torch.float32, device="cuda")
    a = pad[1:].view(n, c, h, w)
    a.copy_(torch.from_numpy(sr))
    b = torch.from_numpy(hr).cuda()
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mse = torch.zeros(n, dtype=torch.float64, device="cuda")
    raw = torch.zeros(n * h * w * 3 + 1, dtype=torch.uint8, device="cuda")
    assert a.data_ptr() % 16 == 4
    for rgb8 in (raw[:-1], raw[1:]):  # an aligned and an odd byte run
        hip.check(L.sisr_eval_output(a.data_ptr(), 3, None, b.data_ptr(), 0, 3, n, h, w, 0, mse.data_ptr(), rgb8.data_ptr(),
                                     ws.data_ptr(), nbytes, hip.stream()), "sisr_eval_output")
        torch.cuda.synchronize()
        assert mse.cpu().numpy().tobytes() == want_mse.tobytes()
        np.testing.assert_array_equal(rgb8.cpu().numpy().reshape(n, h, w, 3), want_rgb8)
    a2 = torch.from_numpy(sr).cuda()
    out8 = torch.zeros((n, h, w, 3), dtype=torch.uint8, device="cuda")
    mse.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.check(L.sisr_eval_output(a2.data_ptr(), 3, None, b.data_ptr(), 0, 3, n, h, w, 0, mse.data_ptr(),
                                     out8.data_ptr(), ws.data_ptr(), nbytes, hip.stream()), "sisr_eval_output")
    graph.replay()
    torch.cuda.synchronize()
    assert mse.cpu().numpy().tobytes() == want_mse.tobytes()
    np.testing.assert_array_equal(out8.cpu().numpy(), want_rgb8)


# ----------------------------------------------------------------------------- entry points
def _edsr_config(tmp_path):
    cfg = copy.deepcopy(golden_json("g5_train_sisr")["edsr"]["config"])
    cfg["experiment_save_loc"] = str(tmp_path)
    for part in ("training_sets", "eval_sets"):
        for d in cfg["data"][part].values():
            d["lr"] = d["lr"].replace("SET5", os.path.join(GOLDEN, "set5"))
            d["hr"] = d["hr"].replace("SET5", os.path.join(GOLDEN, "set5"))
    cfg["training"].update(gpu="single", sp_gpu=0, metrics=["PSNR", "SSIM"], num_epochs=1)
    return cfg


def _eval(tmp_path, experiment, results_name, **kw):
    d = os.path.join(GOLDEN, "set5")
    return sisr_amd.cli.eval_sisr(model_and_epoch=[[experiment, "0"]], model_loc=str(tmp_path), gpu=True,
                                  hr_dir=os.path.join(d, "hr"), lr_dir=os.path.join(d, "lr_random_blur"),
                                  full_directory=True, scale=4, out_loc=str(tmp_path), results_name=results_name,
                                  metrics=["PSNR", "SSIM"], **kw)


def test_train_and_eval_switches_against_the_default_path(tmp_path, monkeypatch):
    from PIL import Image
    cfg = _edsr_config(tmp_path)
    plain = sisr_amd.cli.train_sisr(copy.deepcopy(cfg))
    sw = copy.deepcopy(cfg)
    sw["experiment"] = cfg["experiment"] + "_dm"
    sw["training"]["device_metrics"] = True
    host_calls = []
    real = sisr_amd.handlers.ModelInterface.net_run_and_process
    monkeypatch.setattr(sisr_amd.handlers.ModelInterface, "net_run_and_process",
                        lambda self, *a, **k: host_calls.append(1) or real(self, *a, **k))
    switched = sisr_amd.cli.train_sisr(sw)  # the same seed: the same weights, so the same validation outputs
    assert not host_calls
    print(plain["val-PSNR"], switched["val-PSNR"], plain["val-SSIM"], switched["val-SSIM"])
    assert list(switched["val-loss"]) == list(plain["val-loss"])
    np.testing.assert_allclose(switched["val-PSNR"], plain["val-PSNR"], rtol=0, atol=1e-4)
    assert list(switched["val-SSIM"]) == list(plain["val-SSIM"])

    df0, avg0 = _eval(tmp_path, cfg["experiment"], "ev_plain", save_im=True)
    df1, avg1 = _eval(tmp_path, cfg["experiment"], "ev_dev", save_im=True, device_outputs=True)
    assert not host_calls
    assert list(df1.columns) == list(df0.columns) == ["Image_Name", "Model", "PSNR", "SSIM", "runtime"]
    assert list(df1["Image_Name"]) == list(df0["Image_Name"]) and len(df1) == 5
    print(list(df0["PSNR"]), list(df1["PSNR"]))
    np.testing.assert_allclose(df1["PSNR"], df0["PSNR"], rtol=0, atol=1e-4)
    np.testing.assert_array_equal(df1["SSIM"], df0["SSIM"])
    for tag in df0["Image_Name"]:
        a, b = (np.asarray(Image.open(os.path.join(str(tmp_path), r, cfg["experiment"], os.path.basename(tag))))
                for r in ("ev_plain", "ev_dev"))
        assert a.dtype == np.uint8 and a.ndim == 3
        np.testing.assert_array_equal(a, b)
    df2, _ = _eval(tmp_path, cfg["experiment"], "ev_shave", device_outputs=True, psnr_shave=4)
    assert (np.asarray(df2["PSNR"]) != np.asarray(df1["PSNR"])).all()
    with pytest.raises(ValueError, match="psnr_shave"):
        _eval(tmp_path, cfg["experiment"], "ev_bad", psnr_shave=4)


def test_a_y_channel_checkpoint_through_eval_sisr_with_the_switch_on(tmp_path):
    """srcnn: one output plane, chroma from the interpolated input, the HR batch in YCbCr (hr_form 1)"""
    from PIL import Image
    cfg = R.b4_config(tmp_path)
    cfg["training"].update(gpu="single", sp_gpu=0, metrics=["PSNR", "SSIM"], num_epochs=1)
    sisr_amd.cli.train_sisr(cfg)
    df0, _ = _eval(tmp_path, cfg["experiment"], "ev_plain", save_im=True)
    df1, _ = _eval(tmp_path, cfg["experiment"], "ev_dev", save_im=True, device_outputs=True)
    assert len(df1) == 5 and list(df1["Image_Name"]) == list(df0["Image_Name"])
    print(list(df0["PSNR"]), list(df1["PSNR"]))
    np.testing.assert_allclose(df1["PSNR"], df0["PSNR"], rtol=0, atol=1e-4)
    np.testing.assert_array_equal(df1["SSIM"], df0["SSIM"])
    for tag in df0["Image_Name"]:
        # the bytes differ only where the host cast wrapped an out-of-gamut value (a network after one epoch has many), and
        # there the device byte is saturated; byte-for-byte agreement inside the gamut is test_one_plane_form's subject
        a, b = (np.asarray(Image.open(os.path.join(str(tmp_path), r, cfg["experiment"], os.path.basename(tag)))).astype(int)
                for r in ("ev_plain", "ev_dev"))
        differ = a != b
        assert a.shape == b.shape and not differ.all()
        assert (np.isin(b[differ], (0, 255))).all()
