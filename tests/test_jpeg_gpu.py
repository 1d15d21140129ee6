"""The JPEG degradation kernel (csrc/jpeg.hip) and the data path around it on a real MI355X (pytest -m gpu): byte-identical
to Pillow's `save(buf, "JPEG", subsampling=0, quality=q)` + `open` (ref: sr_tools/data_converter.py:178-194)."""
import os
import random

import numpy as np
import pytest
import torch

import sisr_amd
from conftest import GOLDEN
import _jpeg as J

pytestmark = pytest.mark.gpu
D = sisr_amd.degrade
CANARY = 0xA5


def _in_canary(dev_img, quality, to_float):
    """sisr_jpeg_roundtrip with its output placed inside a larger buffer: -> (the output, the buffer's bytes around it)."""
    C, H, W = dev_img.shape
    item = 4 if to_float else 1
    n, guard = C * H * W * item, 4096
    buf = torch.full((guard + n + guard,), CANARY, dtype=torch.uint8, device="cuda")
    out = buf[guard:guard + n]
    assert out.data_ptr() % 4 == 0
    sisr_amd.hip.check(sisr_amd.hip.lib().sisr_jpeg_roundtrip(dev_img.data_ptr(), out.data_ptr(), C, H, W, quality, int(to_float),
                                                              sisr_amd.hip.stream()), "sisr_jpeg_roundtrip")
    host = buf.cpu().numpy()
    res = host[guard:guard + n].view(np.float32 if to_float else np.uint8).reshape(C, H, W)
    return res, np.concatenate((host[:guard], host[guard + n:]))


@pytest.mark.parametrize("C", [3, 1])
def test_kernel_is_byte_identical_to_pillow(C):
    """Every size (below a block, across block edges, whole blocks, more than one workgroup at 64 x 96), quality and pattern,
    both output forms; the output sits in a canary buffer and nothing around it may change."""
    for label, img, q in J.cases(C, J.SIZES + [(64, 96)]):
        want = J.pil_roundtrip(img, q)
        dev = torch.from_numpy(img).cuda()
        got, around = _in_canary(dev, q, False)
        assert np.array_equal(got, want), (label, C, q, int((got != want).sum()))
        assert (around == CANARY).all(), (label, C, q, "uint8 form wrote outside [C][H][W]")
        gotf, around = _in_canary(dev, q, True)
        assert np.array_equal(gotf, want.astype(np.float32) / np.float32(255)), (label, C, q)
        assert (around == CANARY).all(), (label, C, q, "fp32 form wrote outside [C][H][W]")


def test_python_surface_and_repeatability():
    img = J.baby()
    dev = torch.from_numpy(img).cuda()
    want = J.pil_roundtrip(img, 40)
    f = D.jpeg_roundtrip(dev, 40)
    u = D.jpeg_roundtrip(dev, 40, to_float=False)
    assert f.dtype == torch.float32 and u.dtype == torch.uint8 and f.shape == u.shape == dev.shape
    assert np.array_equal(u.cpu().numpy(), want) and torch.equal(f, D.jpeg_roundtrip(dev, 40))
    assert np.array_equal(f.cpu().numpy(), want.astype(np.float32) / np.float32(255))
    assert np.array_equal(D.jpeg_roundtrip(dev[:, 3:40, 5:50], 40, to_float=False).cpu().numpy(),  # a view: made contiguous
                          J.pil_roundtrip(np.ascontiguousarray(img[:, 3:40, 5:50]), 40))
    with pytest.raises(ValueError):
        D.jpeg_roundtrip(dev, 0)
    with pytest.raises(ValueError):
        D.jpeg_roundtrip(dev.float(), 50)


def _hr(name="butterfly.png"):
    from PIL import Image
    hr = np.asarray(Image.open(os.path.join(GOLDEN, "set5", "hr", name)).convert("RGB"))
    return torch.from_numpy(hr.transpose(2, 0, 1).copy()).float().div(255).cuda()


@pytest.mark.parametrize("noise", [False, True])
def test_degrader_with_jpeg_is_pillows_round_trip_of_the_plain_degraders_bytes(noise):
    """The quality is the last draw, so the same seed with jpeg off gives the bytes that go into the compression."""
    pca = torch.from_numpy(np.random.RandomState(0).randn(441, 10).astype(np.float32))
    kw = dict(scale=4, pca=pca, noise=noise)
    x = _hr()
    np.random.seed(31)
    lr, code, kernel, box = D.OnlineDegrader(jpeg=True, jpeg_quality=[30, 90], **kw)(x)
    np.random.seed(31)
    lr0, code0, kernel0, box0 = D.OnlineDegrader(jpeg=False, **kw)(x)
    q = int(np.random.randint(30, 91))
    pre = (lr0.cpu().numpy() * np.float32(255)).round().astype(np.uint8)
    assert np.array_equal(pre.astype(np.float32) / np.float32(255), lr0.cpu().numpy())
    assert np.array_equal(lr.cpu().numpy(), J.pil_roundtrip(pre, q).astype(np.float32) / np.float32(255))
    assert torch.equal(kernel, kernel0) and box == box0 and torch.equal(code[:-1], code0)
    assert code.dtype == torch.float32 and code[-1].item() == np.float32((q - 30) / 60)
    assert not torch.equal(lr, lr0)


def test_device_tile_loader_with_jpeg_equals_the_dataloader_path(monkeypatch):
    """As test_degrade_gpu's loader test, with the JPEG stage on: same batches from DeviceTileLoader and from
    DataLoader(shuffle=True, num_workers=0) over SuperResImages.__getitem__ under the same seeds."""
    from torch.utils.data import DataLoader
    real = D.pca_matrix
    monkeypatch.setattr(D, "pca_matrix", lambda batch=2000, k=10: real(batch=2000, k=k))
    hr_dir = os.path.join(GOLDEN, "set5", "hr")
    keys = ["blur_kernel"] * 10 + ["jpeg_quality"]

    def dataset():
        np.random.seed(5)
        return sisr_amd.data.SuperResImages(hr_dir=hr_dir, online_degradations=True, split="all", scale=4, random_crop=24,
                                            random_augments=True,
                                            online_degradation_params=dict(jpeg=True, jpeg_quality=[30, 90]))

    def seed():
        torch.manual_seed(3)
        np.random.seed(6)
        random.seed(7)

    host_loader = DataLoader(dataset=dataset(), batch_size=2, shuffle=True, num_workers=0)
    dev_loader = sisr_amd.data.DeviceTileLoader([dataset()], 2, torch.device("cuda:0"))
    seed()
    host = list(host_loader)
    seed()
    dev = list(dev_loader)
    assert len(host) == len(dev) == 3
    tails = []
    for a, b in zip(host, dev):
        assert list(a["tag"]) == list(b["tag"]) and list(a["hr_tag"]) == list(b["hr_tag"])
        assert torch.equal(a["lr"], b["lr"].cpu()) and torch.equal(a["hr"], b["hr"].cpu())
        assert torch.equal(a["metadata"], b["metadata"]) and a["metadata"].dtype == b["metadata"].dtype
        assert a["metadata"].shape[1] == 11
        assert torch.equal(a["blur_kernels"], b["blur_kernels"])
        assert [tuple(k) for k in a["metadata_keys"]] == [tuple(k) for k in b["metadata_keys"]]
        assert [k[0] for k in b["metadata_keys"]] == keys
        tails += a["metadata"][:, -1].tolist()
    assert all(0.0 <= t <= 1.0 for t in tails) and len(set(tails)) > 1


def test_reduced_qedsr_trains_on_a_jpeg_batch(monkeypatch):
    """metadata = ['blur_kernel', 'jpeg_quality'] selects the 11 values by key; one train_step gives a finite loss."""
    real = D.pca_matrix
    monkeypatch.setattr(D, "pca_matrix", lambda batch=2000, k=10: real(batch=2000, k=k))
    np.random.seed(5)
    ds = sisr_amd.data.SuperResImages(hr_dir=os.path.join(GOLDEN, "set5", "hr"), online_degradations=True, split="all", scale=4,
                                      random_crop=24, random_augments=True,
                                      online_degradation_params=dict(jpeg=True, jpeg_quality=[30, 90]))
    torch.manual_seed(3)
    random.seed(7)
    batch = next(iter(sisr_amd.data.DeviceTileLoader([ds], 2, torch.device("cuda:0"))))
    torch.manual_seed(8)
    h = sisr_amd.available_models["qedsr"](device=0, model_save_dir="/tmp", eval_mode=False, scale=4, num_blocks=2,
                                           metadata=["blur_kernel", "jpeg_quality"])
    assert h.num_metadata == 11
    ch = h.generate_channels(batch["lr"], batch["metadata"], batch["metadata_keys"])
    assert ch.shape == (2, 11, 1, 1) and torch.equal(ch[:, :, 0, 0], batch["metadata"].float())
    loss, out = h.train_step(batch["lr"], batch["hr"], metadata=batch["metadata"], metadata_keys=batch["metadata_keys"])
    assert out.shape == batch["hr"].shape and torch.isfinite(loss).item() and loss.item() > 0
