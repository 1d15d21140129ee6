"""Geometric self-ensemble on the HIP path: the two kernels of csrc/ensemble.hip against the host form of ensemble.py, bit for
bit; run_eval(self_ensemble=True) against a stand-in forward and, for real reduced networks, against the same computation
laid out by hand (host-form variants, plain run_eval at the same batch shapes, host-form merge); eval_sisr's config key."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _basic as R
import sisr_amd
from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
E = sisr_amd.ensemble
DEV = "cuda:0"
SET5 = os.path.join(GOLDEN, "set5")
# aligned | both sizes off-tile, w no multiple of 4 | single row | single column | tile + 1 and tile - 1, odd c | several
# tiles each way.  Between them: every pairing of the 16-byte and the lane-by-lane forms (w % 4, h % 4 each zero and not)
SHAPES = [(1, 3, 64, 64), (2, 3, 37, 70), (1, 1, 1, 65), (1, 1, 65, 1), (3, 5, 33, 31), (1, 3, 128, 96)]


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _nan(shape):
    return torch.full(shape, float("nan"), device=DEV)


@pytest.mark.parametrize("shape", SHAPES)
def test_fan_kernel_equals_the_host_form_bit_for_bit(shape):
    n, c, h, w = shape
    x = _rand(shape, 100 + h)
    want_up, want_tu = E.dihedral_fan(x)
    up, tu = E.dihedral_fan(x.to(DEV))
    assert up.is_cuda and tu.is_cuda and up.shape == want_up.shape and tu.shape == want_tu.shape
    assert torch.equal(up.cpu(), want_up) and torch.equal(tu.cpu(), want_tu)
    # the entry point itself into buffers full of NaN: an element it does not write stays NaN and fails
    L, hip, xd = sisr_amd.hip.lib(), sisr_amd.hip, x.to(DEV)
    up, tu = _nan((4 * n, c, h, w)), _nan((4 * n, c, w, h))
    assert L.sisr_dihedral_fan(hip.ptr(xd), n, c, h, w, hip.ptr(up), hip.ptr(tu), hip.stream()) == 0
    assert torch.equal(up.cpu(), want_up) and torch.equal(tu.cpu(), want_tu)


@pytest.mark.parametrize("shape", SHAPES)
def test_merge_kernel_equals_the_host_form_bit_for_bit(shape):
    """eight independent random maps (not fanned copies), of spread magnitudes: a wrong inverse or another order of the adds
    moves bits"""
    n, c, H, W = shape
    scale = torch.tensor([10.0 ** (k - 2) for k in range(4)]).repeat_interleave(n).view(4 * n, 1, 1, 1)
    up, tu = _rand((4 * n, c, H, W), 200 + H) * scale, _rand((4 * n, c, W, H), 300 + H) * scale * 3
    want = E.dihedral_merge(up, tu)
    got = E.dihedral_merge(up.to(DEV), tu.to(DEV))
    assert got.is_cuda and torch.equal(got.cpu(), want)
    L, hip, ud, td = sisr_amd.hip.lib(), sisr_amd.hip, up.to(DEV), tu.to(DEV)
    out = _nan((n, c, H, W))
    assert L.sisr_dihedral_merge(hip.ptr(ud), hip.ptr(td), n, c, H, W, hip.ptr(out), hip.stream()) == 0
    assert torch.equal(out.cpu(), want)


def test_kernels_take_misaligned_bases():
    """a batch that starts 4 bytes into an allocation: rows of a multiple of 4 floats, yet no 16-byte access is allowed"""
    x = _rand((1, 2, 8, 12), 7)
    flat = torch.empty(x.numel() + 1, device=DEV)
    xd = flat[1:].view(x.shape)
    xd.copy_(x)
    assert xd.data_ptr() % 16 == 4
    want = E.dihedral_fan(x)
    up, tu = E.dihedral_fan(xd)
    assert torch.equal(up.cpu(), want[0]) and torch.equal(tu.cpu(), want[1])
    fu, ft = torch.empty(up.numel() + 1, device=DEV), torch.empty(tu.numel() + 3, device=DEV)
    u2, t2 = fu[1:].view(up.shape), ft[3:].view(tu.shape)
    u2.copy_(up), t2.copy_(tu)
    assert torch.equal(E.dihedral_merge(u2, t2).cpu(), x)


def _handler(name, **kw):
    torch.manual_seed(8)
    return sisr_amd.available_models[name](device=0, model_save_dir="/tmp", eval_mode=True, **kw)


def test_run_eval_with_a_stand_in_forward_equals_the_plain_run():
    """a reduced RCAN handler (the 16-feature configuration of the reduced-net fixtures) whose run_model is nearest-neighbour
    x4 on the device: pointwise, so it commutes with every variant and the ensemble of it is the plain result, exactly"""
    h = _handler("rcan", scale=4)
    _, meta = load_golden("g2_rcan")
    h.net = sisr_amd.architectures.RCAN(**meta).to(DEV)
    calls = []

    def stand_in(t, *a, **k):
        calls.append(tuple(t.shape))
        assert t.is_cuda
        return F.interpolate(t, scale_factor=4, mode="nearest")
    h.run_model = stand_in
    x, y = _rand((2, 3, 24, 40), 31), _rand((2, 3, 96, 160), 32)
    plain, loss0, _ = h.run_eval(x, y, request_loss=True)
    plus, loss1, secs = h.run_eval(x, y, request_loss=True, timing=True, self_ensemble=True)
    assert calls == [(2, 3, 24, 40), (8, 3, 24, 40), (8, 3, 40, 24)]
    assert torch.equal(plain, plus) and float(loss0) == float(loss1) and secs > 0
    assert torch.equal(plain, F.interpolate(x, scale_factor=4, mode="nearest"))
    on_dev, _, _ = h.run_eval(x, keep_on_device=True, self_ensemble=True)
    assert on_dev.is_cuda and torch.equal(on_dev.cpu(), plain)


def _manual_form_equality(h, x, md=None, keys=None):
    """run_eval(self_ensemble=True) against the same computation laid out by hand: the 4n upright and 4n turned batches made
    with the host form and uploaded, plain run_eval on each, the host-form merge.  The network sees identical inputs at
    identical batch shapes both ways, so nothing but equality will do -- given a forward that repeats itself, which is
    asserted first."""
    def run(t, **extra):
        kw = {} if md is None else dict(metadata=md.repeat(t.shape[0] // md.shape[0], 1),
                                        metadata_keys=[k * (t.shape[0] // md.shape[0]) for k in keys])
        return h.run_eval(t, **kw, **extra)[0]
    first, second = run(x), run(x)
    assert torch.equal(first, second), "the plain forward is not reproducible run to run"
    up, tu = E.dihedral_fan(x)  # host form
    want = E.dihedral_merge(run(up), run(tu))
    got = run(x, self_ensemble=True)
    assert got.shape == first.shape and not got.is_cuda
    assert torch.equal(got, want)
    # (and the ensemble is no stand-in for the plain forward: a real network does not commute with the variants)
    assert not torch.equal(got, first)
    return got


def test_reduced_edsr_equals_the_manual_form():
    h = _handler("edsr", scale=4, num_features=16, num_blocks=2)
    _manual_form_equality(h, torch.rand((2, 3, 24, 40), generator=torch.Generator().manual_seed(41)))


def test_reduced_qrcan_with_metadata_equals_the_manual_form():
    h = _handler("qrcan", scale=4, n_feats=16, n_resgroups=2, n_resblocks=2, reduction=16, metadata=["blur_kernel"],
                 style="standard", include_q_layer=True)
    g = torch.Generator().manual_seed(42)
    x = torch.rand((2, 3, 24, 40), generator=g)
    md = torch.rand(2, 10, generator=g, dtype=torch.float64) * 0.4
    _manual_form_equality(h, x, md, [("blur_kernel",) * 2] * 10)


def test_reduced_vdsr_y_channel_equals_the_manual_form():
    """c = 1, output size = input size"""
    h = _handler("vdsr", kernel_pattern=[3] * 4, channel_pattern=[1, 64, 64, 64, 1])
    out = _manual_form_equality(h, torch.rand((1, 1, 40, 24), generator=torch.Generator().manual_seed(43)))
    assert out.shape == (1, 1, 40, 24)


def test_reduced_sparnet_same_size_equals_the_manual_form():
    h = _handler("sparnet", scale=1, min_ch=32, max_ch=128, in_size=32, out_size=32, min_feat_size=8, res_depth=1,
                 bottleneck_size=32)
    out = _manual_form_equality(h, torch.rand((1, 3, 128, 128), generator=torch.Generator().manual_seed(44)))
    assert out.shape == (1, 3, 128, 128)


def test_reduced_san_chopped_eval_equals_the_manual_form():
    """through _ChoppedEval: 28 x 36 chops once into four 24 x 28 tiles (672 positions < max_combined_im_size = 1000), and the
    turned batch into four 28 x 24 ones"""
    h = _handler("san", scale=4, max_combined_im_size=1000)
    torch.manual_seed(8)
    h.net = sisr_amd.san.SAN(n_resgroups=2, n_resblocks=2, scale=4).to(DEV)
    seen = []
    real = h.net.forward
    h.net.forward = lambda t, *a, **k: (seen.append(tuple(t.shape)), real(t, *a, **k))[1]
    out = _manual_form_equality(h, torch.rand((1, 3, 28, 36), generator=torch.Generator().manual_seed(45)))
    assert out.shape == (1, 3, 112, 144)
    assert set(seen) == {(1, 3, 24, 28), (4, 3, 24, 28), (4, 3, 28, 24)}


# ----------------------------------------------------------------------------- eval_sisr
def _eval(tmp_path, cfg, total, name, **kw):
    last = len(total["epoch"]) - 1
    return sisr_amd.cli.eval_sisr(model_and_epoch=[[cfg["experiment"], str(last)]], model_loc=str(tmp_path), gpu=True,
                                  hr_dir=os.path.join(SET5, "hr"), lr_dir=os.path.join(SET5, "lr_random_blur"),
                                  full_directory=True, scale=4, out_loc=str(tmp_path), results_name=name, time_models=False,
                                  lr_baseline=True, **kw)


def test_eval_sisr_self_ensemble_key(tmp_path):
    """a tiny trained srcnn experiment (as tests/test_interp_gpu.py builds its own) evaluated from the raw LR folder"""
    import pandas as pd
    cli, M = sisr_amd.cli, sisr_amd.metrics
    cfg = R.b4_config(tmp_path)
    cfg["training"].update(gpu="single", sp_gpu=0)
    total = cli.train_sisr(cfg)
    name = cfg["experiment"]
    df, avg = _eval(tmp_path, cfg, total, "ev_plus", self_ensemble=True, save_im=True)
    assert sorted(set(df["Model"])) == ["LR", name + "+"] and sorted(avg["Model"]) == ["LR", name + "+"]
    assert len(df[df["Model"] == name + "+"]) == 5
    assert len(os.listdir(os.path.join(str(tmp_path), "ev_plus", name + "+"))) == 5  # the saved images
    assert not os.path.exists(os.path.join(str(tmp_path), "ev_plus", name))

    # PSNR per image = the value of net_run_and_process(..., self_ensemble=True) on the same feed
    m = sisr_amd.ModelInterface(str(tmp_path), name, gpu="single", sp_gpu=0, mode="eval", load_epoch=len(total["epoch"]) - 1)
    data = sisr_amd.data.SuperResImages(os.path.join(SET5, "lr_random_blur"), os.path.join(SET5, "hr"), split="all", scale=4)
    want, plain = {}, {}
    for batch in torch.utils.data.DataLoader(dataset=data, batch_size=1):
        _, ycc, _ = cli._interpolated(batch["lr"], 4, torch.device("cuda", 0), True, False)
        feed = {**batch, "lr": ycc, "hr": torch.stack([sisr_amd.data.rgb_to_ycbcr(im, y_only=False) for im in batch["hr"]])}
        hr_y = sisr_amd.ModelInterface.colorspace_convert(batch["hr"], colorspace="rgb")[0, 0]
        want[batch["tag"][0]] = M.psnr(m.net_run_and_process(**feed, self_ensemble=True)[1][0, 0], hr_y, 1)
        plain[batch["tag"][0]] = M.psnr(m.net_run_and_process(**feed)[1][0, 0], hr_y, 1)
    mine = df[df["Model"] == name + "+"]
    assert dict(zip(mine["Image_Name"], mine["PSNR"])) == want
    assert want != plain  # (the ensemble moves the numbers)

    # key absent = key false = the CSVs of before: the plain model name and the plain numbers
    read = lambda run, f: open(os.path.join(str(tmp_path), run, "standard_metrics", f), "rb").read()  # noqa: E731
    df0, _ = _eval(tmp_path, cfg, total, "ev_absent")
    _eval(tmp_path, cfg, total, "ev_false", self_ensemble=False)
    for f in ("individual_metrics.csv", "average_metrics.csv"):
        assert read("ev_absent", f) == read("ev_false", f)
    ours = df0[df0["Model"] == name]
    assert sorted(set(df0["Model"])) == ["LR", name] and dict(zip(ours["Image_Name"], ours["PSNR"])) == plain
    lr_rows = lambda d: d[d["Model"] == "LR"].reset_index(drop=True)  # noqa: E731
    pd.testing.assert_frame_equal(lr_rows(df0), lr_rows(df))  # the LR baseline rows are unaffected
