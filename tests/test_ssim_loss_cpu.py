"""Structural (SSIM) loss: the oracle and the analytic gradient in float64, handler plumbing and host-side argument checks
(no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sisr_amd
from sisr_amd import handlers, perceptual, structural

import _perceptual as P
import _ssim_loss as S
from _ssim_common import set5_y_pairs

CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- oracle and formula
def test_float64_oracle_is_the_metric_on_set5():
    """the grouped-conv2d oracle in float64 on the Set5 Y pairs equals metrics.ssim, the host restatement of scikit-image, to
    1e-12 (the bound tests/test_ssim_cpu.py holds the same two forms to)"""
    pairs = set5_y_pairs()
    assert len(pairs) == 5
    for name, hr, lr in pairs:
        want = sisr_amd.metrics.ssim(hr, lr)
        got = float(S.ssim_mean(torch.from_numpy(np.ascontiguousarray(lr)).double()[None, None],
                                torch.from_numpy(np.ascontiguousarray(hr)).double()[None, None]))
        assert abs(got - want) <= 1e-12, (name, got, want)


def test_oracle_taps_are_the_metrics():
    assert np.array_equal(S.taps().numpy(), sisr_amd.metrics.ssim_taps())


@pytest.mark.parametrize("shape", [(2, 3, 11, 11), (1, 1, 23, 140)])
@pytest.mark.parametrize("noise", [0.05, 0.002])
def test_analytic_gradient_is_float64_autograd(shape, noise):
    """the formula the kernels implement (alpha, beta, gamma maps through the transposed Gaussian) against float64 autograd of
    the oracle: 1e-12 relative L2"""
    sr, y = (t.double() for t in S.make_pair(shape, noise))
    _, want = S.autograd_grad(sr, y)
    got = S.analytic_grad(sr, y)
    assert got.shape == sr.shape
    e = S.rel_l2(got, want)
    print(f"analytic gradient {shape} noise {noise}: rel L2 {e:.3e}")
    assert e <= 1e-12, e
    # another data range scales the constants only
    _, want = S.autograd_grad(255 * sr, 255 * y, data_range=255.0)
    assert S.rel_l2(S.analytic_grad(255 * sr, 255 * y, data_range=255.0), want) <= 1e-12


def test_oracle_is_one_on_equal_images_and_in_range_on_the_test_inputs():
    for shape, noise in S.CASES:
        sr, y = (t.double() for t in S.make_pair(shape, noise))
        assert float(S.ssim_mean(y, y)) == 1.0
        assert 0.5 <= float(S.ssim_mean(sr, y)) < 1.0, (shape, noise)


# ----------------------------------------------------------------------------- criterion module
def test_mechanism_keeps_the_base_as_a_submodule_and_has_no_parameters():
    base = handlers.L1Loss()
    m = structural.StructuralMechanism(base, 0.2, data_range=2.0)
    assert m.base is base and m.alpha == 0.2 and m.data_range == 2.0
    assert list(m.parameters()) == [] and list(m.state_dict()) == []
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ssim_loss"):
            structural.StructuralMechanism(base, bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="ssim_data_range"):
            structural.StructuralMechanism(base, 0.1, data_range=bad)


# ----------------------------------------------------------------------------- handler wiring
def test_ssim_loss_wraps_the_l1_criterion(tmp_path):
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ssim_loss=0.1)
    assert isinstance(h.criterion, structural.StructuralMechanism)
    assert type(h.criterion.base) is handlers.L1Loss and h.criterion.alpha == 0.1 and h.criterion.data_range == 1.0
    assert h.ssim_loss == 0.1 and h.ssim_data_range == 1.0
    assert list(h.criterion.parameters()) == []
    state = h.save_model("m", 0, extract_state_only=True)
    assert set(state["network"]) == set(h.net.state_dict())
    h2 = handlers.RCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ssim_loss=0.3, ssim_data_range=255.0)
    assert isinstance(h2.criterion, structural.StructuralMechanism) and h2.criterion.data_range == 255.0


def test_ssim_loss_wraps_the_mse_criterion_of_the_y_channel_handlers(tmp_path):
    for cls in (sisr_amd.basic.SRCNNHandler, sisr_amd.basic.VDSRHandler):
        h = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ssim_loss=0.1)
        assert isinstance(h.criterion, structural.StructuralMechanism), cls.__name__
        assert type(h.criterion.base) is sisr_amd.basic.MSELoss, cls.__name__
        h0 = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False)
        assert type(h0.criterion) is sisr_amd.basic.MSELoss, cls.__name__


def test_ssim_loss_wraps_the_perceptual_criterion_when_both_are_given(tmp_path, monkeypatch):
    monkeypatch.delenv("SISR_VGG19_WEIGHTS", raising=False)
    path = str(tmp_path / "vgg.pth")
    torch.save(P.seeded_state(3, "vgg19_54"), path)
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, perceptual=0.05,
                             perceptual_weights=path, ssim_loss=0.1)
    assert isinstance(h.criterion, structural.StructuralMechanism)
    assert isinstance(h.criterion.base, perceptual.PerceptualMechanism) and h.criterion.base.lambda_per == 0.05
    assert list(h.criterion.state_dict()) == ["base.vgg_extractor." + k for k in P.state_keys()]
    vgg = {id(p) for p in h.criterion.parameters()}
    assert len(vgg) == 32 and not vgg & {id(p) for grp in h.optimizer.param_groups for p in grp["params"]}


def test_meta_attention_and_kwargs_networks_take_the_keys(tmp_path):
    """QRCANHandler and the SPARNet / SRMD handlers hand their **kwargs on to the network as well: `ssim_loss` and
    `ssim_data_range` must pass through both, as `perceptual_weights` does"""
    h = handlers.QRCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ssim_loss=0.1, ssim_data_range=1.0,
                              n_resgroups=1, n_resblocks=1)
    assert isinstance(h.criterion, structural.StructuralMechanism) and type(h.criterion.base) is handlers.L1Loss
    h = handlers.QEDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ssim_loss=0.1, num_blocks=1)
    assert isinstance(h.criterion, structural.StructuralMechanism) and type(h.criterion.base) is handlers.L1Loss
    small = dict(min_ch=32, max_ch=32, in_size=16, out_size=16, min_feat_size=8, res_depth=1)
    for cls, extra in ((sisr_amd.sparnet.SPARNetHandler, {}), (sisr_amd.sparnet.QSPARNetHandler, {"metadata": ["blur_sigma"]})):
        h = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ssim_loss=0.1, ssim_data_range=1.0, **small, **extra)
        assert isinstance(h.criterion, structural.StructuralMechanism), cls.__name__
        assert type(h.criterion.base) is handlers.L1Loss, cls.__name__
    h = sisr_amd.srmd.SRMDHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ssim_loss=0.1, ssim_data_range=1.0,
                                  metadata=["blur_sigma"], nb=1, nc=64)
    assert isinstance(h.criterion, structural.StructuralMechanism)


def test_unset_and_zero_leave_the_criterion_as_it_is(tmp_path):
    for v in (None, 0, 0.0):
        h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ssim_loss=v)
        assert type(h.criterion) is handlers.L1Loss, v
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1)
    assert type(h.criterion) is handlers.L1Loss and h.ssim_loss is None


def test_negative_weight_raises(tmp_path):
    with pytest.raises(ValueError, match="ssim_loss"):
        handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ssim_loss=-0.1)
    with pytest.raises(ValueError, match="ssim_loss"):
        sisr_amd.basic.VDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ssim_loss=-1)


def test_eval_mode_does_not_wrap(tmp_path):
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=True, num_blocks=1, ssim_loss=0.1)
    assert type(h.criterion) is handlers.L1Loss
    h = sisr_amd.basic.SRCNNHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=True, ssim_loss=0.1)
    assert type(h.criterion) is sisr_amd.basic.MSELoss


# ----------------------------------------------------------------------------- entry points and operator
def test_entry_points_refuse_bad_arguments_before_any_device_call():
    """sisr_ssim_loss validates on the host and returns an error code: no launch is made, so this runs without a GPU (the
    pointers are host stand-ins that must never be dereferenced)"""
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    ERR_ARG, ERR_ALIGN = -1, -2
    wsb = L.sisr_ssim_loss_workspace_bytes
    # 2 planes of 43 x 75: 33 x 65 windows = 2 x 2 tiles per plane, 8 doubles; with a gradient three float64 maps more
    assert wsb(2, 43, 75, 0) == 2 * 4 * 8
    assert wsb(2, 43, 75, 1) == 2 * 4 * 8 + 3 * 2 * 33 * 65 * 8
    assert wsb(1, 11, 11, 0) == 16 and wsb(1, 11, 11, 1) == 16 + 24  # one tile sum, padded to 16 bytes
    assert wsb(0, 43, 75, 1) == 0 and wsb(1, 10, 75, 1) == 0 and wsb(1, 43, 10, 0) == 0 and wsb(-1, 43, 75, 0) == 0
    big = 1 << 30
    f = L.sisr_ssim_loss
    # null operands
    assert f(None, a, 1, 16, 16, 1.0, a, a, a, big, None) == ERR_ARG
    assert f(a, None, 1, 16, 16, 1.0, a, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 16, 16, 1.0, None, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 16, 16, 1.0, a, a, None, big, None) == ERR_ARG
    # planes <= 0, a side below the window
    assert f(a, a, 0, 16, 16, 1.0, a, a, a, big, None) == ERR_ARG
    assert f(a, a, -3, 16, 16, 1.0, a, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 10, 16, 1.0, a, a, a, big, None) == ERR_ARG
    assert f(a, a, 1, 16, 10, 1.0, a, a, a, big, None) == ERR_ARG
    # data_range not finite or <= 0
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert f(a, a, 1, 16, 16, r, a, a, a, big, None) == ERR_ARG, r
    # workspace too small: for the value alone, and for the gradient's maps
    assert f(a, a, 1, 16, 16, 1.0, a, None, a, wsb(1, 16, 16, 0) - 1, None) == ERR_ARG
    assert f(a, a, 1, 16, 16, 1.0, a, a, a, wsb(1, 16, 16, 1) - 1, None) == ERR_ARG
    assert f(a, a, 1, 16, 16, 1.0, a, a, a, wsb(1, 16, 16, 0), None) == ERR_ARG
    # misaligned pointers
    assert f(a, a, 1, 16, 16, 1.0, a, a, a + 8, big, None) == ERR_ALIGN
    assert f(a + 2, a, 1, 16, 16, 1.0, a, a, a, big, None) == ERR_ALIGN
    assert f(a, a + 1, 1, 16, 16, 1.0, a, a, a, big, None) == ERR_ALIGN
    assert f(a, a, 1, 16, 16, 1.0, a + 2, a, a, big, None) == ERR_ALIGN
    assert f(a, a, 1, 16, 16, 1.0, a, a + 2, a, big, None) == ERR_ALIGN


def test_operator_has_no_cpu_path_and_names_the_window_limit():
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP device"):
        sisr_amd.ops.ssim_mean(x, x.clone())
    for shape in ((1, 1, 10, 16), (1, 1, 16, 10)):
        t = torch.rand(shape)
        with pytest.raises(ValueError, match="at least 11"):
            sisr_amd.ops.ssim_mean(t, t.clone())
    with pytest.raises(RuntimeError, match="one shape"):
        sisr_amd.ops.ssim_mean(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 17))
    with pytest.raises(RuntimeError, match="one shape"):
        sisr_amd.ops.ssim_mean(torch.rand(3, 16, 16), torch.rand(3, 16, 16))