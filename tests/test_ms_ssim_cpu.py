"""Multi-scale SSIM: the oracle and the analytic gradient in float64, the host metric, handler plumbing and host-side
argument checks (no GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sisr_amd
from sisr_amd import frequency, handlers, multiscale, perceptual, structural

import _ms_ssim as MS
import _perceptual as P
import _ssim_loss as S
from _ssim_common import set5_y_pairs

CPU = torch.device("cpu")


# ----------------------------------------------------------------------------- oracle, formula, host metric
@pytest.mark.parametrize("case", MS.CASES, ids=MS.CASE_IDS)
def test_analytic_gradient_is_float64_autograd(case):
    """the formula the kernels implement (per-scale coefficient maps through the transposed Gaussian, the per-plane factors
    w_j MS / (c_j windows_j planes), a quarter of the parent pixel from the coarser scale) against float64 autograd of the
    oracle: 1e-12 relative L2, at data ranges 1 and 255"""
    sr, y, weights = MS.make_case(case)
    sr, y = sr.double(), y.double()
    _, _, want = MS.autograd_grad(sr, y, weights)
    got = MS.analytic_grad(sr, y, weights)
    assert got.shape == sr.shape
    e = S.rel_l2(got, want)
    print(f"analytic gradient {case}: rel L2 {e:.3e}")
    assert e <= 1e-12, e
    _, _, want = MS.autograd_grad(255 * sr, 255 * y, weights, data_range=255.0)
    e = S.rel_l2(MS.analytic_grad(255 * sr, 255 * y, weights, data_range=255.0), want)
    assert e <= 1e-12, e


def test_host_metric_is_the_oracle_on_set5():
    pairs = set5_y_pairs()
    assert len(pairs) == 5
    for name, hr, lr in pairs:
        assert min(hr.shape) >= 176, (name, hr.shape)
        want = float(MS.ms_ssim(torch.from_numpy(np.ascontiguousarray(lr)).double()[None, None],
                                torch.from_numpy(np.ascontiguousarray(hr)).double()[None, None])[1])
        got = sisr_amd.metrics.ms_ssim(lr, hr)
        assert abs(got - want) <= 1e-12, (name, got, want)


def test_one_weight_of_one_is_the_single_scale_metric():
    for name, hr, lr in set5_y_pairs():
        assert abs(sisr_amd.metrics.ms_ssim(lr, hr, weights=(1.0,)) - sisr_amd.metrics.ssim(lr, hr)) <= 1e-12, name


def test_default_weights_are_the_papers_and_shared():
    assert sisr_amd.metrics.MS_SSIM_WEIGHTS == MS.WEIGHTS == sisr_amd.ops.MS_SSIM_WEIGHTS
    assert sisr_amd.ops.ms_ssim_min_side(5) == 176 and sisr_amd.ops.ms_ssim_min_side(4) == 88


def test_oracle_is_one_on_equal_images_and_in_range_on_the_test_inputs():
    for case in MS.CASES:
        sr, y, weights = MS.make_case(case)
        sr, y = sr.double(), y.double()
        per, v = MS.ms_ssim(y, y, weights)
        assert float(v) == 1.0 and bool((per == 1.0).all())
        per, v = MS.ms_ssim(sr, y, weights)
        assert 0.5 <= float(v) < 1.0 and bool(((per >= 0.5) & (per < 1.0)).all()), case
        for c in MS.scale_means(sr, y, len(weights)):
            assert bool(((c > 0.5) & (c <= 1.0)).all()), case


def test_an_anticorrelated_pair_has_a_negative_scale_mean_and_the_value_zero():
    _, y = S.make_pair((1, 1, 44, 44), 0.0)
    y = y.double()
    means = MS.scale_means(1 - y, y, 3)
    assert any(float(c.min()) < 0 for c in means)
    assert float(MS.ms_ssim(1 - y, y, MS.WEIGHTS[:3])[1]) == 0.0
    assert sisr_amd.metrics.ms_ssim((1 - y)[0, 0].numpy(), y[0, 0].numpy(), weights=MS.WEIGHTS[:3]) == 0.0
    assert bool((MS.analytic_grad(1 - y, y, MS.WEIGHTS[:3]) == 0).all())


def test_a_scale_mean_at_or_below_zero_zeroes_the_value_whatever_its_weight():
    """MS.checker_pair: c_0 < 0, c_1 = 1.  With weights (0, 1) the bare product max(c_0, 0)^0 * c_1 is 1; the rule `any
    c_j <= 0 -> 0` looks at the means, not at the weights, so the host metric and the gradient formula give exactly 0.  A
    positive weight on that scale gives 0 both ways; without that scale (weights (1,) on the pooled pair) the value is 1."""
    sr, y = (t.double() for t in MS.checker_pair())
    c0, c1 = (float(c) for c in MS.scale_means(sr, y, 2))
    assert c0 < 0 and abs(c1 - 1) <= 1e-9, (c0, c1)  # the float32 rounding of the pair survives the pooling
    assert float(MS.ms_ssim(sr, y, (0.0, 1.0))[1]) == pytest.approx(1.0, abs=1e-9)  # the bare product: not what is computed
    a, b = sr[0, 0].numpy(), y[0, 0].numpy()
    assert sisr_amd.metrics.ms_ssim(a, b, weights=(0.0, 1.0)) == 0.0
    assert sisr_amd.metrics.ms_ssim(a, b, weights=(0.5, 0.5)) == 0.0
    assert bool((MS.analytic_grad(sr, y, (0.0, 1.0)) == 0).all())
    # a zero weight on a scale whose mean is positive is max(c, 0)^0 = 1: the other scale's value alone
    _, y2 = S.make_pair((1, 1, 22, 22), 0.05)
    x2, y2 = (y2 + 0.05).double()[0, 0].numpy(), y2.double()[0, 0].numpy()
    one = sisr_amd.metrics.ms_ssim(x2, y2, weights=(0.0, 1.0))
    pooled = [t.reshape(11, 2, 11, 2).mean(axis=(1, 3)) for t in (x2, y2)]
    assert 0 < one < 1 and abs(one - sisr_amd.metrics.ssim(*pooled)) <= 1e-12


def test_host_metric_names_the_minimum_side():
    t = np.zeros((175, 300))
    with pytest.raises(ValueError, match="at least 176.*ms_ssim_weights"):
        sisr_amd.metrics.ms_ssim(t, t)
    with pytest.raises(ValueError, match="at least 176"):
        sisr_amd.metrics.batch_ms_ssim(np.zeros((1, 1, 300, 175), np.float32), np.zeros((1, 1, 300, 175), np.float32))
    assert sisr_amd.metrics.ms_ssim(t, t, weights=MS.WEIGHTS[:4]) == 1.0
    for bad in ((), (0.1,) * 9, (0.5, -0.1), (float("nan"),)):
        with pytest.raises(ValueError, match="ms_ssim_weights"):
            sisr_amd.metrics.ms_ssim(t, t, weights=bad)


# ----------------------------------------------------------------------------- criterion module
def test_mechanism_keeps_the_base_as_a_submodule_and_has_no_parameters():
    base = handlers.L1Loss()
    m = multiscale.MultiScaleStructuralMechanism(base, 0.2, data_range=2.0, weights=[0.5, 0.5])
    assert m.base is base and m.alpha == 0.2 and m.data_range == 2.0 and m.weights == (0.5, 0.5)
    assert multiscale.MultiScaleStructuralMechanism(base, 0.2).weights == MS.WEIGHTS
    assert list(m.parameters()) == [] and list(m.state_dict()) == []
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ms_ssim_loss"):
            multiscale.MultiScaleStructuralMechanism(base, bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="ssim_data_range"):
            multiscale.MultiScaleStructuralMechanism(base, 0.1, data_range=bad)
    for bad in ((), (0.1,) * 9, (0.5, -0.1), (float("inf"),), 3):
        with pytest.raises(ValueError, match="ms_ssim_weights"):
            multiscale.MultiScaleStructuralMechanism(base, 0.1, weights=bad)


# ----------------------------------------------------------------------------- handler wiring
def test_ms_ssim_loss_wraps_the_l1_criterion(tmp_path):
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ms_ssim_loss=0.1)
    assert isinstance(h.criterion, multiscale.MultiScaleStructuralMechanism)
    assert type(h.criterion.base) is handlers.L1Loss and h.criterion.alpha == 0.1 and h.criterion.data_range == 1.0
    assert h.criterion.weights == MS.WEIGHTS and h.ms_ssim_loss == 0.1 and h.ms_ssim_weights is None
    assert list(h.criterion.parameters()) == []
    state = h.save_model("m", 0, extract_state_only=True)
    assert set(state["network"]) == set(h.net.state_dict())
    h2 = handlers.RCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ms_ssim_loss=0.3, ssim_data_range=255.0,
                              ms_ssim_weights=[0.1, 0.2, 0.3, 0.4])
    assert isinstance(h2.criterion, multiscale.MultiScaleStructuralMechanism)
    assert h2.criterion.data_range == 255.0 and h2.criterion.weights == (0.1, 0.2, 0.3, 0.4)


def test_ms_ssim_loss_wraps_the_mse_criterion_of_the_y_channel_handlers(tmp_path):
    for cls in (sisr_amd.basic.SRCNNHandler, sisr_amd.basic.VDSRHandler):
        h = cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ms_ssim_loss=0.1, ms_ssim_weights=MS.WEIGHTS[:4])
        assert isinstance(h.criterion, multiscale.MultiScaleStructuralMechanism), cls.__name__
        assert type(h.criterion.base) is sisr_amd.basic.MSELoss and h.criterion.weights == MS.WEIGHTS[:4], cls.__name__


def test_ms_ssim_loss_wraps_the_perceptual_criterion_when_both_are_given(tmp_path, monkeypatch):
    monkeypatch.delenv("SISR_VGG19_WEIGHTS", raising=False)
    path = str(tmp_path / "vgg.pth")
    torch.save(P.seeded_state(3, "vgg19_54"), path)
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, perceptual=0.05,
                             perceptual_weights=path, ms_ssim_loss=0.1)
    assert isinstance(h.criterion, multiscale.MultiScaleStructuralMechanism)
    assert isinstance(h.criterion.base, perceptual.PerceptualMechanism) and h.criterion.base.lambda_per == 0.05
    assert list(h.criterion.state_dict()) == ["base.vgg_extractor." + k for k in P.state_keys()]


def test_the_three_terms_nest_in_order(tmp_path):
    """pixel base -> StructuralMechanism -> MultiScaleStructuralMechanism -> FrequencyMechanism, outermost last"""
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ssim_loss=0.1,
                             ms_ssim_loss=0.2, freq_loss=0.3)
    assert isinstance(h.criterion, frequency.FrequencyMechanism)
    assert isinstance(h.criterion.base, multiscale.MultiScaleStructuralMechanism) and h.criterion.base.alpha == 0.2
    assert isinstance(h.criterion.base.base, structural.StructuralMechanism) and h.criterion.base.base.alpha == 0.1
    assert type(h.criterion.base.base.base) is handlers.L1Loss


def test_meta_attention_and_kwargs_networks_take_the_keys(tmp_path):
    """the handlers that hand their **kwargs on to the network let `ms_ssim_loss` and `ms_ssim_weights` through"""
    keys = dict(ms_ssim_loss=0.1, ms_ssim_weights=[0.5, 0.5])

    def check(h):
        assert isinstance(h.criterion, multiscale.MultiScaleStructuralMechanism), type(h).__name__
        assert type(h.criterion.base) is handlers.L1Loss and h.criterion.weights == (0.5, 0.5), type(h).__name__
    check(handlers.QRCANHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, n_resgroups=1, n_resblocks=1, **keys))
    check(handlers.QEDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, **keys))
    small = dict(min_ch=32, max_ch=32, in_size=16, out_size=16, min_feat_size=8, res_depth=1)
    for cls, extra in ((sisr_amd.sparnet.SPARNetHandler, {}), (sisr_amd.sparnet.QSPARNetHandler, {"metadata": ["blur_sigma"]})):
        check(cls(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, **keys, **small, **extra))
    check(sisr_amd.srmd.SRMDHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, metadata=["blur_sigma"], nb=1,
                                    nc=64, **keys))
    check(sisr_amd.sftmd.SFTMDHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, metadata=["blur_sigma"],
                                      **keys))


def test_unset_and_zero_leave_the_criterion_as_it_is(tmp_path):
    for v in (None, 0, 0.0):
        h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ms_ssim_loss=v)
        assert type(h.criterion) is handlers.L1Loss, v
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1)
    assert type(h.criterion) is handlers.L1Loss and h.ms_ssim_loss is None
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ssim_loss=0.1)
    assert type(h.criterion) is structural.StructuralMechanism


def test_bad_weight_raises_naming_the_key(tmp_path):
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="ms_ssim_loss"):
            handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ms_ssim_loss=bad)
    with pytest.raises(ValueError, match="ms_ssim_loss"):
        sisr_amd.basic.VDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, ms_ssim_loss=-1)
    with pytest.raises(ValueError, match="ms_ssim_weights"):
        handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=False, num_blocks=1, ms_ssim_loss=0.1,
                             ms_ssim_weights=[0.5, -0.5])


def test_eval_mode_does_not_wrap(tmp_path):
    h = handlers.EDSRHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=True, num_blocks=1, ms_ssim_loss=0.1)
    assert type(h.criterion) is handlers.L1Loss
    h = sisr_amd.basic.SRCNNHandler(device=CPU, model_save_dir=str(tmp_path), eval_mode=True, ms_ssim_loss=0.1)
    assert type(h.criterion) is sisr_amd.basic.MSELoss


# ----------------------------------------------------------------------------- entry points and operator
def test_entry_points_refuse_bad_arguments_before_any_device_call():
    """sisr_ms_ssim validates on the host and returns an error code: no launch is made, so this runs without a GPU (the
    pointers are host stand-ins that must never be dereferenced)"""
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    ERR_ARG, ERR_ALIGN = -1, -2
    wsb = L.sisr_ms_ssim_workspace_bytes
    w5 = (C.c_double * 5)(*MS.WEIGHTS)
    # refused shapes: planes <= 0, a side under 11 * 2^(levels - 1), levels outside 1 .. 8
    assert wsb(0, 176, 176, 5, 1) == 0 and wsb(-1, 176, 176, 5, 0) == 0
    assert wsb(1, 175, 176, 5, 1) == 0 and wsb(1, 176, 175, 5, 0) == 0 and wsb(1, 87, 88, 4, 0) == 0
    assert wsb(1, 10, 11, 1, 0) == 0 and wsb(1, 4000, 4000, 0, 0) == 0 and wsb(1, 4000, 4000, 9, 0) == 0
    # accepted: growing with the gradient's maps, with the planes and with the scales
    assert 0 < wsb(1, 176, 176, 5, 0) < wsb(1, 176, 176, 5, 1) < wsb(2, 176, 176, 5, 1)
    assert 0 < wsb(1, 88, 88, 4, 1) and 0 < wsb(1, 11, 11, 1, 1) < wsb(1, 22, 22, 2, 1)
    assert wsb(1, 1408, 1408, 8, 0) > 0
    # one scale, no gradient: one tile sum, 8 factors, one value, each padded to 16 bytes; with it three maps of one window
    assert wsb(1, 11, 11, 1, 0) == 16 + 64 + 16 and wsb(1, 11, 11, 1, 1) == 16 + 64 + 16 + 32
    big = 1 << 30
    f = L.sisr_ms_ssim

    def call(sr=a, y=a, planes=1, h=176, w=176, r=1.0, wts=w5, levels=5, per=a, value=a, grad=a, ws=a, nbytes=big):
        return f(sr, y, planes, h, w, r, wts, levels, per, value, grad, ws, nbytes, None)
    # null operands; neither output
    assert call(sr=None) == ERR_ARG and call(y=None) == ERR_ARG and call(wts=None) == ERR_ARG and call(ws=None) == ERR_ARG
    assert call(per=None, value=None) == ERR_ARG
    # planes <= 0, a side under the rule, levels outside 1 .. 8
    assert call(planes=0) == ERR_ARG and call(planes=-3) == ERR_ARG
    assert call(h=175) == ERR_ARG and call(w=175) == ERR_ARG and call(h=87, w=88, levels=4) == ERR_ARG
    assert call(levels=0) == ERR_ARG and call(levels=9, h=4000, w=4000) == ERR_ARG and call(levels=-1) == ERR_ARG
    # a weight that is negative or not finite, at any position
    for bad in (-0.1, float("nan"), float("inf")):
        for k in (0, 4):
            wts = list(MS.WEIGHTS)
            wts[k] = bad
            assert call(wts=(C.c_double * 5)(*wts)) == ERR_ARG, (bad, k)
    # data_range not finite or <= 0
    for r in (0.0, -1.0, float("nan"), float("inf")):
        assert call(r=r) == ERR_ARG, r
    # workspace too small: for the value alone, and for the gradient's maps
    assert call(grad=None, nbytes=wsb(1, 176, 176, 5, 0) - 1) == ERR_ARG
    assert call(nbytes=wsb(1, 176, 176, 5, 1) - 1) == ERR_ARG
    assert call(nbytes=wsb(1, 176, 176, 5, 0)) == ERR_ARG
    # misaligned pointers
    assert call(ws=a + 8) == ERR_ALIGN
    assert call(sr=a + 2) == ERR_ALIGN and call(y=a + 1) == ERR_ALIGN
    assert call(value=a + 2) == ERR_ALIGN and call(grad=a + 2) == ERR_ALIGN and call(per=a + 4) == ERR_ALIGN
    assert L.sisr_luma_clip(None, 1, 16, 16, a, None) == ERR_ARG and L.sisr_luma_clip(a, 1, 16, 16, None, None) == ERR_ARG
    assert L.sisr_luma_clip(a, 0, 16, 16, a, None) == ERR_ARG and L.sisr_luma_clip(a + 2, 1, 16, 16, a, None) == ERR_ALIGN


def test_too_many_tiles_are_refused():
    L = sisr_amd.hip.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    a += (-a) % 16
    w1 = (C.c_double * 1)(1.0)
    # 2^31 planes would not fit an int; 2^30 planes of 16 x 16 have one window tile and one pixel tile each: accepted by the
    # tile rule.  2^30 planes of 16 x 80 have two tiles each: 2^31 tiles
    planes = 1 << 30
    need = L.sisr_ms_ssim_workspace_bytes(planes, 16, 80, 1, 0)
    assert need > 0
    assert L.sisr_ms_ssim(a, a, planes, 16, 80, 1.0, w1, 1, a, a, None, a, need, None) == -4


def test_operator_has_no_cpu_path_and_names_the_minimum_side():
    x = torch.rand(1, 3, 176, 176)
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP device"):
        sisr_amd.ops.ms_ssim_mean(x, x.clone())
    for shape in ((1, 1, 175, 200), (1, 1, 200, 175)):
        t = torch.rand(shape)
        with pytest.raises(ValueError, match="at least 176.*ms_ssim_weights"):
            sisr_amd.ops.ms_ssim_mean(t, t.clone())
    t = torch.rand(1, 1, 87, 128)
    with pytest.raises(ValueError, match="at least 88"):
        sisr_amd.ops.ms_ssim_mean(t, t.clone(), weights=MS.WEIGHTS[:4])
    with pytest.raises(ValueError, match="ms_ssim_weights"):
        sisr_amd.ops.ms_ssim_mean(x, x.clone(), weights=(0.5, float("nan")))
    with pytest.raises(RuntimeError, match="one shape"):
        sisr_amd.ops.ms_ssim_mean(torch.rand(1, 3, 176, 176), torch.rand(1, 3, 176, 177))
    with pytest.raises(RuntimeError, match="one shape"):
        sisr_amd.ops.ms_ssim_mean(torch.rand(3, 176, 176), torch.rand(3, 176, 176))
