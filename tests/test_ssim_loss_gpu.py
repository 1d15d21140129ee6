"""Structural (SSIM) loss on the GPU: ops.ssim_mean against the float64 oracle with the stock torch fp32 composition as the
yardstick, the criterion, and the handlers' training steps."""
import numpy as np
import pytest
import torch

from sisr_amd import architectures as A
from sisr_amd import basic, handlers, metrics, ops, structural

import _ssim_loss as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASE_IDS = ["%dx%dx%dx%d-%g" % (s + (n,)) for s, n in S.CASES]


def _hip(sr, y, scale=1.0, data_range=1.0):
    """(value, d (scale * value) / d sr) from ops.ssim_mean"""
    sr = sr.to(DEV).requires_grad_(True)
    v = ops.ssim_mean(sr, y.to(DEV), data_range)
    (scale * v).backward()
    return v.detach(), sr.grad


@pytest.fixture(scope="module")
def runs():
    """per case, computed once and never modified: the inputs, (value, gradient) of the float64 oracle on the host, of the
    stock torch fp32 composition on the device and of the HIP operator"""
    out = {}
    for cid, (shape, noise) in zip(CASE_IDS, S.CASES):
        sr, y = S.make_pair(shape, noise)
        ref = S.autograd_grad(sr.double(), y.double())
        stock = S.autograd_grad(sr.to(DEV), y.to(DEV))
        out[cid] = (sr, y, ref, stock, _hip(sr, y))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cid", CASE_IDS)
def test_value_is_the_float64_mean_rounded_to_fp32(runs, cid):
    """|v_hip - v_64| <= 2^-24: the value is a float64 quantity rounded to fp32 once and lies in [0.5, 1) for these inputs
    (asserted on the oracle), so half a unit, 2^-25, is the rounding; the factor two leaves room for float64 summation order.
    Measured on an MI355X, |v_hip - v_64| (the stock fp32 composition's in brackets):
      2 x 3 x 11 x 11, s 0.05: 2.50e-08 (3.46e-08)      1 x 1 x 11 x 85, s 0.05: 7.98e-09 (5.16e-08)
      2 x 1 x 42 x 74, s 0.05: 1.06e-10 (1.06e-10)      1 x 3 x 43 x 75, s 0.05: 1.48e-09 (5.81e-08)
      1 x 3 x 43 x 75, s 0.002: 1.37e-09 (6.10e-08)
    all below the rounding alone, 2^-25 = 2.98e-08: the HIP value is the fp32 number nearest the float64 mean in every case."""
    sr, y, (v64, _), (v32, _), (vh, gh) = runs[cid]
    assert 0.5 <= float(v64) < 1.0, float(v64)
    assert vh.dtype == torch.float32 and vh.shape == ()
    d = abs(float(vh.double().cpu()) - float(v64))
    print(f"value {cid}: oracle {float(v64):.9f} |hip - f64| {d:.3e} (stock fp32 {abs(float(v32.double().cpu()) - float(v64)):.3e})")
    assert d <= 2.0 ** -24, d


@pytest.mark.parametrize("cid", CASE_IDS)
def test_gradient_is_no_further_from_float64_than_stock_fp32(runs, cid):
    """relative L2 of d value / d sr against float64 autograd of the oracle, no element excluded.  Bound: the error of the stock
    torch fp32 composition (grouped conv2d, same device, same inputs) against the same float64 values, taken in this run, margin
    factor 1: the kernel holds its statistics and its coefficient maps in float64, so anything above the yardstick is a defect.
    Measured on an MI355X (relative L2 against float64: HIP / stock torch fp32):
      2 x 3 x 11 x 11, s 0.05: 2.36e-08 / 2.01e-06      1 x 1 x 11 x 85, s 0.05: 2.50e-08 / 1.48e-06
      2 x 1 x 42 x 74, s 0.05: 2.49e-08 / 1.28e-06      1 x 3 x 43 x 75, s 0.05: 2.54e-08 / 1.55e-06
      1 x 3 x 43 x 75, s 0.002: 2.61e-08 / 3.74e-05
    The HIP figure is the one rounding of each element to fp32 (2^-24 / sqrt(3) relative in the mean, 3.4e-08 at most) and does
    not grow near convergence; the stock composition's grows with 1 / s."""
    sr, y, (_, g64), (_, g32), (_, gh) = runs[cid]
    assert gh.shape == sr.shape and gh.is_contiguous() and gh.dtype == torch.float32
    e, s = S.rel_l2(gh, g64), S.rel_l2(g32, g64)
    print(f"gradient {cid}: hip {e:.3e} stock {s:.3e}")
    assert e <= s, (e, s)


def test_upstream_gradient_scales_the_result(runs):
    """(3 * ssim_mean).backward(): against float64 autograd of 3 * oracle under the same rule
    Measured on an MI355X (HIP / stock torch fp32): 3.73e-08 / 1.51e-06; the HIP gradient is the unit one times 3, bit for bit."""
    cid = CASE_IDS[-2]
    sr, y, _, _, (_, g1) = runs[cid]
    _, g64 = S.autograd_grad(sr.double(), y.double(), scale=3.0)
    _, g32 = S.autograd_grad(sr.to(DEV), y.to(DEV), scale=3.0)
    _, gh = _hip(sr, y, scale=3.0)
    e, s = S.rel_l2(gh, g64), S.rel_l2(g32, g64)
    print(f"gradient of 3 * ssim_mean {cid}: hip {e:.3e} stock {s:.3e}")
    assert e <= s, (e, s)
    assert torch.equal(gh, g1 * 3.0)


@pytest.mark.parametrize("shape", S.SHAPES)
def test_equal_images_give_exactly_one(shape):
    _, y = S.make_pair(shape, 0.0)
    v, g = _hip(y.clone(), y)
    assert float(v) == 1.0
    # the maximum of S: the three terms of the gradient, O(1 / B2) <= 1 / C2 ~ 1e3 each, cancel in float64
    assert float(g.abs().max()) <= 1e-9


def test_a_repeat_call_is_bit_identical(runs):
    for cid in CASE_IDS[-2:]:
        sr, y, _, _, (v1, g1) = runs[cid]
        ops.l1_loss(torch.rand(1 << 18, device=DEV), torch.rand(1 << 18, device=DEV))  # something else uses the workspace
        v2, g2 = _hip(sr, y)
        assert torch.equal(v1, v2) and torch.equal(g1, g2)


def test_value_without_a_gradient_is_the_same_value(runs):
    sr, y, _, _, (v1, _) = runs[CASE_IDS[-1]]
    with torch.no_grad():
        v = ops.ssim_mean(sr.to(DEV), y.to(DEV))
    assert not v.requires_grad and torch.equal(v, v1)
    # a non-contiguous operand is compared as the batch it shows
    wide = torch.zeros(sr.shape[:3] + (sr.shape[3] + 3,), device=DEV)
    wide[..., :sr.shape[3]] = sr.to(DEV)
    assert torch.equal(ops.ssim_mean(wide[..., :sr.shape[3]], y.to(DEV)), v1)


def test_target_takes_no_gradient():
    x = torch.rand(1, 1, 16, 16, device=DEV)
    with pytest.raises(RuntimeError, match="target takes no gradient"):
        ops.ssim_mean(x, x.clone().requires_grad_(True))


@pytest.mark.parametrize("shape", [(2, 1, 43, 75), (3, 1, 42, 74)])
def test_agrees_with_the_metric_kernel(shape):
    """C = 1 planes in [0, 1]: ssim_mean and the mean over images of metrics.batch_ssim (the float64 metric kernel) differ by at
    most 2^-24 (every image has the same number of windows, so the mean of the per-image means is the mean over all windows).
    Measured on an MI355X: 1.97e-08 at 2 x 1 x 43 x 75, 1.79e-09 at 3 x 1 x 42 x 74."""
    sr, y = S.make_pair(shape, 0.05)
    sr = sr.clamp(0, 1)
    per_image = metrics.batch_ssim(sr.to(DEV), y.to(DEV))
    assert len(per_image) == shape[0]
    with torch.no_grad():
        v = ops.ssim_mean(sr.to(DEV), y.to(DEV))
    d = abs(float(v.double().cpu()) - float(np.mean(per_image, dtype=np.float64)))
    print(f"metric agreement {shape}: {d:.3e}")
    assert d <= 2.0 ** -24, d


# ----------------------------------------------------------------------------- criterion
def test_criterion_matches_float64_within_four_times_stock_fp32():
    """StructuralMechanism(L1Loss(), 0.2) on inputs with |sr - y| >= 0.01 (the L1 kink rule): loss and d loss / d sr against the
    float64 restatement, relative error no larger than 4 x that of the stock torch fp32 composition on the same device -- the L1
    mean's fp32 rounding is shared with the yardstick, and 4 is what the perceptual criterion's test allows for the same reason.
    Measured on an MI355X (HIP / stock torch fp32): loss 2.48e-07 / 1.10e-07, d loss / d sr 3.44e-08 / 2.09e-07.  The loss is
    passed at 2.3 x the stock error, under the 4: an fp32 unit of this loss (0.0313) is 1.19e-07 relative, and the HIP value
    carries the plain l1_loss's fp32 sum times a rounded 1 / n (up to 1.5 units) and the one rounding of the SSIM mean to fp32
    (up to 2^-25 of a value of 0.9936, times 0.2: up to 1.6 units of the loss).  As the HIP figure is fixed, a run in which the stock loss came out
    below 6.2e-08 from float64 would fail it without anything being wrong."""
    shape = (2, 3, 43, 75)
    sr, y = S.kink_free_pair(shape)
    assert float((sr - y).abs().min()) >= 0.01
    crit = structural.StructuralMechanism(handlers.L1Loss(), 0.2)

    def run(fn, sr, y):
        sr = sr.clone().requires_grad_(True)
        loss = fn(sr, y)
        (g,) = torch.autograd.grad(loss, sr)
        return loss.detach(), g

    l64, g64 = run(lambda a, b: S.criterion(a, b, "l1", 0.2), sr.double(), y.double())
    l32, g32 = run(lambda a, b: S.criterion(a, b, "l1", 0.2), sr.to(DEV), y.to(DEV))
    lh, gh = run(crit, sr.to(DEV), y.to(DEV))
    assert gh.shape == sr.shape and gh.is_contiguous()
    e_l, e_g = S.rel_l2(lh, l64), S.rel_l2(gh, g64)
    s_l, s_g = S.rel_l2(l32, l64), S.rel_l2(g32, g64)
    print(f"criterion: loss hip {e_l:.3e} stock {s_l:.3e}; gradient hip {e_g:.3e} stock {s_g:.3e}")
    assert float(l64) > float((sr.double() - y.double()).abs().mean())  # the structural term is in it
    assert e_g <= 4 * s_g, (e_g, s_g)
    assert e_l <= 4 * s_l, (e_l, s_l)


# ----------------------------------------------------------------------------- handlers
class _SmallRCANHandler(handlers.BaseModel):
    """RCANHandler around a reduced RCAN: one group, one block, 64 features, x4"""

    def __init__(self, device, model_save_dir, eval_mode=False, lr=1e-4, perceptual=None, **kwargs):
        super().__init__(device=device, model_save_dir=model_save_dir, eval_mode=eval_mode, **kwargs)
        self.net = A.RCAN(n_resblocks=1, n_resgroups=1, n_feats=64, scale=4)
        self.colorspace = 'rgb'
        self.im_input = 'unmodified'
        self.activate_device()
        self.training_setup(lr, None, None, perceptual, device)
        self.model_name = 'rcan'


def _float64_criterion(out, y, base, alpha):
    return float(S.criterion(out.detach().double().cpu(), y.detach().double().cpu(), base, alpha))


def test_handler_trains_with_the_structural_loss_eager_and_graphed(tmp_path):
    """three train_steps at B = 2, 16 x 16 LR -> 64 x 64, ssim_loss = 0.2, eager and replayed from a hipGraph: the same loss
    trajectory and final parameters (tolerances of the perceptual handler test: 1e-6 absolute per loss, 1e-5 on the parameter
    sum); the first loss is the float64 criterion of the returned output within 1e-5 relative and exceeds its L1 term; run_eval
    reports the combined loss."""
    runs = {}
    for mode in (False, True):
        torch.manual_seed(8)
        h = _SmallRCANHandler(device=0, model_save_dir=str(tmp_path), ssim_loss=0.2)
        h.use_graph = mode
        assert isinstance(h.criterion, structural.StructuralMechanism) and type(h.criterion.base) is handlers.L1Loss
        g = torch.Generator().manual_seed(5)
        ls, first = [], None
        for step in range(3):
            x, y = torch.rand(2, 3, 16, 16, generator=g), torch.rand(2, 3, 64, 64, generator=g)
            loss, out = h.train_step(x, y)
            if step == 0:
                first = (float(loss), _float64_criterion(out, y, "l1", 0.2), float((out.double().cpu() - y.double()).abs().mean()))
            ls.append(float(loss))
        torch.cuda.synchronize()
        print(f"rcan graph={mode}: losses {ls} first {first}")
        assert abs(first[0] - first[1]) <= 1e-5 * abs(first[1]), first
        assert first[0] > first[2], first  # above its L1 term
        state = h.save_model("m", 0, extract_state_only=True)
        assert set(state["network"]) == set(h.net.state_dict())
        runs[mode] = (ls, float(sum(p.double().sum() for p in h.net.parameters())))
        if mode:
            x, y = torch.rand(2, 3, 16, 16, generator=g), torch.rand(2, 3, 64, 64, generator=g)
            out, eval_loss, _ = h.run_eval(x, y, request_loss=True, keep_on_device=True)
            ref = _float64_criterion(out, y, "l1", 0.2)
            assert abs(float(eval_loss) - ref) <= 1e-5 * abs(ref)
            assert float(eval_loss) > float((out.double().cpu() - y.double()).abs().mean())
    assert np.allclose(runs[True][0], runs[False][0], rtol=0, atol=1e-6), runs
    assert abs(runs[True][1] - runs[False][1]) < 1e-5


def test_y_channel_handler_trains_on_mse_plus_the_structural_term(tmp_path):
    """VDSRHandler (reduced: four 3 x 3 layers), one step at B = 2, 1 x 32 x 32: the loss is the float64 MSE + alpha (1 - SSIM) of
    the returned output within 1e-5 relative, above its MSE term, and the parameters move."""
    torch.manual_seed(8)
    h = basic.VDSRHandler(device=0, model_save_dir=str(tmp_path), kernel_pattern=[3] * 4, channel_pattern=[1, 64, 64, 64, 1],
                          ssim_loss=0.2)
    assert isinstance(h.criterion, structural.StructuralMechanism) and type(h.criterion.base) is basic.MSELoss
    start = float(sum(p.double().abs().sum() for p in h.net.parameters()))
    g = torch.Generator().manual_seed(6)
    y = torch.rand(2, 1, 32, 32, generator=g)
    x = (y + 0.05 * torch.randn(2, 1, 32, 32, generator=g)).clamp(0, 1)
    loss, out = h.train_step(x, y)
    ref = _float64_criterion(out, y, "mse", 0.2)
    mse = float(((out.double().cpu() - y.double()) ** 2).mean())
    print(f"vdsr: loss {float(loss):.8f} float64 {ref:.8f} mse term {mse:.8f}")
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (float(loss), ref)
    assert float(loss) > mse
    assert float(sum(p.double().abs().sum() for p in h.net.parameters())) != start
