"""Frequency-domain (FFT L1) loss on the GPU: ops.spectral_l1 against the float64 oracle with the same function in fp32 over
the same tables (torch.matmul on the device) as the yardstick, the table kernel and its cache, the criterion, and the
handlers' training steps."""
import numpy as np
import pytest
import torch

from sisr_amd import architectures as A
from sisr_amd import basic, frequency, handlers, hip, ops, ops_losses, structural

import _freq_loss as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CASE_IDS = ["%dx%dx%dx%d-%g" % (s + (n,)) for s, n in S.CASES]


def _hip(sr, y, scale=1.0):
    """(value, d (scale * value) / d sr) from ops.spectral_l1"""
    sr = sr.to(DEV).requires_grad_(True)
    v = ops.spectral_l1(sr, y.to(DEV))
    (scale * v).backward()
    return v.detach(), sr.grad


@pytest.fixture(scope="module")
def runs():
    """per case, computed once and never modified: the inputs, (value, gradient) of the float64 oracle on the host, of the
    fp32 table form in stock torch on the device and of the HIP operator"""
    out = {}
    for cid, (shape, noise) in zip(CASE_IDS, S.CASES):
        sr, y, margin = S.make_pair(shape, noise)
        assert margin >= S.KINK * noise
        ref = S.autograd_grad(sr.double(), y.double())
        stock = S.autograd_grad(sr.to(DEV), y.to(DEV))
        out[cid] = (sr, y, ref, stock, _hip(sr, y))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("cid", CASE_IDS)
def test_value_is_within_four_times_the_stock_fp32_error(runs, cid):
    """|v_hip - v_64| <= max(4 |v_stock - v_64|, 2^-23 v_64): the margin of 4 is the one the criterion tests of the perceptual
    and structural terms allow a stock fp32 yardstick; the floor is there because an fp32 result rounded once cannot be held
    tighter than about a unit, and the yardstick can land arbitrarily close by luck.
    Measured on an MI355X, |v_hip - v_64| / v_64 (the stock fp32 table form's in brackets):
      2 x 3 x 2 x 2: 2.05e-08 (4.09e-08)       2 x 3 x 8 x 8: 3.24e-08 (3.15e-08)       1 x 1 x 11 x 85: 2.72e-08 (9.23e-08)
      2 x 1 x 32 x 64: 2.95e-08 (2.95e-08)     1 x 1 x 33 x 65: 1.32e-08 (5.28e-08)     1 x 3 x 43 x 75: 1.90e-08 (8.47e-08)
      1 x 1 x 65 x 63: 3.86e-09 (3.86e-09)     1 x 2 x 66 x 34: 1.06e-08 (1.06e-08)     1 x 1 x 128 x 128: 1.21e-08 (5.35e-08)
      1 x 3 x 43 x 75, s 0.002: 5.34e-09 (5.34e-09)
    all below half an fp32 unit (5.96e-08 relative at most): the HIP value is the fp32 number nearest the float64 mean in every
    case, so the floor is never what passes it by more than the rounding."""
    sr, y, (v64, _), (v32, _), (vh, _) = runs[cid]
    assert vh.dtype == torch.float32 and vh.shape == ()
    v64 = float(v64)
    d, s = abs(float(vh.double().cpu()) - v64), abs(float(v32.double().cpu()) - v64)
    print(f"value {cid}: oracle {v64:.9e} |hip - f64| {d:.3e} ({d / v64:.2e} rel) stock fp32 {s:.3e} ({s / v64:.2e} rel)")
    assert d <= max(4 * s, 2.0 ** -23 * v64), (d, s, v64)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_gradient_is_within_four_times_the_stock_fp32_error(runs, cid):
    """relative L2 of d value / d sr against float64 autograd of the oracle, no element excluded, <= 4 x the yardstick's in the
    same run: both are fp32 two-stage products over identical tables, and a real defect (a flipped sign, a dropped edge
    column) shows at >= 1e-3 against ~1e-7 expected.
    Measured on an MI355X (relative L2 against float64: HIP / stock fp32 table form):
      2 x 3 x 2 x 2: 2.98e-08 / 2.98e-08       2 x 3 x 8 x 8: 6.12e-08 / 9.16e-08       1 x 1 x 11 x 85: 1.39e-07 / 1.55e-07
      2 x 1 x 32 x 64: 1.41e-07 / 1.56e-07     1 x 1 x 33 x 65: 1.58e-07 / 1.73e-07     1 x 3 x 43 x 75: 1.72e-07 / 1.74e-07
      1 x 1 x 65 x 63: 1.85e-07 / 1.92e-07     1 x 2 x 66 x 34: 1.64e-07 / 1.60e-07     1 x 1 x 128 x 128: 2.44e-07 / 2.38e-07
      1 x 3 x 43 x 75, s 0.002: 1.72e-07 / 1.74e-07
    The gradient is a sign pattern through two fp32 products: its error does not depend on the noise level, and grows like the
    square root of the chain length in both forms."""
    sr, y, (_, g64), (_, g32), (_, gh) = runs[cid]
    assert gh.shape == sr.shape and gh.is_contiguous() and gh.dtype == torch.float32
    e, s = S.rel_l2(gh, g64), S.rel_l2(g32, g64)
    print(f"gradient {cid}: hip {e:.3e} stock {s:.3e}")
    assert e <= 4 * s, (e, s)


def test_upstream_gradient_scales_the_result_bit_for_bit(runs):
    cid = CASE_IDS[5]
    sr, y, _, _, (_, g1) = runs[cid]
    _, g3 = _hip(sr, y, scale=3.0)
    assert torch.equal(g3, g1 * 3.0)


@pytest.mark.parametrize("shape", S.SHAPES)
def test_equal_images_give_exactly_zero(shape):
    _, y, _ = S.make_pair(shape, 0.05)
    v, g = _hip(y.clone(), y)
    assert float(v) == 0.0
    assert float(g.abs().max()) == 0.0


def test_a_repeat_call_is_bit_identical(runs):
    for cid in (CASE_IDS[5], CASE_IDS[8]):
        sr, y, _, _, (v1, g1) = runs[cid]
        ops.l1_loss(torch.rand(1 << 18, device=DEV), torch.rand(1 << 18, device=DEV))  # something else uses the workspace
        v2, g2 = _hip(sr, y)
        assert torch.equal(v1, v2) and torch.equal(g1, g2)


def test_value_without_a_gradient_is_the_same_value(runs):
    for cid in (CASE_IDS[5], CASE_IDS[8]):
        sr, y, _, _, (v1, _) = runs[cid]
        with torch.no_grad():
            v = ops.spectral_l1(sr.to(DEV), y.to(DEV))
        assert not v.requires_grad and torch.equal(v, v1)
    # a non-contiguous operand is compared as the batch it shows
    wide = torch.zeros(sr.shape[:3] + (sr.shape[3] + 3,), device=DEV)
    wide[..., :sr.shape[3]] = sr.to(DEV)
    assert not wide[..., :sr.shape[3]].is_contiguous()
    assert torch.equal(ops.spectral_l1(wide[..., :sr.shape[3]], y.to(DEV)), v1)


def test_target_takes_no_gradient():
    x = torch.rand(1, 1, 16, 16, device=DEV)
    with pytest.raises(RuntimeError, match="target takes no gradient"):
        ops.spectral_l1(x, x.clone().requires_grad_(True))


# ----------------------------------------------------------------------------- tables
def _split(t, H, W):
    wh = W // 2 + 1
    ch, sh, cw, sw = torch.split(t.cpu(), [H * H, H * H, wh * W, wh * W])
    return ch.view(H, H), sh.view(H, H), cw.view(wh, W), sw.view(wh, W)


def _within_one_unit(got, want):
    """|got - want| <= one fp32 unit of want (the spacing of fp32 numbers at |want|)"""
    unit = torch.ldexp(torch.ones_like(want), torch.frexp(want).exponent - 24)
    return bool(((got - want).abs() <= unit).all())


@pytest.mark.parametrize("n", [2, 8, 75, 128])
def test_device_tables_are_the_helper_tables(n):
    """the table kernel (sincospi of the reduced fraction in float64, rounded once) against the helper's fp32 tables: within
    one fp32 unit everywhere, equal at quarter turns; H = n with W = n + 1 and the reverse, so both table pairs see n"""
    for H, W in ((n, n + 1), (n + 1, n)):
        t = ops.spectral_tables(DEV, H, W)
        assert t.numel() * 4 == hip.lib().sisr_freq_loss_table_bytes(H, W)
        got = _split(t, H, W)
        want = S.tables(H, H, torch.float32) + S.tables(W, W // 2 + 1, torch.float32)
        for g, w_, N, name in zip(got, want, (H, H, W, W), ("Ch", "Sh", "Cw", "Sw")):
            assert _within_one_unit(g, w_), (H, W, name, float((g - w_).abs().max()))
            k = torch.arange(g.shape[0])[:, None] * torch.arange(g.shape[1])[None, :]
            quarter = (4 * (k % N)) % N == 0
            assert torch.equal(g[quarter], w_[quarter]), (H, W, name)
            assert bool(quarter.any())


def test_a_table_miss_during_capture_raises_and_a_hit_does_not():
    shape = (1, 1, 12, 20)
    a, b = torch.rand(shape, device=DEV), torch.rand(shape, device=DEV)
    ops_losses._spectral_tables.get(DEV.index, {}).pop((12, 20), None)
    ops_losses._spectral_held.get(DEV.index, {}).pop((12, 20), None)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        c = a + b  # the graph is not empty
        with pytest.raises(RuntimeError, match="not cached.*capturing"):  # raised on the host, before any launch
            ops.spectral_l1(a, b)
    del c, graph
    with torch.no_grad():
        want = ops.spectral_l1(a, b)  # eager: builds the tables
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        got = ops.spectral_l1(a, b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert (12, 20) in ops_losses._spectral_held[DEV.index]  # a captured graph reads them: out of the LRU list for good


def test_nine_shapes_in_a_row_evict_and_stay_correct():
    shapes = [(1, 1, 6 + k, 9 + 2 * k) for k in range(9)]
    pairs = [(torch.rand(s, generator=torch.Generator().manual_seed(k)), torch.rand(s, generator=torch.Generator().manual_seed(50 + k)))
             for k, s in enumerate(shapes)]
    want = [float(S.spectral_l1(a.double(), b.double())) for a, b in pairs]
    for rnd in range(2):  # the second round finds the first shapes evicted and builds them again
        for (a, b), w_ in zip(pairs, want):
            with torch.no_grad():
                v = float(ops.spectral_l1(a.to(DEV), b.to(DEV)))
            assert abs(v - w_) <= 1e-6 * w_, (a.shape, v, w_)
        cache = ops_losses._spectral_tables[DEV.index]
        assert len(cache) <= ops.SPECTRAL_TABLE_SLOTS
        assert tuple(shapes[0][2:]) not in cache and tuple(shapes[-1][2:]) in cache


# ----------------------------------------------------------------------------- criterion
def test_criterion_matches_float64_within_four_times_stock_fp32():
    """FrequencyMechanism(StructuralMechanism(L1Loss(), 0.2), 0.1) on an input that is kink-free for L1 (|sr - y| >= 0.01) and
    for the spectrum: loss and d loss / d sr against the float64 restatement, relative error no larger than 4 x that of the
    stock torch fp32 composition on the same device.
    Measured on an MI355X (HIP / stock torch fp32): loss 3.11e-08 / 3.11e-08 (the same fp32 number), d loss / d sr
    3.93e-08 / 1.97e-07."""
    shape = (2, 3, 43, 75)
    sr, y = S.kink_free_pair(shape)
    assert float((sr - y).abs().min()) >= 0.01 and S.kink_margin(sr, y) >= 1e-6
    crit = frequency.FrequencyMechanism(structural.StructuralMechanism(handlers.L1Loss(), 0.2), 0.1)

    def run(fn, sr, y):
        sr = sr.clone().requires_grad_(True)
        loss = fn(sr, y)
        (g,) = torch.autograd.grad(loss, sr)
        return loss.detach(), g

    l64, g64 = run(lambda a, b: S.criterion(a, b, "l1", 0.2, 0.1), sr.double(), y.double())
    l32, g32 = run(lambda a, b: S.criterion(a, b, "l1", 0.2, 0.1), sr.to(DEV), y.to(DEV))
    lh, gh = run(crit, sr.to(DEV), y.to(DEV))
    assert gh.shape == sr.shape and gh.is_contiguous()
    e_l, e_g = S.rel_l2(lh, l64), S.rel_l2(gh, g64)
    s_l, s_g = S.rel_l2(l32, l64), S.rel_l2(g32, g64)
    print(f"criterion: loss hip {e_l:.3e} stock {s_l:.3e}; gradient hip {e_g:.3e} stock {s_g:.3e}")
    assert float(l64) > float(S.criterion(sr.double(), y.double(), "l1", 0.2, 0.0))  # the spectral term is in it
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


def _float64_criterion(out, y, base, alpha, beta):
    return float(S.criterion(out.detach().double().cpu(), y.detach().double().cpu(), base, alpha, beta))


def test_handler_trains_with_the_frequency_loss_eager_and_graphed(tmp_path, monkeypatch):
    """three train_steps at B = 2, 16 x 16 LR -> 64 x 64, freq_loss = 0.1, eager and replayed from a hipGraph: the same loss
    trajectory and final parameters (tolerances of the structural handler test: 1e-6 absolute per loss, 1e-5 on the parameter
    sum); the first loss is the float64 criterion of the returned output within 1e-5 relative and exceeds its L1 term; the
    capture never misses the table cache (a miss raises); run_eval reports the combined loss."""
    runs = {}
    for mode in (False, True):
        torch.manual_seed(8)
        h = _SmallRCANHandler(device=0, model_save_dir=str(tmp_path), freq_loss=0.1)
        h.use_graph = mode
        assert isinstance(h.criterion, frequency.FrequencyMechanism) and type(h.criterion.base) is handlers.L1Loss
        if mode:  # the graphed step must find the tables through its own eager warm-up pass, not through earlier tests
            ops_losses._spectral_tables.get(0, {}).pop((64, 64), None)
            ops_losses._spectral_held.get(0, {}).pop((64, 64), None)
        g = torch.Generator().manual_seed(5)
        ls, first = [], None
        for step in range(3):
            x, y = torch.rand(2, 3, 16, 16, generator=g), torch.rand(2, 3, 64, 64, generator=g)
            loss, out = h.train_step(x, y)
            if step == 0:
                first = (float(loss), _float64_criterion(out, y, "l1", 0.0, 0.1), float((out.double().cpu() - y.double()).abs().mean()))
            ls.append(float(loss))
        torch.cuda.synchronize()
        print(f"rcan graph={mode}: losses {ls} first {first}")
        assert abs(first[0] - first[1]) <= 1e-5 * abs(first[1]), first
        assert first[0] > first[2], first  # above its L1 term
        state = h.save_model("m", 0, extract_state_only=True)
        assert set(state["network"]) == set(h.net.state_dict())
        runs[mode] = (ls, float(sum(p.detach().double().sum() for p in h.net.parameters())))
        if mode:
            assert (64, 64) in ops_losses._spectral_held[0]
            x, y = torch.rand(2, 3, 16, 16, generator=g), torch.rand(2, 3, 64, 64, generator=g)
            out, eval_loss, _ = h.run_eval(x, y, request_loss=True, keep_on_device=True)
            ref = _float64_criterion(out, y, "l1", 0.0, 0.1)
            assert abs(float(eval_loss) - ref) <= 1e-5 * abs(ref)
            assert float(eval_loss) > float((out.double().cpu() - y.double()).abs().mean())
    assert np.allclose(runs[True][0], runs[False][0], rtol=0, atol=1e-6), runs
    assert abs(runs[True][1] - runs[False][1]) < 1e-5


def test_y_channel_handler_trains_on_mse_plus_the_frequency_term(tmp_path):
    """VDSRHandler (reduced: four 3 x 3 layers), one step at B = 2, 1 x 32 x 32: the loss is the float64 MSE + beta * spectral L1
    of the returned output within 1e-5 relative, above its MSE term, and the parameters move."""
    torch.manual_seed(8)
    h = basic.VDSRHandler(device=0, model_save_dir=str(tmp_path), kernel_pattern=[3] * 4, channel_pattern=[1, 64, 64, 64, 1],
                          freq_loss=0.1)
    assert isinstance(h.criterion, frequency.FrequencyMechanism) and type(h.criterion.base) is basic.MSELoss
    start = float(sum(p.detach().double().abs().sum() for p in h.net.parameters()))
    g = torch.Generator().manual_seed(6)
    y = torch.rand(2, 1, 32, 32, generator=g)
    x = (y + 0.05 * torch.randn(2, 1, 32, 32, generator=g)).clamp(0, 1)
    loss, out = h.train_step(x, y)
    ref = _float64_criterion(out, y, "mse", 0.0, 0.1)
    mse = float(((out.double().cpu() - y.double()) ** 2).mean())
    print(f"vdsr: loss {float(loss):.8f} float64 {ref:.8f} mse term {mse:.8f}")
    assert abs(float(loss) - ref) <= 1e-5 * abs(ref), (float(loss), ref)
    assert float(loss) > mse
    assert float(sum(p.detach().double().abs().sum() for p in h.net.parameters())) != start
