"""Stride-2 K x K conv on the HIP kernels (pytest -m gpu).

Kernel level: forward, input gradient (the polyphase transposed conv) and weight / bias gradient against torch's float64
`F.conv2d(stride=2)` and its autograd on the exact data of tests/_exact.py: after `assert_budget` every comparison is exact.
Model level: IKC's predictor (one stride-2 layer) against its float64 twin with the bound and the kink protocol of
tests/test_predictor_gpu.py."""
import pytest
import torch
import torch.nn.functional as F

import _basic as R
import _exact as E
import _predictor as P
import _stride2 as S
import sisr_amd

pytestmark = pytest.mark.gpu
ops = sisr_amd.ops
DEV = "cuda:0"
CL = torch.channels_last


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _f64(t):
    return t.detach().double().requires_grad_(True)


# ----------------------------------------------------------------------------- 1. forward and the three gradients, exact
@pytest.mark.parametrize("hw", S.SIZES)
@pytest.mark.parametrize("K", [1, 3, 5])
@pytest.mark.parametrize("cin, cout", S.WIDTHS)
@pytest.mark.parametrize("slope", [0.25, 0.5, None])  # None: no activation (act off)
def test_stride2_forward_and_gradients_exact(hw, K, cin, cout, slope):
    H, W = hw
    Ho, Wo = S.out_size(H), S.out_size(W)
    cip, cop = R.pad_width(cin), R.pad_width(cout)
    x, w = E.ints((R.B, cin, H, W), 141, zeros=0.25), E.weights((cout, cin, K, K), 142)
    b = E.biases(cout, 143)
    cot = E.ints((R.B, cop, Ho, Wo), 144)  # a cotangent on the padded channels too: it must not reach any gradient
    E.conv_budget(x.to(DEV), w.to(DEV), extras=(b,), padding=K // 2, what="stride-2 kxk")  # (stride-1 outputs: a superset)
    xl, wl, bl = R.to_map(x, cip, DEV).requires_grad_(True), _leaf(w), _leaf(b)
    y = ops.conv_kxk(xl, wl, bl, slope=slope, stride=2)
    assert y.shape == (R.B, cop, Ho, Wo) and y.is_contiguous(memory_format=CL)
    x64, w64, b64 = _f64(x), _f64(w), _f64(b)
    pre = S.conv_s2(x64, w64, b64)
    ref = pre if slope is None else F.leaky_relu(pre, slope)
    E.assert_exact(y[:, :cout], ref.detach(), "stride-2 kxk output")  # slope * v is exact: v is on the 1/8 grid
    assert not y[:, cout:].any(), "padded channels must be written as zero"
    S.assert_gradient_budgets(x, w, cot[:, :cout], slope, "stride-2 kxk")
    y.backward(cot.to(DEV))
    ref.backward(cot[:, :cout].double())
    E.assert_exact(xl.grad[:, :cin], x64.grad, "stride-2 kxk dx")
    assert xl.grad.shape == (R.B, cip, H, W) and not xl.grad[:, cin:].any(), "padded input channels take no gradient"
    E.assert_exact(wl.grad, w64.grad, "stride-2 kxk dw")
    E.assert_exact(bl.grad, b64.grad, "stride-2 kxk db")
    first = (wl.grad.clone(), xl.grad.clone(), bl.grad.clone())
    wl.grad = xl.grad = bl.grad = None
    ops.conv_kxk(xl, wl, bl, slope=slope, stride=2).backward(cot.to(DEV))
    assert torch.equal(first[0], wl.grad) and torch.equal(first[1], xl.grad) and torch.equal(first[2], bl.grad), \
        "gradients must be bit-identical run to run"


@pytest.mark.parametrize("K", [7, 9])
def test_stride2_largest_kernels_run_within_the_lds_of_a_cu(K):
    """K = 9 asks for 152 KB of the 160 KB a workgroup can have: it launches and is exact (both widths of the output)"""
    H, W = 17, 65
    x = E.ints((R.B, 64, H, W), 145, zeros=0.5)
    for cout in (64, 32):
        w = E.weights((cout, 64, K, K), 146, kmax=2)
        E.conv_budget(x.to(DEV), w.to(DEV), padding=K // 2, what="stride-2 kxk")
        xl, wl = R.to_map(x, 64, DEV).requires_grad_(True), _leaf(w)
        y = ops.conv_kxk(xl, wl, None, slope=0.5, stride=2)
        x64, w64 = _f64(x), _f64(w)
        ref = F.leaky_relu(S.conv_s2(x64, w64), 0.5)
        E.assert_exact(y, ref.detach(), "stride-2 %d x %d output" % (K, K))
        cot = E.ints(tuple(y.shape), 147, -1, 1)
        S.assert_gradient_budgets(x, w, cot, 0.5, "stride-2 %d x %d" % (K, K))
        y.backward(cot.to(DEV))
        ref.backward(cot.double())
        E.assert_exact(xl.grad, x64.grad, "dx")
        E.assert_exact(wl.grad, w64.grad, "dw")


# ----------------------------------------------------------------------------- 2. the gradient kernels read the MASK map
@pytest.mark.parametrize("hw", [(9, 21), (16, 64), (37, 70)])
@pytest.mark.parametrize("slope", [0.25, 0.5])
def test_stride2_dgrad_and_wgrad_read_the_mask_map_not_the_sign_of_dy(hw, slope):
    """raw entry points with a mask map unrelated to the output: dy_eff = m > 0 ? dy : slope * dy with m drawn on its own"""
    H, W = hw
    Ho, Wo = S.out_size(H), S.out_size(W)
    K, cin, cout, cip, cop = 5, 64, 32, 64, 32
    hip, L = sisr_amd.hip, sisr_amd.hip.lib()
    x, w = E.ints((R.B, cin, H, W), 161), E.weights((cout, cin, K, K), 162)
    dy, m = E.ints((R.B, cout, Ho, Wo), 163), E.ints((R.B, cout, Ho, Wo), 164, -1, 1)
    eff = dy.double() * E.leaky_mask(m, slope)
    assert torch.equal(eff, torch.where(m > 0, dy.double(), slope * dy.double()))
    assert ((dy > 0) & (m <= 0)).any() and ((dy < 0) & (m > 0)).any(), "test bug: sign of dy and mask never disagree"
    S.assert_gradient_budgets(x, w, dy, slope, "stride-2 leaky")
    x64, w64, b64 = _f64(x), _f64(w), torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    S.conv_s2(x64, w64, b64).backward(eff)
    xm, dym, mm = R.to_map(x, cip, DEV), R.to_map(dy, cop, DEV), R.to_map(m, cop, DEV)
    _, pd = ops.pack_convk(w.to(DEV), need_dgrad=True)
    dx = torch.full((R.B, cip, H, W), float("nan"), device=DEV).contiguous(memory_format=CL)
    hip.check(L.sisr_dgradk_s2_mfma_leaky(hip.ptr(dym), hip.ptr(mm), hip.ptr(pd), hip.ptr(dx), R.B, H, W, K, cop, cip, slope,
                                          hip.stream()), "sisr_dgradk_s2_mfma_leaky")
    E.assert_exact(dx, x64.grad, "stride-2 dgrad through a foreign mask")
    dw, db = torch.full_like(w, float("nan")).to(DEV), torch.full((cout,), float("nan"), device=DEV)
    nb = L.sisr_wgradk_s2_mfma_workspace_bytes(R.B, H, W, K, cip, cop)
    ws = hip.workspace(torch.device(DEV), nb)
    hip.check(L.sisr_wgradk_s2_mfma_leaky(hip.ptr(xm), hip.ptr(dym), hip.ptr(mm), hip.ptr(dw), hip.ptr(db), R.B, H, W, K, cout,
                                          cin, cop, cip, hip.ptr(ws), nb, slope, hip.stream()), "sisr_wgradk_s2_mfma_leaky")
    E.assert_exact(dw, w64.grad, "stride-2 wgrad through a foreign mask")
    E.assert_exact(db, b64.grad, "stride-2 bias gradient through a foreign mask")


# ----------------------------------------------------------------------------- 3. stride=1 is the path it was
def test_conv_kxk_with_stride_1_is_bit_identical_to_a_call_without_the_argument():
    g = torch.Generator().manual_seed(171)
    x, w, b = torch.randn((R.B, 64, 37, 70), generator=g), torch.randn((48, 64, 5, 5), generator=g) * 0.05, torch.randn(48, generator=g)
    cot = torch.randn((R.B, 64, 37, 70), generator=g).contiguous(memory_format=CL).to(DEV)
    got = []
    for kwargs in ({}, {"stride": 1}):
        xl, wl, bl = R.to_map(x, 64, DEV).requires_grad_(True), _leaf(w), _leaf(b)
        y = ops.conv_kxk(xl, wl, bl, slope=0.2, **kwargs)
        y.backward(cot)
        got.append((y.detach(), xl.grad, wl.grad, bl.grad))
    for a, c in zip(*got):
        assert torch.equal(a, c)


# ----------------------------------------------------------------------------- 4. IKC's predictor against its float64 twin
@pytest.mark.parametrize("M", [1, 12])
@pytest.mark.parametrize("num_features", [64, 48])
def test_ikc_predictor_output_and_gradients_against_the_float64_twin(M, num_features):
    """DegradationPredictor(strides=[1, 1, 1, 2, 1, 1]) on (2, 3, 37, 70): relative L2 distance of the output and of every
    parameter gradient from float64 < 5e-5, with the kink protocol of test_predictor_gpu.py (inside |z64| < KINK the
    reference takes the branch the HIP forward took; at most two elements of a case are decided that way)."""
    shape = (2, 3, 37, 70)
    cfg = dict(num_outputs=M, num_features=num_features, num_layers=6, strides=S.IKC_STRIDES)
    net = sisr_amd.predictor.DegradationPredictor(**cfg)
    sd = P.kaiming_state(net, 170 + M + num_features)
    net.load_state_dict(sd, strict=True)
    net.to(DEV)
    g = torch.Generator().manual_seed(172)
    x, cot = torch.rand(shape, generator=g), torch.randn((shape[0], M), generator=g)
    out = net(x.to(DEV))
    assert out.shape == (shape[0], M)
    out.backward(cot.to(DEV))
    with torch.no_grad():  # the branch every LeakyReLU of the HIP forward took: the same launches again, layer by layer
        t, branches = ops.nchw_to_nhwc_pad(x.to(DEV), cp=32), []
        for i in range(6):
            m = net.layer_dict["conv_%d" % i]
            t = ops.conv_kxk(t, m.weight, m.bias, slope=net.slope, stride=S.IKC_STRIDES[i])
            branches.append(t[:, :m.out_channels].cpu() > 0)
        assert t.shape[2:] == (19, 35) and torch.equal(ops.map_mean(t, M), out.detach())
    ref = S.twin(sd, torch.float64, **cfg)
    want, decided = P.twin_forward(ref, x, branches)
    assert decided <= 2
    want.backward(cot.double())
    assert 0.005 < float(want.detach().abs().mean()) < 10, "test bug: degenerate outputs"
    worst = P.rel_l2(out, want)
    assert worst < 5e-5, ("output", worst)
    for (k, p), q in zip(net.named_parameters(), ref.parameters()):
        err = P.rel_l2(p.grad, q.grad)
        worst = max(worst, err)
        assert err < 5e-5, (k, err)
    print("IKC predictor parity", cfg, "largest relative L2 distance from float64: %.3g" % worst, "at-the-kink:", decided)
