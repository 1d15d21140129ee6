"""The exact-data helper (tests/_exact.py) on its own, no GPU: its shifted-matmul references equal ATen's float64 conv and
autograd, its budget check accepts the planned cases and rejects an over-budget one, its generators are deterministic."""
import pytest
import torch
import torch.nn.functional as F

import _exact as X


@pytest.mark.parametrize("B,C,O,H,W", [(2, 5, 7, 6, 9), (1, 3, 64, 1, 1), (1, 64, 3, 2, 1), (2, 8, 4, 1, 7), (1, 4, 6, 13, 2)])
def test_shifted_matmuls_equal_aten_conv_and_its_autograd(B, C, O, H, W):
    x = X.ints((B, C, H, W), seed=1).double().requires_grad_(True)
    w = X.weights((O, C, 3, 3), seed=2).double().requires_grad_(True)
    b = X.biases(O, seed=3).double().requires_grad_(True)
    dy = X.ints((B, O, H, W), seed=4).double()
    want = F.conv2d(x, w, b, padding=1)
    got = X.conv_ref(x, w, b)
    assert torch.equal(got, want)
    gx, gw, gb = torch.autograd.grad(want, (x, w, b), dy)
    assert torch.equal(X.dgrad_ref(dy, w.detach()), gx)
    assert torch.equal(X.wgrad_ref(x.detach(), dy), gw)
    assert torch.equal(dy.sum(dim=(0, 2, 3)), gb)
    # autograd through the reference itself gives the same gradients (the geometric references rely on it)
    assert all(torch.equal(a, c) for a, c in zip(torch.autograd.grad(got, (x, w, b), dy), (gx, gw, gb)))


def test_9x9_reference_equals_aten():
    x = X.ints((1, 64, 5, 11), seed=5, lo=-1, hi=1).double()
    w = X.weights((3, 64, 9, 9), seed=6).double()
    assert torch.equal(X.conv_ref(x, w), F.conv2d(x, w, padding=4))
    dy = X.ints((1, 3, 5, 11), seed=7).double()
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    gx, gw = torch.autograd.grad(F.conv2d(xr, wr, padding=4), (xr, wr), dy)
    assert torch.equal(X.dgrad_ref(dy, w), gx)
    assert torch.equal(X.wgrad_ref(x, dy, padding=4, k=9), gw)


@pytest.mark.parametrize("up,stride,H,W", [(1, 1, 5, 7), (2, 1, 3, 4), (1, 2, 7, 5), (1, 2, 2, 2), (2, 1, 2, 3), (1, 2, 6, 9)])
def test_geometric_reference_equals_reflect_nearest_aten(up, stride, H, W):
    x = X.ints((2, 6, H, W), seed=8).double().requires_grad_(True)
    w = X.weights((5, 6, 3, 3), seed=9).double().requires_grad_(True)
    b = X.biases(5, seed=10).double().requires_grad_(True)
    t = F.interpolate(x, scale_factor=up, mode="nearest") if up > 1 else x
    want = F.conv2d(F.pad(t, (1, 1, 1, 1), mode="reflect"), w, b, stride=stride)
    got = X.geo_conv_ref(x, w, b, up=up, stride=stride)
    assert torch.equal(got, want)
    dy = X.ints(want.shape, seed=11).double()
    for a, c in zip(torch.autograd.grad(got, (x, w, b), dy), torch.autograd.grad(want, (x, w, b), dy)):
        assert torch.equal(a, c)


def test_masks_follow_pytorch_tie_conventions():
    m = torch.tensor([-1.0, 0.0, 0.5, -0.0])
    assert X.relu_mask(m).tolist() == [0.0, 0.0, 1.0, 0.0]  # ReLU': 0 at a tie
    assert X.leaky_mask(m).tolist() == [X.SLOPE32, X.SLOPE32, 1.0, X.SLOPE32]  # LeakyReLU': the slope at a tie
    v = torch.tensor([-3.0, 0.0, 2.0, -7.0], dtype=torch.float64)
    got = X.leaky_ref(v)
    want = (v.float() * torch.tensor(0.2, dtype=torch.float32)).double()  # fp32 multiply by 0.2f, one rounding
    assert torch.equal(got, torch.where(v > 0, v, want))


def test_generators_are_deterministic_and_exact():
    for fn, args in ((X.ints, ((4, 64, 5, 5),)), (X.weights, ((64, 64, 3, 3),)), (X.scales, ((3, 64),)), (X.shifts, ((3, 64),)),
                     (X.nonzero_ints, ((9, 9),))):
        a, b, c = fn(*args, seed=12), fn(*args, seed=12), fn(*args, seed=13)
        assert torch.equal(a, b) and not torch.equal(a, c)
        assert torch.equal(a.to(torch.bfloat16).float(), a), fn.__name__  # bf16-exact
    assert torch.equal(X.biases(64, seed=1), X.biases(64, seed=1))
    x = X.ints((100000,), seed=14, zeros=0.3)
    share = float((x == 0).float().mean())
    assert 0.3 < share < 0.5  # forced zeros plus the generator's own (1 in 5)
    assert set(X.ints((1000,), seed=15, lo=-1, hi=1).unique().tolist()) == {-1.0, 0.0, 1.0}
    assert set(X.weights((1000,), seed=16).mul(8).unique().tolist()) == set(float(k) for k in range(-4, 5))
    assert set(X.scales((1000,), seed=17).unique().tolist()) == {0.5, 1.0, 1.5, 2.0}
    assert (X.nonzero_ints((1000,), seed=18) != 0).all()
    assert (X.weights((1000,), seed=19, nonzero=True) != 0).all()


def test_granule():
    assert X.granule(torch.tensor([1.0, -2.0, 3.0])) == 1.0
    assert X.granule(torch.tensor([0.5, 1.25])) == 0.25
    assert X.granule(torch.tensor([4.0]), torch.tensor([0.125])) == 0.125
    assert X.granule(torch.zeros(3)) == 1.0
    with pytest.raises(AssertionError):
        X.granule(torch.tensor([0.1], dtype=torch.float64))


def test_budget_accepts_the_planned_cases_and_rejects_an_oversized_one():
    # the 64 -> 64 conv on {-2..2} x k/8 data with affine prologue values: far below 2^22
    x = X.ints((1, 64, 6, 6), seed=20) * X.scales((1, 64, 1, 1), seed=21) + X.shifts((1, 64, 1, 1), seed=22)
    w = X.weights((64, 64, 3, 3), seed=23)
    assert X.conv_budget(x, w, extras=(X.biases(64, seed=24),)) < 17
    assert X.winograd_budget(x, w) < 22
    # a 32 x 128^2 weight gradient on {-1, 0, 1} data with half the entries zero fits ...
    assert X.budget_bits(32 * 128 * 128 * 0.25, 1.0) < 22
    # ... a contraction whose partial sums need 23 bits is refused as a test bug, not passed on as a kernel failure
    big = torch.full((1, 64, 4, 4), 2.0 ** 14)
    with pytest.raises(AssertionError, match="TEST BUG"):
        X.conv_budget(big, torch.full((64, 64, 3, 3), 1.0))
    with pytest.raises(AssertionError, match="TEST BUG"):
        X.wgrad_budget(torch.ones(1, 1, 2048, 2048), torch.full((1, 1, 2048, 2048), 2.0))  # 2^23 per tap


def test_comparison_sees_unwritten_and_single_term_errors():
    ref = X.conv_ref(X.ints((1, 4, 5, 5), seed=30), X.weights((4, 4, 3, 3), seed=31))
    got = ref.float().clone()
    X.assert_exact(got, ref)
    got[0, 1, 2, 3] = float("nan")
    bad = X.mismatch(got, ref)
    assert bad.sum() == 1 and bad[0, 1, 2, 3]
    got[0, 1, 2, 3] = ref[0, 1, 2, 3] + 0.125
    with pytest.raises(AssertionError, match="1 of 100"):
        X.assert_exact(got, ref)
    assert torch.equal(X.bf16_of(torch.tensor([257.0], dtype=torch.float64)).float(), torch.tensor([256.0]))  # RNE tie to even
