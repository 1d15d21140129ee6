"""Dense-block growth convs on the HIP kernels (pytest -m gpu): forward in place, input gradient (accumulating and not) and
weight / bias gradient against the float64 references of tests/_exact.py on dyadic data -- after `assert_budget` every
comparison is exact -- and what the kernels must leave alone: every channel of a stack outside the range they own."""
import pytest
import torch

import _dense as D
import _exact as E
import sisr_amd

pytestmark = pytest.mark.gpu
ops, hip = sisr_amd.ops, sisr_amd.hip
DEV = "cuda:0"
GROW = 32
GSLOPE = 0.25  # the gradient tests' slope: dyadic, so that slope * dy is exact (0.2f * dy is not: tests/_exact.py's budget)


def _case(hw, B, cin, seed):
    H, W = hw
    x = E.ints((B, cin, H, W), seed, zeros=0.25)
    w = E.weights((GROW, cin, 3, 3), seed + 1)
    b = E.biases(GROW, seed + 2)
    return H, W, x, w, b


@pytest.mark.parametrize("hw", D.SIZES)
@pytest.mark.parametrize("B", D.BATCHES)
@pytest.mark.parametrize("cin", D.CINS)
def test_dense_forward_in_place_is_exact_and_touches_only_its_slot(hw, B, cin):
    H, W, x, w, b = _case(hw, B, cin, 500)
    E.conv_budget(x.to(DEV), w.to(DEV), extras=(b,), what="dense forward")
    pre = E.conv_ref(x.to(DEV), w.to(DEV), b.to(DEV))
    for act, slope in ((True, 0.2), (True, 0.0), (False, 0.2)):
        S = D.stack([(0, x)], B, H, W, DEV)
        before = S.clone()
        slot = ops.dense_conv(S, cin, w.to(DEV), b.to(DEV), slope=slope, act=act)
        assert slot.data_ptr() == S.data_ptr() + 4 * cin and slot.shape == (B, GROW, H, W)
        ref = pre if not act else (E.leaky_ref(pre) if slope else pre.clamp(min=0))
        E.assert_exact(S[:, cin:cin + GROW], ref, "dense forward cin=%d act=%s slope=%s" % (cin, act, slope))
        assert D.same_bits(S[:, :cin], before[:, :cin]), "the input channels were written"
        assert D.same_bits(S[:, cin + GROW:], before[:, cin + GROW:]), "channels behind the slot were written"


@pytest.mark.parametrize("hw", D.SIZES)
def test_dense_forward_between_separate_buffers_of_other_pitches(hw):
    """pitch-64 input to a pitch-32 output (no bias, no activation): pins the pitch arithmetic of both sides"""
    B, cin = 2, 64
    H, W, x, w, _ = _case(hw, B, cin, 510)
    E.conv_budget(x.to(DEV), w.to(DEV), what="dense forward")
    xs = D.stack([(0, x)], B, H, W, DEV, pitch=64)
    y = torch.full((B, GROW, H, W), float("nan"), device=DEV).contiguous(memory_format=D.CL)
    pf, _ = ops.dense_pack(w.to(DEV), need_dgrad=False)
    hip.check(hip.lib().sisr_dense3x3_fwd(hip.ptr(xs), 64, cin, hip.ptr(pf), None, 0, 0.2, hip.ptr(y), 32, B, H, W, hip.stream()),
              "sisr_dense3x3_fwd")
    E.assert_exact(y, E.conv_ref(x.to(DEV), w.to(DEV)), "dense forward 64 -> 32 between buffers")


def _gradient_case(hw, B, cin, seed):
    H, W, x, w, _ = _case(hw, B, cin, seed)
    dy, m = E.ints((B, GROW, H, W), seed + 3), E.ints((B, GROW, H, W), seed + 4, -1, 1)
    if B * H * W >= 64:
        assert (m > 0).any() and (m < 0).any() and (m == 0).any(), "test bug: the mask map needs all three signs"
    eff = dy.double() * E.leaky_mask(m, GSLOPE)
    assert torch.equal(eff, torch.where(m > 0, dy.double(), GSLOPE * dy.double()))  # zero takes the slope branch
    return H, W, x, w, dy, m, eff


@pytest.mark.parametrize("hw", D.SIZES)
@pytest.mark.parametrize("B", D.BATCHES)
@pytest.mark.parametrize("cin", D.CINS)
def test_dense_dgrad_accumulates_in_place_exactly_and_leaves_the_rest(hw, B, cin):
    H, W, x, w, dy, m, eff = _gradient_case(hw, B, cin, 520)
    prefill = E.ints((B, cin, H, W), 527, -4, 4)
    D.gradient_budgets(x, w, eff, prefill, "dense")
    ref = E.dgrad_ref(eff.to(DEV), w.to(DEV))
    _, pd = ops.dense_pack(w.to(DEV))
    S = D.stack([(0, x), (cin, m)], B, H, W, DEV)  # the mask is the slot of the forward stack
    for accumulate in (1, 0):
        dS = D.stack([(0, prefill), (cin, dy)], B, H, W, DEV)
        before = dS.clone()
        hip.check(hip.lib().sisr_dense3x3_dgrad(hip.ptr(dS) + 4 * cin, D.PITCH, hip.ptr(S) + 4 * cin, D.PITCH, GSLOPE, hip.ptr(pd),
                                                hip.ptr(dS), D.PITCH, cin, accumulate, B, H, W, hip.stream()),
                  "sisr_dense3x3_dgrad")
        want = ref + prefill.double().to(DEV) if accumulate else ref
        E.assert_exact(dS[:, :cin], want, "dense dgrad cin=%d accumulate=%d" % (cin, accumulate))
        assert D.same_bits(dS[:, cin:], before[:, cin:]), "dy's slot or the sentinels behind it were written"


@pytest.mark.parametrize("hw", D.SIZES)
@pytest.mark.parametrize("B", D.BATCHES)
@pytest.mark.parametrize("cin", D.CINS)
def test_dense_wgrad_and_bias_gradient_are_exact_and_repeat_bit_for_bit(hw, B, cin):
    H, W, x, w, dy, m, eff = _gradient_case(hw, B, cin, 530)
    D.gradient_budgets(x, w, eff, None, "dense")
    S = D.stack([(0, x), (cin, m)], B, H, W, DEV)
    dS = D.stack([(cin, dy)], B, H, W, DEV)
    L = hip.lib()
    nb = L.sisr_dense3x3_wgrad_workspace_bytes(B, H, W, cin)
    assert nb > 0
    ws = hip.workspace(torch.device(DEV), nb)
    got = []
    for _ in range(2):
        dw, db = torch.full((GROW, cin, 3, 3), float("nan"), device=DEV), torch.full((GROW,), float("nan"), device=DEV)
        hip.check(L.sisr_dense3x3_wgrad(hip.ptr(S), D.PITCH, cin, hip.ptr(dS) + 4 * cin, D.PITCH, hip.ptr(S) + 4 * cin, D.PITCH,
                                        GSLOPE, hip.ptr(dw), hip.ptr(db), hip.ptr(ws), nb, B, H, W, hip.stream()),
                  "sisr_dense3x3_wgrad")
        got.append((dw, db))
    E.assert_exact(got[0][0], E.wgrad_ref(x.to(DEV), eff.to(DEV)), "dense wgrad cin=%d" % cin)
    E.assert_exact(got[0][1], eff.sum(dim=(0, 2, 3)), "dense bias gradient cin=%d" % cin)
    assert D.same_bits(got[0][0], got[1][0]) and D.same_bits(got[0][1], got[1][1]), "two calls must give identical bits"
    dw = torch.full((GROW, cin, 3, 3), float("nan"), device=DEV)  # without a mask and without a bias gradient
    hip.check(L.sisr_dense3x3_wgrad(hip.ptr(S), D.PITCH, cin, hip.ptr(dS) + 4 * cin, D.PITCH, None, 0, GSLOPE, hip.ptr(dw), None,
                                    hip.ptr(ws), nb, B, H, W, hip.stream()), "sisr_dense3x3_wgrad")
    E.assert_exact(dw, E.wgrad_ref(x.to(DEV), dy.to(DEV)), "dense wgrad without a mask")


def test_dense_skip_reads_and_writes_stacks_at_their_pitch():
    B, H, W = 2, 9, 21
    t, x, g = E.ints((B, 64, H, W), 540), E.ints((B, 64, H, W), 541), E.scales((B, 64), 542)
    ts, xs = D.stack([(0, t)], B, H, W, DEV), D.stack([(0, x)], B, H, W, DEV, pitch=64)
    y = ops.dense_skip(ts[:, :64], g.to(DEV), xs)
    E.assert_exact(y, t.double() * g.double()[:, :, None, None] + x.double(), "dense skip")
    assert y.stride() == (H * W * D.PITCH, 1, W * D.PITCH, D.PITCH), "the result opens a new stack"
