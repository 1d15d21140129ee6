"""The gate references (tests/_gates.py) on their own, no GPU: each hand-written forward and backward formula equals float64
autograd of the oracle's own functions (O.ca_gate, O.para_ca_gate, O.qca_layer, O.pa_layer, F.l1_loss), ReLU' ties at
exactly 0 included, and the |.| (A) form of every backward bounds its value form."""
import pytest
import torch
import torch.nn.functional as F

import _exact as X
import _gates as G
from oracle import sisr_oracle as O


def close(got, want, what=""):
    """float64 against float64 in another summation order: agreement to 1e-12 of the largest value"""
    got, want = got.detach().double(), want.detach().double().reshape(got.shape)
    tol = 1e-12 * max(float(want.abs().max()), 1.0)
    assert float((got - want).abs().max()) <= tol, f"{what}: max |diff| {float((got - want).abs().max())}"


def leaf(t):
    return t.double().clone().requires_grad_(True)


def mag_bounds(ref, mag):
    for k, v in ref.items():
        if v is None:
            continue
        vs = v if isinstance(v, list) else [v]
        ms = mag[k] if isinstance(mag[k], list) else [mag[k]]
        for a, m in zip(vs, ms):
            assert bool((a.abs() <= m + 1e-12 * (1 + m)).all()), f"|{k}| exceeds its A-form magnitude"


# ----------------------------------------------------------------------------- CA gate
@pytest.mark.parametrize("B,R,H,W,with_mul", [(2, 4, 3, 5, False), (3, 1, 2, 2, True), (9, 16, 1, 4, True), (1, 5, 4, 4, False)])
def test_ca_gate_reference_equals_oracle_autograd(B, R, H, W, with_mul):
    x = leaf(X.ints((B, 64, H, W), 11, zeros=0.3))
    w1, b1 = leaf(X.weights((R, 64), 12)), leaf(X.biases(R, 13))
    w2, b2 = leaf(X.weights((64, R), 14)), leaf(X.biases(64, 15))
    mul = leaf(X.scales((B, 64), 16)) if with_mul else None
    sd = {"k.conv_du.0.weight": w1.view(R, 64, 1, 1), "k.conv_du.0.bias": b1,
          "k.conv_du.2.weight": w2.view(64, R, 1, 1), "k.conv_du.2.bias": b2}
    ca = O.ca_gate(sd, "k", x).view(B, 64)
    g = ca * mul if with_mul else ca
    s = x.detach().mean(dim=(2, 3))
    ref = G.ca_fwd_ref(s, w1, b1, w2, b2, mul)
    close(ref["ca"], ca, "ca")
    close(ref["g"], g, "g")
    dg = X.ints((B, 64), 17).double()
    want = torch.autograd.grad(g, [x, w1, b1, w2, b2] + ([mul] if with_mul else []), dg)
    got = G.ca_bwd_ref(dg, ref["ca"], ref["hid"], s, w1, w2, mul, inv_hw=1.0 / (H * W))
    close(got["shift"], want[0][:, :, 0, 0], "shift (d x, broadcast over the pixels)")
    assert torch.equal(want[0], want[0][:, :, :1, :1].expand_as(want[0]))
    for k, w in zip(("dw1", "db1", "dw2", "db2"), want[1:5]):
        close(got[k], w, k)
    if with_mul:
        close(got["dmul"], want[5], "dmul")
    mag_bounds(got, G.ca_bwd_ref(dg, ref["ca"], ref["hid"], s, w1, w2, mul, inv_hw=1.0 / (H * W), A=True))


def test_ca_gate_relu_tie_has_zero_gradient():
    """a hidden pre-activation exactly 0: the reference's dz1 is 0 there, as PyTorch's ReLU' gives"""
    s = torch.zeros(2, 64)
    s[0, 3] = 1.0
    w1, b1 = X.weights((4, 64), 1, nonzero=True), torch.zeros(4)
    w2, b2 = X.weights((64, 4), 2, nonzero=True), X.biases(64, 3)
    ref = G.ca_fwd_ref(s, w1, b1, w2, b2)
    assert bool((ref["pre"][1] == 0).all())
    dz1 = G.ca_bwd_ref(torch.ones(2, 64), ref["ca"], ref["hid"], s, w1, w2)["dz1"]
    assert bool((dz1[1] == 0).all())
    x = leaf(s.view(2, 64, 1, 1))
    sd = {"k.conv_du.0.weight": leaf(w1.view(4, 64, 1, 1)), "k.conv_du.0.bias": leaf(b1),
          "k.conv_du.2.weight": leaf(w2.view(64, 4, 1, 1)), "k.conv_du.2.bias": leaf(b2)}
    (gb1,) = torch.autograd.grad(O.ca_gate(sd, "k", x).sum(), [sd["k.conv_du.0.bias"]])
    close(G.ca_bwd_ref(torch.ones(2, 64), ref["ca"], ref["hid"], s, w1, w2)["db1"], gb1, "db1 at the tie")


# ----------------------------------------------------------------------------- meta gate
@pytest.mark.parametrize("B,M,Hd,C,relu", [(2, 10, 32, 64, True), (3, 1, 5, 7, False), (5, 20, 42, 64, True), (1, 33, 16, 300, False)])
def test_meta_gate_reference_equals_oracle_autograd(B, M, Hd, C, relu):
    md = leaf(X.ints((B, M), 21, -1, 1))
    v1, c1 = leaf(X.weights((Hd, M), 22)), leaf(X.biases(Hd, 23))
    v2, c2 = leaf(X.weights((C, Hd), 24)), leaf(X.biases(C, 25))
    i2 = 2 if relu else 1
    sd = {"k.attribute_integrator.0.weight": v1.view(Hd, M, 1, 1), "k.attribute_integrator.0.bias": c1,
          f"k.attribute_integrator.{i2}.weight": v2.view(C, Hd, 1, 1), f"k.attribute_integrator.{i2}.bias": c2}
    m = O.para_ca_gate(sd, "k", md.view(B, M, 1, 1), relu).view(B, C)
    ref = G.meta_fwd_ref(md, v1, c1, v2, c2, relu)
    close(ref["m"], m, "m")
    if relu:
        assert bool((ref["pre"] == 0).any()), "no ReLU tie in the data"
    dm = X.ints((B, C), 26).double()
    want = torch.autograd.grad(m, [md, v1, c1, v2, c2], dm)
    got = G.meta_bwd_ref(dm, ref["m"], ref["hid"], md, v1, v2, relu)
    for k, w in zip(("dmd", "dv1", "dc1", "dv2", "dc2"), want):
        close(got[k], w, k)
    mag_bounds(got, G.meta_bwd_ref(dm, ref["m"], ref["hid"], md, v1, v2, relu, A=True))


# ----------------------------------------------------------------------------- gate MLP (QCALayer styles, wide CA)
STYLE_KEYS = {
    "modulate": ["conv_du.0", "conv_du.2"], "max_concat": ["conv_du.0", "conv_du.2"], "softmax": ["conv_du.0", "conv_du.2"],
    "mini_concat": ["pre_concat", "conv_du.1"],
    "extended_attention": ["feature_convs.0.0", "feature_convs.1.0", "feature_convs.2.0", "final_conv.0"],
}
QCA_STYLES = {  # the layout of ops.QCA_STYLES (restated: this test must not import the package)
    "modulate": ([(0, 0, 1), (0, 0, 2)], 2),
    "max_concat": ([(1, 0, 1), (0, 0, 2)], 0),
    "softmax": ([(1, 0, 1), (0, 0, 2)], 1),
    "mini_concat": ([(0, 0, 0), (1, 1, 2)], 0),
    "extended_attention": ([(1, 0, 1), (1, 0, 1), (1, 0, 1), (0, 0, 2)], 0),
}


def style_widths(style, C, M):
    """[(nout, inw)] of a style's layers"""
    if style == "extended_attention":
        return [(32, C + M), (16, 32 + M), (4, 16 + M), (C, 4)]
    if style == "mini_concat":
        return [(4, C), (C, 4 + M)]
    if style == "modulate":
        return [(4, C), (C, 4)]
    return [(4, C + M), (C, 4)]


@pytest.mark.parametrize("style", sorted(QCA_STYLES))
@pytest.mark.parametrize("with_mul", [False, True])
def test_gate_mlp_reference_equals_oracle_qca_layer(style, with_mul):
    """out = x * gate on a 1x1 map (gap(x) = x): d x = dy * gate + d pool(dy * x)"""
    B, C = 3, 64
    M = C if style == "modulate" else 10
    x = leaf(X.ints((B, C), 31, zeros=0.2) / 2)
    md = leaf(X.ints((B, M), 32, -2, 2))
    ws, bs, sd = [], [], {}
    for k, (key, (nout, inw)) in enumerate(zip(STYLE_KEYS[style], style_widths(style, C, M))):
        ws.append(leaf(X.weights((nout, inw), 33 + k)))
        bs.append(leaf(X.biases(nout, 43 + k)))
        sd[f"k.{key}.weight"], sd[f"k.{key}.bias"] = ws[-1].view(nout, inw, 1, 1), bs[-1]
    mul = leaf(X.scales((B, C), 50)) if with_mul else None
    out = O.qca_layer(sd, "k", x.view(B, C, 1, 1), md.view(B, M, 1, 1), style).view(B, C)
    if with_mul:
        out = out * mul
    spec = QCA_STYLES[style]
    ref = G.mlp_fwd_ref(x, md, ws, bs, spec, mul)
    close(ref["y"] * x.detach(), out, "gate")
    dy = X.ints((B, C), 51).double()
    want = torch.autograd.grad(out, [x, md] + ws + bs + ([mul] if with_mul else []), dy)
    got = G.mlp_bwd_ref(dy * x.detach(), md, mul, ws, spec, ref["acts"], ref["yfin"])
    close(got["dpool"] + dy * ref["y"], want[0], "d pool")
    close(got["dmd"], want[1], "d metadata")
    L = len(ws)
    for k in range(L):
        close(got["dws"][k], want[2 + k], f"dW{k}")
        close(got["dbs"][k], want[2 + L + k], f"db{k}")
    if with_mul:
        close(got["dmul"], want[-1], "d mul")
    mag_bounds(got, G.mlp_bwd_ref(dy * x.detach(), md, mul, ws, spec, ref["acts"], ref["yfin"], A=True))


def test_mini_concat_relu_masks_the_metadata_gradient():
    """mini_concat: ReLU(cat(., md)) -- metadata <= 0 gets no gradient (PyTorch's ReLU' at 0 is 0)"""
    B, C, M = 2, 64, 6
    md = torch.tensor([[-2.0, 0.0, 1.0, -1.0, 2.0, 0.0], [0.0, 1.0, -1.0, 0.0, 0.0, 2.0]])
    ws = [X.weights((4, C), 1), X.weights((C, 4 + M), 2, nonzero=True)]
    bs = [X.biases(4, 3), X.biases(C, 4)]
    spec = QCA_STYLES["mini_concat"]
    ref = G.mlp_fwd_ref(X.ints((B, C), 5), md, ws, bs, spec)
    got = G.mlp_bwd_ref(X.ints((B, C), 6).double(), md, None, ws, spec, ref["acts"], ref["yfin"])
    assert bool((got["dmd"][md <= 0] == 0).all()) and bool((got["dmd"][md > 0] != 0).any())


@pytest.mark.parametrize("C", [128, 256])
def test_wide_ca_spec_equals_oracle_ca_gate(C):
    """the generic MLP with ([(0,0,1),(0,0,2)], 0) is the CA gate at C > 64 (ops.ca_layer's wide path)"""
    B, R, H, W = 2, C // 16, 2, 3
    x = leaf(X.ints((B, C, H, W), 61))
    w1, b1, w2, b2 = leaf(X.weights((R, C), 62)), leaf(X.biases(R, 63)), leaf(X.weights((C, R), 64)), leaf(X.biases(C, 65))
    sd = {"k.conv_du.0.weight": w1.view(R, C, 1, 1), "k.conv_du.0.bias": b1,
          "k.conv_du.2.weight": w2.view(C, R, 1, 1), "k.conv_du.2.bias": b2}
    ca = O.ca_gate(sd, "k", x).view(B, C)
    spec = ([(0, 0, 1), (0, 0, 2)], 0)
    s = x.detach().mean(dim=(2, 3))
    ref = G.mlp_fwd_ref(s, torch.zeros(B, 1), [w1, w2], [b1, b2], spec)
    close(ref["y"], ca, "wide CA gate")
    dy = X.ints((B, C), 66).double()
    want = torch.autograd.grad(ca, [x, w1, b1, w2, b2], dy)
    got = G.mlp_bwd_ref(dy, torch.zeros(B, 1), None, [w1, w2], spec, ref["acts"], ref["yfin"])
    close(got["dpool"] / (H * W), want[0][:, :, 0, 0], "d pool / hw")
    for a, b in zip([got["dws"][0], got["dbs"][0], got["dws"][1], got["dbs"][1]], want[1:]):
        close(a, b)


# ----------------------------------------------------------------------------- pixel attention
def test_pa_reference_equals_oracle_autograd():
    B, H, W = 2, 5, 7
    x = leaf(X.ints((B, 64, H, W), 71, zeros=0.3))
    with torch.no_grad():
        x[1, :, 2, 3] = 0  # that pixel's hidden pre-activations are b1: exactly 0 where b1 is
    w1, b1, w2, b2 = leaf(X.weights((8, 64), 72)), leaf(X.biases(8, 73)), leaf(X.weights((8,), 74)), leaf(X.biases(1, 75))
    with torch.no_grad():
        b1[::2] = 0
    sd = {"k.pa.0.weight": w1.view(8, 64, 1, 1), "k.pa.0.bias": b1, "k.pa.2.weight": w2.view(1, 8, 1, 1), "k.pa.2.bias": b2}
    y = O.pa_layer(sd, "k", x)
    xr = x.detach().permute(0, 2, 3, 1).reshape(-1, 64)
    ref = G.pa_fwd_ref(xr, w1, b1, w2, b2)
    assert bool((ref["pre"] == 0).any()), "no ReLU tie in the data"
    close(ref["y"], y.permute(0, 2, 3, 1).reshape(-1, 64), "y")
    dy = X.ints((B, 64, H, W), 76)
    want = torch.autograd.grad(y, [x, w1, b1, w2, b2], dy.double())
    got = G.pa_bwd_ref(xr, w1, b1, w2, b2, dy.permute(0, 2, 3, 1).reshape(-1, 64))
    close(got["dx"], want[0].permute(0, 2, 3, 1).reshape(-1, 64), "dx")
    for k, w in zip(("dw1", "db1", "dw2", "db2"), want[1:]):
        close(got[k], w, k)
    mag_bounds(got, G.pa_bwd_ref(xr, w1, b1, w2, b2, dy.permute(0, 2, 3, 1).reshape(-1, 64), A=True))


# ----------------------------------------------------------------------------- pixel sums, residual, L1
@pytest.mark.parametrize("hw", [1, 17, 512, 513, 1025, 65537])
def test_dg_partials_sum_to_the_pixel_sum(hw):
    dy, t = X.ints((2, hw, 4), 81), X.ints((2, hw, 4), 82)
    parts = G.dg_parts(hw)
    assert parts == min(128, -(-hw // 512))
    p = G.dg_partial_ref(dy, t, parts)
    assert torch.equal(p.sum(1), (dy.double() * t.double()).sum(1))
    assert torch.equal(G.dg_partial_ref(dy, None, parts).sum(1), dy.double().sum(1))


def test_residual_reference():
    t, x = X.ints((2, 3, 8), 91), X.ints((2, 3, 8), 92)
    g, sh = X.scales((2, 8), 93), X.shifts((2, 8), 94)
    assert torch.equal(G.residual_ref(t, g, sh, x), (t * g[:, None] + sh[:, None] + x).double())
    assert torch.equal(G.residual_ref(t), t.double())


@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_l1_reference_equals_autograd(n):
    a = leaf(X.ints((n,), 101))
    b = X.ints((n,), 102).double()
    loss = F.l1_loss(a, b)
    (ga,) = torch.autograd.grad(loss, [a])
    v, g = G.l1_ref(a, b)
    close(v, loss, "value")
    assert torch.equal(g, ga) or float((g - ga).abs().max()) <= 1e-15
    assert bool((g[a.detach() == b] == 0).all())
