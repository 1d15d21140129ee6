"""Float64 references of the gate kernels (helper module, not collected; torch only, no HIP import).

Hand-written forward and backward formulas of the channel-attention (CA) gate, the ParaCALayer meta gate, the generic gate
MLP of the metadata-mixing QCALayer styles, pixel attention (PA), the pixel sums, the gated residual and the L1 loss.
tests/test_gates_cpu.py checks every one of them against float64 autograd of the oracle's own functions; the GPU tests
(tests/test_gates_gpu.py) compare the kernels with them.

Backward references take a flag `A`: False evaluates the formula, True the SAME computation on absolute values with every
subtraction turned into an addition (1 - s -> 1 + s, dv - <dv, y> -> |dv| + <|dv|, y>).  The result bounds the magnitude
every fp32 rounding of the kernel's evaluation is relative to, so a forward error bound reads
    |got - ref| <= c * 2**-24 * mag,
c a small per-family constant (tests/test_gates_gpu.py states each).  Masks (ReLU') are always taken from the values, with
PyTorch's convention: the derivative at exactly 0 is 0.
"""
import torch

U = 2.0 ** -24


def _d(t):
    return None if t is None else t.detach().double()


def _ab(A):
    return (lambda t: None if t is None else t.abs()) if A else (lambda t: t)


def _one_minus(s, A):
    return 1 + s if A else 1 - s


# ----------------------------------------------------------------------------- comparisons (bounded tier)
def bound_ok(got, ref, mag, c):
    """bool map: |got - ref| <= c * 2^-24 * mag (NaN -- an unwritten element -- fails)"""
    got = got.detach().double()
    return (got - ref.to(got.device).double()).abs() <= c * U * mag.to(got.device).double()


def assert_bounded(got, ref, mag, c, what=""):
    ok = bound_ok(got, ref, mag, c)
    if bool(ok.all()):
        return
    bad = ~ok
    idx = bad.nonzero()[:5].tolist()
    g, r, m = got.detach().double(), ref.to(got.device).double(), mag.to(got.device).double()
    vals = [(float(g[tuple(i)]), float(r[tuple(i)]), c * U * float(m[tuple(i)])) for i in idx]
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside {c} * 2^-24 * mag of the float64 "
                         f"value; first at {idx}: (got, float64, bound) = {vals}")


# ----------------------------------------------------------------------------- CA gate (C = 64, R hidden units)
def ca_fwd_ref(s, w1, b1, w2, b2, mul=None):
    """s [B,64] pooled mean, w1 [R,64], b1 [R], w2 [64,R], b2 [64], mul [B,64] or None ->
    pre = W1 s + b1, hid = relu(pre), z = W2 hid + b2, ca = sigmoid(z), g = ca [* mul]"""
    s, w1, b1, w2, b2, mul = map(_d, (s, w1, b1, w2, b2, mul))
    pre = s @ w1.T + b1
    hid = torch.relu(pre)
    z = hid @ w2.T + b2
    ca = torch.sigmoid(z)
    return dict(pre=pre, hid=hid, z=z, ca=ca, g=ca * mul if mul is not None else ca)


def ca_fwd_mag(s, w1, b1, w2, b2):
    """|.| computation of the CA forward's two contractions (the exact-data budget of pre and z)"""
    s, w1, b1, w2, b2 = (t.detach().double().abs() for t in (s, w1, b1, w2, b2))
    pre = s @ w1.T + b1
    return dict(pre=pre, z=pre @ w2.T + b2)


def ca_bwd_ref(dg, ca, hid, s, w1, w2, mul=None, inv_hw=1.0, A=False):
    """dg [B,64] = sum_hw dOut * t;  dca = dg [* mul]; dmul = dg * ca; dz2 = dca * ca * (1 - ca); dz1 = (W2^T dz2) * [hid > 0];
    shift = (W1^T dz1) * inv_hw (the GAP backward broadcast); dw2 = sum_b dz2 (x) hid, dw1 = sum_b dz1 (x) s, db2, db1"""
    mask = (_d(hid) > 0).double()
    dg, ca, hid, s, w1, w2, mul = map(_ab(A), map(_d, (dg, ca, hid, s, w1, w2, mul)))
    dca = dg * mul if mul is not None else dg
    dz2 = dca * ca * _one_minus(ca, A)
    dz1 = (dz2 @ w2) * mask
    ds = dz1 @ w1
    return dict(dmul=dg * ca if mul is not None else None, dz2=dz2, dz1=dz1, shift=ds * inv_hw, dw2=dz2.T @ hid,
                dw1=dz1.T @ s, db2=dz2.sum(0), db1=dz1.sum(0))


# ----------------------------------------------------------------------------- meta gate (ParaCALayer)
def meta_fwd_ref(md, v1, c1, v2, c2, relu):
    """md [B,M], v1 [Hd,M], c1 [Hd], v2 [C,Hd], c2 [C] -> pre, hid = act(pre), z, m = sigmoid(z)"""
    md, v1, c1, v2, c2 = map(_d, (md, v1, c1, v2, c2))
    pre = md @ v1.T + c1
    hid = torch.relu(pre) if relu else pre
    z = hid @ v2.T + c2
    return dict(pre=pre, hid=hid, z=z, m=torch.sigmoid(z))


def meta_fwd_mag(md, v1, c1, v2, c2):
    md, v1, c1, v2, c2 = (t.detach().double().abs() for t in (md, v1, c1, v2, c2))
    pre = md @ v1.T + c1
    return dict(pre=pre, z=pre @ v2.T + c2)


def meta_bwd_ref(dm, m, hid, md, v1, v2, relu, A=False):
    """dz2 = dm * m * (1 - m); dz1 = (V2^T dz2) [* (hid > 0)]; dmd = V1^T dz1; dv2 = sum_b dz2 (x) hid, dc2 = sum_b dz2,
    dv1 = sum_b dz1 (x) md, dc1 = sum_b dz1.  hid is the stored activation (post-ReLU when relu)."""
    mask = (_d(hid) > 0).double() if relu else torch.ones_like(_d(hid))
    dm, m, hid, md, v1, v2 = map(_ab(A), map(_d, (dm, m, hid, md, v1, v2)))
    dz2 = dm * m * _one_minus(m, A)
    dz1 = (dz2 @ v2) * mask
    return dict(dz2=dz2, dz1=dz1, dmd=dz1 @ v1, dv2=dz2.T @ hid, dc2=dz2.sum(0), dv1=dz1.T @ md, dc1=dz1.sum(0))


# ----------------------------------------------------------------------------- generic gate MLP (QCALayer styles)
# spec = ([(cat metadata, ReLU on the layer input, act 0 none / 1 relu / 2 sigmoid)] per layer, final mode 0 / 1 softmax /
# 2 times the metadata) -- the layout of ops.QCA_STYLES
def _mlp_in(cur, md, cat):
    return torch.cat([cur, md], dim=1) if cat else cur


def mlp_fwd_ref(pool, md, ws, bs, spec, mul=None):
    """-> acts (list: the pooled input, then every layer's output), pre-activations zs, yfin (before mul), y"""
    layers, fm = spec
    pool, md, mul = _d(pool), _d(md), _d(mul)
    cur, acts, zs = pool, [pool], []
    for k, (cat, relu_in, act) in enumerate(layers):
        v = _mlp_in(cur, md, cat)
        if relu_in:
            v = torch.relu(v)
        z = v @ _d(ws[k]).T
        if bs[k] is not None:
            z = z + _d(bs[k])
        zs.append(z)
        cur = torch.relu(z) if act == 1 else torch.sigmoid(z) if act == 2 else z
        acts.append(cur)
    yfin = torch.softmax(cur, dim=1) if fm == 1 else cur * md if fm == 2 else cur
    return dict(acts=acts, zs=zs, yfin=yfin, y=yfin * mul if mul is not None else yfin)


def mlp_fwd_mag(pool, md, ws, bs, spec):
    """|.| computation of every layer's pre-activation (the exact-data budget of the layers before the sigmoid)"""
    layers, _ = spec
    ref = mlp_fwd_ref(pool, md, ws, bs, spec)
    md = _d(md).abs()
    mags = []
    for k, (cat, relu_in, act) in enumerate(layers):
        v = _mlp_in(ref["acts"][k].abs(), md, cat)
        z = v @ _d(ws[k]).abs().T
        if bs[k] is not None:
            z = z + _d(bs[k]).abs()
        mags.append(z)
    return mags


def mlp_bwd_ref(dy, md, mul, ws, spec, acts, yfin, A=False):
    """acts: the stored per-layer outputs (acts[0] = pool), yfin: the stored output before mul.  -> dzs (per layer),
    dpool, dmd, dmul, dws, dbs"""
    layers, fm = spec
    L = len(layers)
    acts = [_d(a) for a in acts]
    md_v = _d(md)
    act_mask = [(a > 0).double() for a in acts]
    ab = _ab(A)
    dy, md, mul, yfin = ab(_d(dy)), ab(md_v), ab(_d(mul)), ab(_d(yfin))
    ws = [ab(_d(w)) for w in ws]
    av = [ab(a) for a in acts]
    dmul = dy * yfin if mul is not None else None
    dv = dy * mul if mul is not None else dy
    dmd = torch.zeros_like(md)
    if fm == 1:
        red = (dv * yfin).sum(1, keepdim=True)
        dv = yfin * (dv + red if A else dv - red)
    elif fm == 2:
        dmd = dmd + dv * av[L]
        dv = dv * md
    dzs, dws, dbs = [None] * L, [None] * L, [None] * L
    for k in range(L - 1, -1, -1):
        cat, relu_in, act = layers[k]
        v = av[k + 1]
        g = dv * act_mask[k + 1] if act == 1 else dv * v * _one_minus(v, A) if act == 2 else dv
        dzs[k] = g
        raw_v = _mlp_in(acts[k], md_v, cat)
        inp = _mlp_in(av[k], md, cat)
        gin = g @ ws[k]
        if relu_in:
            gin = gin * (raw_v > 0).double()
            inp = inp * (raw_v > 0).double()  # relu(inp) (inp is |.| in A mode: masked by the values' sign)
        nin = acts[k].shape[1]
        if cat:
            dmd = dmd + gin[:, nin:]
        dv = gin[:, :nin]
        dws[k] = g.T @ inp
        dbs[k] = g.sum(0)
    return dict(dzs=dzs, dpool=dv, dmd=dmd, dmul=dmul, dws=dws, dbs=dbs)


# ----------------------------------------------------------------------------- pixel attention (64 -> 8 -> 1)
def pa_fwd_ref(x, w1, b1, w2, b2):
    """x [N,64], w1 [8,64], b1 [8], w2 [8], b2 [1] -> pre, a = relu(pre), z, g = sigmoid(z) [N], y = x * g"""
    x, w1, b1, w2, b2 = map(_d, (x, w1, b1, w2, b2))
    pre = x @ w1.T + b1
    a = torch.relu(pre)
    z = a @ w2 + b2
    g = torch.sigmoid(z)
    return dict(pre=pre, a=a, z=z, g=g, y=x * g[:, None])


def pa_fwd_mag(x, w1, b1, w2, b2):
    x, w1, b1, w2, b2 = (t.detach().double().abs() for t in (x, w1, b1, w2, b2))
    pre = x @ w1.T + b1
    return dict(pre=pre, z=pre @ w2 + b2)


def pa_bwd_ref(x, w1, b1, w2, b2, dy, A=False):
    """dz = <dy, x> g (1 - g); da = dz w2 [a > 0]; dx = dy g + W1^T da; dw1 = sum da (x) x, db1 = sum da,
    dw2 = sum dz a, db2 = sum dz (sums over all pixels)"""
    f = pa_fwd_ref(x, w1, b1, w2, b2)
    mask = (f["a"] > 0).double()
    ab = _ab(A)
    x, w1, w2, dy = ab(_d(x)), ab(_d(w1)), ab(_d(w2)), ab(_d(dy))
    g, a = f["g"], f["a"]
    dot = (dy * x).sum(1)
    dz = dot * g * _one_minus(g, A)
    da = dz[:, None] * w2[None, :] * mask
    dx = dy * g[:, None] + da @ w1
    return dict(dz=dz, dx=dx, dw1=da.T @ x, db1=da.sum(0), dw2=(dz[:, None] * a).sum(0), db2=dz.sum().reshape(1))


# ----------------------------------------------------------------------------- pixel sums, gated residual, L1
def dg_parts(hw):
    """sisr_gate_dg_parts: >= 512 pixels per partial, at most 128 partials"""
    return min(128, max(1, (hw + 511) // 512))


def dg_partial_ref(dy, t, parts):
    """dy, t [B,hw,C] (t None: plain sums) -> [B,parts,C]: partial k sums pixels [k*per, min((k+1)*per, hw)),
    per = ceil(hw / parts)"""
    dy = _d(dy)
    prod = dy * _d(t) if t is not None else dy
    B, hw, C = prod.shape
    per = (hw + parts - 1) // parts
    out = torch.zeros((B, parts, C), dtype=torch.float64, device=prod.device)
    for k in range(parts):
        p0, p1 = k * per, min((k + 1) * per, hw)
        if p0 < p1:
            out[:, k] = prod[:, p0:p1].sum(1)
    return out


def sum_partials_fp32(exact_sum, scale):
    """what sisr_sum_partials must return when the sum itself is exact in fp32: one fp32 multiply fl(S * fl32(scale))"""
    return (exact_sum.float() * torch.tensor(scale, dtype=torch.float32, device=exact_sum.device)).double()


def residual_ref(t, g=None, shift=None, x=None, A=False):
    """y = t * g[b,c] + shift[b,c] + x;  t, x [B,hw,C]; g, shift [B,C]"""
    ab = _ab(A)
    y = ab(_d(t))
    if g is not None:
        y = y * ab(_d(g))[:, None, :]
    if shift is not None:
        y = y + ab(_d(shift))[:, None, :]
    if x is not None:
        y = y + ab(_d(x))
    return y


def l1_ref(a, b):
    """mean |a - b| and its gradient sign(a - b) / n (sign(0) = 0), float64"""
    d = _d(a) - _d(b)
    n = d.numel()
    return d.abs().sum() / n, torch.sign(d) / n
