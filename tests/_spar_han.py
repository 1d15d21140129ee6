"""Float64 references of the SPARNet norm / activation / attention-product / geometry kernels and of HAN's LAM and CSAM
(helper module, not collected; torch only, no HIP import).

Every function takes the kernels' own layout -- channels-last maps flattened to [pixels][C] (batch norm, pixel norm, the
activations, the attention products), [B][HW][C] (group norm), [B][H][W][C] (geometry, CSAM), [B][N][K] (LAM) -- and
evaluates the textbook formula in float64.  tests/test_spar_han_cpu.py checks each against float64 autograd of its PyTorch
or oracle counterpart; tests/test_spar_han_gpu.py compares the kernels with them.

As in tests/_gates.py, backward references take a flag `A`: True evaluates the same computation on absolute values with
every subtraction turned into an addition.  The result bounds the magnitude each fp32 rounding of the kernel is relative to,
so a bound reads |got - ref| <= c * 2^-24 * mag, c per family (stated next to each GPU test).
"""
import torch

SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SCALE = 1.0507009873554804934193349852946
PN_EPS = 1e-12


def _d(t):
    return None if t is None else t.detach().double()


def _f(v):
    return float(v.detach()) if torch.is_tensor(v) else float(v)


def _sub(a, b, A):
    return a + b if A else a - b


# ----------------------------------------------------------------------------- batch norm (+ LeakyReLU)
def bn_fwd_ref(x, gamma, beta, eps, slope, running_mean=None, running_var=None, momentum=0.1, training=True):
    """x [npix][C] -> mean, var (biased), invstd, z = xhat * gamma + beta, y = LeakyReLU(slope)(z), and in training mode the
    updated running statistics rm = (1 - m) rm + m mean, rv = (1 - m) rv + m var n / (n - 1)"""
    x, gamma, beta, rm, rv = map(_d, (x, gamma, beta, running_mean, running_var))
    n = x.shape[0]
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
    else:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    z = (x - mean) * invstd * gamma + beta
    out = dict(mean=mean, var=var, invstd=invstd, z=z, y=torch.where(z > 0, z, z * slope))
    if training and rm is not None:
        out["rm"] = (1 - momentum) * rm + momentum * mean
        out["rv"] = (1 - momentum) * rv + momentum * var * (n / (n - 1) if n > 1 else 1.0)
    return out


def bn_bwd_ref(x, dy, gamma, beta, mean, invstd, slope, A=False):
    """the batch-norm + LeakyReLU backward at given statistics: dz = dy * act'(z) (1 where z > 0, slope where z <= 0, z the
    forward pre-activation), xhat = (x - mean) invstd, dbeta = sum dz, dgamma = sum dz xhat,
    dx = gamma invstd (dz - dbeta / n - xhat dgamma / n)"""
    x, dy, gamma, beta, mean, invstd = map(_d, (x, dy, gamma, beta, mean, invstd))
    n = x.shape[0]
    z = (x - mean) * invstd * gamma + beta
    dz = dy * torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    if A:
        dz, xh, gamma = dz.abs(), (x.abs() + mean.abs()) * invstd, gamma.abs()
    else:
        xh = (x - mean) * invstd
    db, dg = dz.sum(0), (dz * xh).sum(0)
    dx = gamma * invstd * _sub(_sub(dz, db / n, A), xh * dg / n, A)
    return dict(dz=dz, xhat=xh, dbeta=db, dgamma=dg, dx=dx)


# ----------------------------------------------------------------------------- group / instance norm
def gn_fwd_ref(x, gamma, beta, cg, eps):
    """x [B][HW][C] (C real channels, a multiple of cg) -> mean, invstd [B][C / cg] (two-pass, biased), y"""
    x, gamma, beta = map(_d, (x, gamma, beta))
    B, hw, C = x.shape
    xg = x.view(B, hw, C // cg, cg)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    invstd = 1.0 / torch.sqrt(var + eps)
    xh = ((xg - mean[:, None, :, None]) * invstd[:, None, :, None]).view(B, hw, C)
    return dict(mean=mean, var=var, invstd=invstd, y=xh * gamma + beta)


def gn_bwd_ref(x, dy, gamma, mean, invstd, cg, A=False):
    """dxhat = dy gamma; dx = invstd (dxhat - mean_g(dxhat) - xhat mean_g(dxhat xhat)); per-sample parameter partials
    dgamma_b[b][c] = sum_hw dy xhat, dbeta_b[b][c] = sum_hw dy"""
    x, dy, gamma, mean, invstd = map(_d, (x, dy, gamma, mean, invstd))
    B, hw, C = x.shape
    G = C // cg
    m = mean.repeat_interleave(cg, dim=1)[:, None, :]
    iv = invstd.repeat_interleave(cg, dim=1)[:, None, :]
    if A:
        dy, gamma, xh = dy.abs(), gamma.abs(), (x.abs() + m.abs()) * iv
    else:
        xh = (x - m) * iv
    dh = dy * gamma
    s1 = dh.view(B, hw, G, cg).mean(dim=(1, 3)).repeat_interleave(cg, dim=1)[:, None, :]
    s2 = (dh * xh).view(B, hw, G, cg).mean(dim=(1, 3)).repeat_interleave(cg, dim=1)[:, None, :]
    dx = iv * _sub(_sub(dh, s1, A), xh * s2, A)
    return dict(dx=dx, dgamma_b=(dy * xh).sum(1), dbeta_b=dy.sum(1))


# ----------------------------------------------------------------------------- pixel norm (F.normalize(p=2, dim=channels))
def pn_fwd_ref(x):
    """x [npix][C] -> norm, den = max(norm, 1e-12), y = x / den"""
    x = _d(x)
    nrm = torch.sqrt((x * x).sum(1, keepdim=True))
    den = torch.clamp(nrm, min=PN_EPS)
    return dict(norm=nrm, den=den, y=x / den)


def pn_bwd_ref(x, dy, A=False):
    """dx = (dy - y <dy, y>) / den where norm > eps, dy / eps where it is not (the clamp passes no gradient)"""
    f = pn_fwd_ref(x)
    dy, y, den = _d(dy), f["y"], f["den"]
    if A:
        dy, y = dy.abs(), y.abs()
    dot = (dy * y).sum(1, keepdim=True)
    return torch.where(f["norm"] > PN_EPS, _sub(dy, y * dot, A) / den, dy / den)


# ----------------------------------------------------------------------------- PReLU / SELU
def prelu_ref(x, a):
    """x [npix][C], a [C] (one slope per channel) -> y = x > 0 ? x : a x"""
    x, a = _d(x), _d(a)
    return torch.where(x > 0, x, a * x)


def prelu_bwd_ref(x, dy, a):
    """dx = x > 0 ? dy : a dy;  dyx = dy min(x, 0) (exactly 0 where x > 0);  da = sum over pixels of dyx"""
    x, dy, a = _d(x), _d(dy), _d(a)
    dyx = torch.where(x > 0, torch.zeros_like(x), dy * x)
    return dict(dx=torch.where(x > 0, dy, a * dy), dyx=dyx, da=dyx.sum(0))


def selu_ref(x, A=False):
    """scale * (x > 0 ? x : alpha (e^x - 1)); A: the magnitude scale * (x > 0 ? x : alpha |e^x - 1|)"""
    x = _d(x)
    neg = SELU_ALPHA * torch.expm1(x)
    return SELU_SCALE * torch.where(x > 0, x, neg.abs() if A else neg)


def selu_bwd_ref(x, dy):
    x, dy = _d(x), _d(dy)
    return dy * SELU_SCALE * torch.where(x > 0, torch.ones_like(x), SELU_ALPHA * torch.exp(x))


# ----------------------------------------------------------------------------- SPARNet attention products
def spar_combine_ref(x, logit, identity=None):
    """x [npix][C], logit [npix] (channel 0 of the attention conv) -> a = sigmoid(logit), y = identity + x a"""
    x, logit, identity = map(_d, (x, logit, identity))
    a = torch.sigmoid(logit)
    y = x * a[:, None]
    return dict(a=a, y=y + identity if identity is not None else y)


def spar_combine_bwd_ref(dy, x, a, A=False):
    """dx = dy a;  dlogit = <dy, x> a (1 - a) (the gradient of every other logit channel is 0)"""
    dy, x, a = map(_d, (dy, x, a))
    if A:
        dy, x = dy.abs(), x.abs()
    dot = (dy * x).sum(1)
    return dict(dx=dy * a[:, None], dlogit=dot * a * _sub(1, a, A))


def spar3d_ref(x, logits, identity=None):
    """one logit per element: a = sigmoid(logits), y = identity + x a"""
    x, logits, identity = map(_d, (x, logits, identity))
    a = torch.sigmoid(logits)
    return dict(a=a, y=x * a + identity if identity is not None else x * a)


def spar3d_bwd_ref(dy, x, logits, A=False):
    """dx = dy a, dlogits = dy x a (1 - a)"""
    dy, x, logits = map(_d, (dy, x, logits))
    a = torch.sigmoid(logits)
    if A:
        dy, x = dy.abs(), x.abs()
    return dict(dx=dy * a, dlogits=dy * x * a * _sub(1, a, A))


# ----------------------------------------------------------------------------- geometry ([B][H][W][C] maps)
def _reflect_src(n, up):
    """source row of each of the up * n + 2 rows of [nearest x up] -> ReflectionPad2d(1): padded row i reads upsampled row
    |i - 1| reflected at both ends, i.e. source row (that) // up"""
    nu = n * up
    src = []
    for i in range(nu + 2):
        u = abs(i - 1)
        if u >= nu:
            u = 2 * nu - 2 - u
        src.append(u // up)
    return torch.tensor(src, dtype=torch.long)


def pad_reflect_up_ref(x, up):
    """(B, H, W, C) -> (B, up H + 2, up W + 2, C): gather by the source-row / source-column maps"""
    x = _d(x)
    r, c = _reflect_src(x.shape[1], up).to(x.device), _reflect_src(x.shape[2], up).to(x.device)
    return x[:, r][:, :, c]


def pad_reflect_up_adj(dy, H, W, up):
    """adjoint: every padded position's gradient added onto the source pixel it reads"""
    dy = _d(dy)
    r, c = _reflect_src(H, up).to(dy.device), _reflect_src(W, up).to(dy.device)
    B, Hp, Wp, C = dy.shape
    rows = torch.zeros((B, H, Wp, C), dtype=torch.float64, device=dy.device).index_add_(1, r, dy)
    return torch.zeros((B, H, W, C), dtype=torch.float64, device=dy.device).index_add_(2, c, rows)


def crop_stride_ref(src, stride):
    """(B, Hf, Wf, C) -> (B, Ho, Wo, C), Ho = (Hf - 3) // stride + 1: y[h][w] = src[1 + stride h][1 + stride w]"""
    src = _d(src)
    Ho, Wo = (src.shape[1] - 3) // stride + 1, (src.shape[2] - 3) // stride + 1
    return src[:, 1:1 + stride * (Ho - 1) + 1:stride, 1:1 + stride * (Wo - 1) + 1:stride]


def crop_stride_adj(y, Hf, Wf, stride):
    """adjoint (the embed): a zero (B, Hf, Wf, C) map holding y at the cropped positions"""
    y = _d(y)
    out = torch.zeros((y.shape[0], Hf, Wf, y.shape[3]), dtype=torch.float64, device=y.device)
    Ho, Wo = y.shape[1], y.shape[2]
    out[:, 1:1 + stride * (Ho - 1) + 1:stride, 1:1 + stride * (Wo - 1) + 1:stride] = y
    return out


def nearest_up_ref(x, up):
    x = _d(x)
    return x.repeat_interleave(up, dim=1).repeat_interleave(up, dim=2)


def nearest_up_adj(dy, up):
    """adjoint: the sum of each up x up block"""
    dy = _d(dy)
    B, Ho, Wo, C = dy.shape
    return dy.view(B, Ho // up, up, Wo // up, up, C).sum(dim=(2, 4))


# ----------------------------------------------------------------------------- LAM (layer attention)
def lam_fwd_ref(X, gamma):
    """X [B][N][K] -> E = X X^T, A = softmax_j(max_j E_ij - E_ij), y = gamma A X + X"""
    X, gamma = _d(X), _f(gamma)
    E = X @ X.transpose(1, 2)
    A = torch.softmax(E.max(dim=-1, keepdim=True)[0] - E, dim=-1)
    return dict(E=E, A=A, y=gamma * (A @ X) + X)


def lam_bwd_ref(X, Att, gamma, dO, A=False):
    """at a given attention A (row-stochastic, the forward's): G = dO X^T, dgamma = sum A G, dA = gamma G,
    dE = -A (dA - rowsum(dA A)) (the row-max term cancels: softmax rows sum to 1), dX = (I + gamma A^T) dO + (dE + dE^T) X.
    A=True: the same on |dO|, |X|, |gamma| with dE = A |gamma| (|G| + rowsum(|G| A))"""
    X, Att, dO, g = _d(X), _d(Att), _d(dO), _f(gamma)
    if A:
        X, dO, g = X.abs(), dO.abs(), abs(g)
    G = dO @ X.transpose(1, 2)
    rowdot = (G * Att).sum(-1, keepdim=True)
    dgamma = (G * Att).sum()
    dE = Att * g * (G + rowdot) if A else -(Att * g * (G - rowdot))
    eye = torch.eye(X.shape[1], dtype=torch.float64, device=X.device)
    C1 = g * Att.transpose(1, 2) + eye
    C2 = dE + dE.transpose(1, 2)
    return dict(G=G, dE=dE, dgamma=dgamma, dx=C1 @ dO + C2 @ X)


# ----------------------------------------------------------------------------- CSAM (channel-spatial attention)
def _shift3(v, dc, dh, dw):
    """v [B][H][W][C] zero-padded by one in C, H, W, read at offset (dc, dh, dw) in {0, 1, 2}^3: v[c + dc - 1][h + dh - 1]..."""
    B, H, W, C = v.shape
    vp = torch.nn.functional.pad(v, (1, 1, 1, 1, 1, 1))
    return vp[:, dh:dh + H, dw:dw + W, dc:dc + C]


def csam_conv(v, w):
    """Conv3d(1 -> 1, k 3, pad 1) over the (C, H, W) volume of each sample, w [3][3][3] = [dc][dh][dw], no bias"""
    v, w = _d(v), _d(w).view(3, 3, 3)
    out = torch.zeros_like(v)
    for dc in range(3):
        for dh in range(3):
            for dw in range(3):
                out = out + w[dc, dh, dw] * _shift3(v, dc, dh, dw)
    return out


def csam_conv_t(v, w):
    """the adjoint of csam_conv: correlation with the kernel flipped in all three axes"""
    return csam_conv(v, _d(w).view(3, 3, 3).flip(0, 1, 2))


def csam_fwd_ref(x, w, bias, gamma):
    """x [B][H][W][64] -> z = bias + conv3d(x), s = sigmoid(z), y = x (1 + gamma s)"""
    x, bias, gamma = _d(x), _f(bias), _f(gamma)
    z = csam_conv(x, w) + bias
    s = torch.sigmoid(z)
    return dict(z=z, s=s, y=x * (1 + gamma * s))


def csam_bwd_ref(x, w, bias, gamma, dy, A=False):
    """dgamma = sum dy x s;  dz = dy x gamma s (1 - s);  dbias = sum dz;  dw[dc][dh][dw] = sum dz x(shifted);
    dx = dy (1 + gamma s) + conv3d^T(dz)"""
    f = csam_fwd_ref(x, w, bias, gamma)
    s = f["s"]
    x, dy, w, g = _d(x), _d(dy), _d(w).view(3, 3, 3), _f(gamma)
    if A:
        x, dy, w, g = x.abs(), dy.abs(), w.abs(), abs(g)
    dz = dy * x * g * s * _sub(1, s, A)
    dw = torch.stack([(dz * _shift3(x, dc, dh, dw_)).sum() for dc in range(3) for dh in range(3) for dw_ in range(3)])
    dx = dy * (1 + g * s) + csam_conv_t(dz, w)
    return dict(dz=dz, dgamma=(dy * x * s).sum(), dbias=dz.sum(), dw=dw, dx=dx)
