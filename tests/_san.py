"""Float64 references of SAN's second-order channel attention kernels (csrc/san.hip: covariance pooling, Newton-Schulz
square root forward / backward, the SOCA input gradient, the streaming non-local attention) and of the kernels around the
attention (csrc/nonlocal.hip: the 64 -> 24 projection and its gradients, split / 2x2 max pool and its scatter, the 8 -> 64
output projection and its backward).  Helper module, not collected; torch only, no HIP import.

Every function takes the kernels' own layout -- x [B][M][64] and mean [B][64] (covariance), cov [B][64][64], attention rows
[nb][n][8], maps flattened to [npix][64] / [npix][24], and the 9-int `domains` record (B, H, W, y0, x0, hq, wq, nqy, nqx) of
the sisr_nl_* entry points -- and evaluates the textbook formula in `dt` (float64; float32 gives the same formula's fp32
evaluation, which the chain tier of tests/test_san_kernels_gpu.py measures its bar with).  tests/test_san_cpu.py checks
each against float64 autograd of the oracle or of PyTorch.

As in tests/_spar_han.py, references used in bounded comparisons take a flag `A`: True evaluates the same computation on
absolute values with every subtraction turned into an addition, the magnitude each fp32 rounding of the kernel is relative
to, so a bound reads |got - ref| <= c * 2^-24 * mag.
"""
import torch

F64 = torch.float64


def _c(t, dt=F64):
    return None if t is None else t.detach().to(dt)


def _sub(a, b, A):
    return a + b if A else a - b


# ----------------------------------------------------------------------------- covariance pooling
def covpool_ref(x, mean, A=False, dt=F64):
    """x [B][M][64], mean [B][64] (as given: the kernel takes it as an argument) ->
    cov[b][i][j] = (1 / M) sum_p (x[b][p][i] - mean[b][i]) x[b][p][j]"""
    x, mean = _c(x, dt), _c(mean, dt)
    if A:
        x, mean = x.abs(), mean.abs()
    return torch.einsum("bpi,bpj->bij", _sub(x, mean[:, None, :], A), x) / x.shape[1]


def covpool_sum_ref(x, mean, dt=F64):
    """the un-scaled sum of covpool_ref (what the slab partials add up to before the one multiplication by fl32(1 / M))"""
    x, mean = _c(x, dt), _c(mean, dt)
    return torch.einsum("bpi,bpj->bij", x - mean[:, None, :], x)


# ----------------------------------------------------------------------------- Newton-Schulz square root
def _eye3(a):
    return 3.0 * torch.eye(a.shape[-1], dtype=a.dtype, device=a.device)


def sqrtm_fwd_ref(cov, iters, dt=F64):
    """cov [B][64][64] -> trace [B]; A = cov / trace; Z_0 = (3I - A) / 2, Y_0 = A Z_0; for i = 1 .. iters - 2:
    T = (3I - Z Y) / 2, Y_i = Y T, Z_i = T Z; last = Y (3I - Z Y) / 2; pooled[b][j] = mean_i sqrt(trace) last[i][j].
    Y, Z: [B][iters - 1][64][64] (the kernel's saved iterates)."""
    a = _c(cov, dt)
    I3 = _eye3(a)
    tr = a.diagonal(dim1=1, dim2=2).sum(1)
    an = a / tr[:, None, None]
    zy = 0.5 * (I3 - an)
    ys, zs = [an @ zy], [zy]
    for _ in range(1, iters - 1):
        zy = 0.5 * (I3 - zs[-1] @ ys[-1])
        ys.append(ys[-1] @ zy)
        zs.append(zy @ zs[-1])
    last = 0.5 * (ys[-1] @ (I3 - zs[-1] @ ys[-1]))
    pooled = (last * tr.sqrt()[:, None, None]).mean(1)
    return dict(trace=tr, Y=torch.stack(ys, 1), Z=torch.stack(zs, 1), last=last, pooled=pooled)


def sqrtm_bwd_ref(cov, iters, dpooled, dt=F64):
    """the gradient G of sum(pooled * dpooled) with respect to cov by the hand-derived recurrences of the reference
    (every entry of cov independent), returned as G + G^T [B][64][64], the form the covariance backward consumes"""
    f = sqrtm_fwd_ref(cov, iters, dt)
    a, tr, ys, zs, last = _c(cov, dt), f["trace"], f["Y"], f["Z"], f["last"]
    B, d, _ = a.shape
    I3 = _eye3(a)
    an = a / tr[:, None, None]
    rt = tr.sqrt()
    g = (_c(dpooled, dt) / d)[:, None, :].expand(B, d, d)
    gp = g * rt[:, None, None]
    aux = (g * last).sum(dim=(1, 2)) / (2.0 * rt)
    k = ys.shape[1] - 1
    yk, zk = ys[:, k], zs[:, k]
    dy = 0.5 * (gp @ (I3 - yk @ zk) - zk @ yk @ gp)
    dz = -0.5 * (yk @ gp @ yk)
    for i in range(k - 1, -1, -1):
        yi, zi = ys[:, i], zs[:, i]
        yz = I3 - yi @ zi
        zyi = zi @ yi
        dy, dz = (0.5 * (dy @ yz - zi @ dz @ zi - zyi @ dy), 0.5 * (yz @ dz - yi @ dy @ yi - dz @ zyi))
    dn = 0.5 * (dy @ (I3 - an) - dz - an @ dy)
    diag = aux - (dn * a).sum(dim=(1, 2)) / (tr * tr)
    G = dn / tr[:, None, None] + diag[:, None, None] * torch.eye(d, dtype=a.dtype, device=a.device)
    return G + G.transpose(1, 2)


# ----------------------------------------------------------------------------- SOCA input gradient
def soca_bwd_apply_ref(dy, gate, x, mean, dsym, A=False, dt=F64):
    """dx[b][p][c] = dy[b][p][c] gate[b][c] + (1 / M) sum_c' dsym[b][c][c'] (x[b][p][c'] - mean[b][c'])"""
    dy, gate, x, mean, dsym = (_c(t, dt) for t in (dy, gate, x, mean, dsym))
    if A:
        dy, gate, x, mean, dsym = dy.abs(), gate.abs(), x.abs(), mean.abs(), dsym.abs()
    M = x.shape[1]
    return dy * gate[:, None, :] + torch.einsum("bck,bpk->bpc", dsym, _sub(x, mean[:, None, :], A)) / M


# ----------------------------------------------------------------------------- non-local attention
def attn_fwd_ref(theta, phi, g, dt=F64):
    """theta [nb][nq][8], phi / g [nb][nk][8] -> y = softmax_j(theta . phi_j) g, lse = log sum_j exp(theta . phi_j)"""
    theta, phi, g = _c(theta, dt), _c(phi, dt), _c(g, dt)
    s = theta @ phi.transpose(1, 2)
    lse = torch.logsumexp(s, dim=-1)
    return dict(y=torch.exp(s - lse[..., None]) @ g, lse=lse)


def attn_bwd_ref(theta, phi, g, dy, dt=F64):
    """p = softmax, dsum_i = dy_i . y_i, ds_ij = p_ij (dy_i . g_j - dsum_i), dtheta = ds phi, dphi = ds^T theta,
    dg = p^T dy"""
    theta, phi, g, dy = _c(theta, dt), _c(phi, dt), _c(g, dt), _c(dy, dt)
    s = theta @ phi.transpose(1, 2)
    p = torch.exp(s - torch.logsumexp(s, dim=-1, keepdim=True))
    y = p @ g
    dsum = (dy * y).sum(-1)
    ds = p * (dy @ g.transpose(1, 2) - dsum[..., None])
    return dict(dtheta=ds @ phi, dphi=ds.transpose(1, 2) @ theta, dg=p.transpose(1, 2) @ dy, dsum=dsum)


# ----------------------------------------------------------------------------- projections 64 -> 24 (theta | phi | g)
def _wp(w_theta, w_phi, w_g, dt):
    return torch.cat([_c(w_theta, dt), _c(w_phi, dt), _c(w_g, dt)], 0)


def project_fwd_ref(x, w_theta, b_theta, w_phi, b_phi, w_g, b_g, A=False, dt=F64):
    """x [npix][64], w_* [8][64], b_* [8] -> proj [npix][24] = x Wp^T + bp"""
    x, W, b = _c(x, dt), _wp(w_theta, w_phi, w_g, dt), torch.cat([_c(b_theta, dt), _c(b_phi, dt), _c(b_g, dt)])
    if A:
        x, W, b = x.abs(), W.abs(), b.abs()
    return x @ W.t() + b


def project_dgrad_ref(dproj, dz, w_theta, w_phi, w_g, A=False, dt=F64):
    """dx [npix][64] = dproj Wp + dz (the skip)"""
    dproj, dz, W = _c(dproj, dt), _c(dz, dt), _wp(w_theta, w_phi, w_g, dt)
    if A:
        dproj, dz, W = dproj.abs(), dz.abs(), W.abs()
    return dproj @ W + dz


def project_wgrad_ref(x, dproj, A=False, dt=F64):
    """dWp [24][64] = dproj^T x, db [24] = sum_p dproj (the partial rows summed)"""
    x, dproj = _c(x, dt), _c(dproj, dt)
    if A:
        x, dproj = x.abs(), dproj.abs()
    return dict(dW=dproj.t() @ x, db=dproj.sum(0))


# ----------------------------------------------------------------------------- attention domains
def domain_pixels(dom):
    """dom = (B, H, W, y0, x0, hq, wq, nqy, nqx) -> LongTensor [B * nqy * nqx][hq][wq] of flat pixel indices
    (b H + y) W + x; domain (b, iy, ix) is the rectangle at (y0 + iy hq, x0 + ix wq), domains ordered b, iy, ix"""
    B, H, W, y0, x0, hq, wq, nqy, nqx = (int(v) for v in dom)
    b = torch.arange(B).view(B, 1, 1, 1, 1)
    yy = (y0 + torch.arange(nqy).view(1, nqy, 1, 1, 1) * hq + torch.arange(hq).view(1, 1, 1, hq, 1))
    xx = (x0 + torch.arange(nqx).view(1, 1, nqx, 1, 1) * wq + torch.arange(wq).view(1, 1, 1, 1, wq))
    return ((b * H + yy) * W + xx).reshape(B * nqy * nqx, hq, wq)


def _windows(v, hq, wq):
    """[nd][hq][wq][C] -> [nd][hp][wp][4][C], the floor-mode 2x2 windows, members in scan order (0,0) (0,1) (1,0) (1,1)"""
    nd, C = v.shape[0], v.shape[-1]
    hp, wp = hq // 2, wq // 2
    w = v[:, :2 * hp, :2 * wp].reshape(nd, hp, 2, wp, 2, C)
    return w.permute(0, 1, 3, 2, 4, 5).reshape(nd, hp, wp, 4, C)


def _first_max(win):
    """[..., 4, C] -> (max, index of the first member in scan order that attains it): a later member replaces the running
    maximum only when strictly greater, so +0 and -0 tie"""
    m, arg = win[..., 0, :], torch.zeros(win.shape[:-2] + win.shape[-1:], dtype=torch.long, device=win.device)
    for s in range(1, 4):
        v = win[..., s, :]
        better = v > m
        m = torch.where(better, v, m)
        arg = torch.where(better, torch.full_like(arg, s), arg)
    return m, arg


def split_pool_fwd_ref(proj, dom, dt=F64):
    """proj [npix][24] -> theta [nd][hq wq][8] (channels 0..7 of every position), phi / g [nd][hp wp][8] (channels 8..15 /
    16..23 max-pooled 2x2, floor mode)"""
    proj = _c(proj, dt)
    hq, wq = int(dom[5]), int(dom[6])
    pix = domain_pixels(dom).to(proj.device)
    nd = pix.shape[0]
    v = proj[pix.reshape(-1)].view(nd, hq, wq, 24)
    m, _ = _first_max(_windows(v[..., 8:], hq, wq))
    m = m.reshape(nd, -1, 16)
    return dict(theta=v[..., :8].reshape(nd, hq * wq, 8), phi=m[..., :8], g=m[..., 8:])


def split_pool_bwd_ref(proj, dtheta, dphi, dg, dom, npix, fill=float("nan"), dt=F64):
    """-> dproj [npix][24]: at every pixel of the domains channels 0..7 = dtheta, channels 8..23 = the window's dphi | dg at
    the window's first maximum in scan order and 0 elsewhere (leftover rows / columns of odd domains included); pixels
    outside the domains keep `fill`"""
    proj, dtheta, dphi, dg = _c(proj, dt), _c(dtheta, dt), _c(dphi, dt), _c(dg, dt)
    hq, wq = int(dom[5]), int(dom[6])
    hp, wp = hq // 2, wq // 2
    pix = domain_pixels(dom).to(proj.device)
    nd = pix.shape[0]
    v = proj[pix.reshape(-1)].view(nd, hq, wq, 24)
    _, arg = _first_max(_windows(v[..., 8:], hq, wq))
    gsrc = torch.cat([dphi, dg], -1).view(nd, hp, wp, 1, 16)
    member = torch.arange(4, device=proj.device).view(1, 1, 1, 4, 1)
    routed = torch.where(arg[..., None, :] == member, gsrc.expand(nd, hp, wp, 4, 16), torch.zeros((), dtype=dt, device=proj.device))
    pooled = torch.zeros((nd, hq, wq, 16), dtype=dt, device=proj.device)
    pooled[:, :2 * hp, :2 * wp] = routed.view(nd, hp, wp, 2, 2, 16).permute(0, 1, 3, 2, 4, 5).reshape(nd, 2 * hp, 2 * wp, 16)
    out = torch.full((npix, 24), fill, dtype=dt, device=proj.device)
    out[pix.reshape(-1)] = torch.cat([dtheta.view(nd, hq, wq, 8), pooled], -1).view(-1, 24)
    return out


# ----------------------------------------------------------------------------- output projection 8 -> 64 + skip
def output_fwd_ref(y, x, w, bias, dom, A=False, fill=float("nan"), dt=F64):
    """y [rows][8] (rows = the domains' positions in order), x [npix][64], w [64][8], bias [64] ->
    z [npix][64]: z[p] = y[r] W^T + bias + x[p] at the domains' pixels, `fill` elsewhere"""
    y, x, w, bias = _c(y, dt), _c(x, dt), _c(w, dt), _c(bias, dt)
    if A:
        y, x, w, bias = y.abs(), x.abs(), w.abs(), bias.abs()
    pix = domain_pixels(dom).reshape(-1).to(x.device)
    z = torch.full_like(x, fill)
    z[pix] = y.reshape(-1, 8) @ w.t() + bias + x[pix]
    return z


def output_bwd_ref(dz, y, w, dom, A=False, dt=F64):
    """dy (shaped like y) = dz[p] W, dW [64][8] = sum_r dz[p]^T y[r], db [64] = sum_r dz[p] over the domains' pixels"""
    shape = y.shape
    dz, y, w = _c(dz, dt), _c(y, dt).reshape(-1, 8), _c(w, dt)
    if A:
        dz, y, w = dz.abs(), y.abs(), w.abs()
    d = dz[domain_pixels(dom).reshape(-1).to(dz.device)]
    return dict(dy=(d @ w).view(shape), dW=d.t() @ y, db=d.sum(0))


# ----------------------------------------------------------------------------- seeded data
def tie_values(shape, seed):
    """values in {-1, -0, +0, 1}: over a 2x2 window the maximum is attained by 1 .. 4 members, +0 and -0 among them"""
    g = torch.Generator().manual_seed(int(seed))
    t = torch.randint(-1, 2, tuple(shape), generator=g).float()
    neg = torch.rand(tuple(shape), generator=g) < 0.5
    return torch.where((t == 0) & neg, torch.tensor(-0.0), t)


def tie_census(proj, dom):
    """how many 2x2 windows of channels 8..23 attain their maximum 1, 2, 3, 4 times, and how many of the tied ones tie a +0
    with a -0 -> ([n1, n2, n3, n4], n_signed_zero)"""
    hq, wq = int(dom[5]), int(dom[6])
    pix = domain_pixels(dom)
    v = proj.detach().cpu()[pix.reshape(-1)].view(pix.shape[0], hq, wq, 24)[..., 8:]
    win = _windows(v, hq, wq)
    top = win == win.max(dim=-2, keepdim=True)[0]
    mult = top.sum(-2)
    sign = torch.signbit(win) & top
    mixed = (sign.any(-2) & (~torch.signbit(win) & top).any(-2))
    return [int((mult == k).sum()) for k in (1, 2, 3, 4)], int(mixed.sum())


def correlated_maps(B, M, r, noise, seed):
    """x [B][M][64]: a 64 x r mix of r Gaussian sources plus `noise` (relative) white noise; r = None: isotropic"""
    g = torch.Generator().manual_seed(int(seed))
    if r is None:
        return torch.randn(B, M, 64, generator=g)
    src, mix = torch.randn(B, M, r, generator=g), torch.randn(B, r, 64, generator=g)
    return src @ mix + noise * (r ** 0.5) * torch.randn(B, M, 64, generator=g)
