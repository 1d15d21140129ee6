"""Multi-scale SSIM testing (helper module, not collected; torch only, no HIP import).

The oracle: MS-SSIM of two (B, C, H, W) batches in the operands' dtype -- float64 for the references, float32 for the
stock-torch yardstick -- from _ssim_loss.window_maps on every scale and F.avg_pool2d(t, 2) between them, with the semantics
of ops.ms_ssim_mean: every plane alone, no clipping, c_j = mean over windows of A2 / B2 (of S at the last scale),
MS = prod_j max(c_j, 0)^w_j.  Beside it the criterion restatement, the analytic gradient the kernels implement and the cases.
"""
import torch
import torch.nn.functional as F

import _ssim_loss as S

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)  # Wang et al. 2003, as given


def scale_means(x, y, levels, data_range=1.0):
    """[c_0 .. c_{levels-1}], each (B, C): the per-plane means of the contrast-structure map, of S at the last scale"""
    out = []
    for j in range(levels):
        if j:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        mx, my, exx, eyy, exy, c1, c2 = S.window_maps(x, y, data_range)
        vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
        a2, b2 = 2 * vxy + c2, vx + vy + c2
        if j == levels - 1:
            a1, b1 = 2 * mx * my + c1, mx * mx + my * my + c1
            out.append(((a1 * a2) / (b1 * b2)).mean(dim=(2, 3)))
        else:
            out.append((a2 / b2).mean(dim=(2, 3)))
    return out


def ms_ssim(x, y, weights=WEIGHTS, data_range=1.0):
    """the oracle -> (per-plane values (B, C), their mean), in the operands' dtype"""
    per = None
    for c, w in zip(scale_means(x, y, len(weights), data_range), weights):
        t = c.clamp(min=0) ** w
        per = t if per is None else per * t
    return per, per.mean()


def criterion(sr, y, base, alpha, weights=WEIGHTS, data_range=1.0):
    """base(sr, y) + alpha * (1 - MS-SSIM(sr, y)) in sr's dtype; base: 'l1' or 'mse'"""
    pix = (sr - y).abs().mean() if base == "l1" else ((sr - y) ** 2).mean()
    return pix + alpha * (1 - ms_ssim(sr, y, weights, data_range)[1])


def analytic_grad(x, y, weights=WEIGHTS, data_range=1.0):
    """d mean(MS) / d x by the formula the kernels implement.  On scale j, with the window maps of that scale,
         cs = A2 / B2:  beta = -cs / B2, gamma = 2 / B2, alpha = -my gamma - 2 mx beta     (j < M - 1)
         S:             beta, gamma, alpha of _ssim_loss.analytic_grad                      (j = M - 1)
         g_j = G^T alpha + 2 x_j G^T beta + y_j G^T gamma
         D_j = w_j MS / (c_j windows_j planes) g_j + (1/4) D_{j+1}[parent pixel]
       coarsest scale first; the pixels of a dropped odd row or column have no parent; a plane with a c_j <= 0 gets zero."""
    levels = len(weights)
    w = S.taps(x.dtype, x.device)
    planes = x.shape[0] * x.shape[1]
    xs, ys, gs, cs = [x], [y], [], []
    for j in range(levels):
        if j:
            xs.append(F.avg_pool2d(xs[-1], 2))
            ys.append(F.avg_pool2d(ys[-1], 2))
        xj, yj = xs[j], ys[j]
        mx, my, exx, eyy, exy, c1, c2 = S.window_maps(xj, yj, data_range)
        vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
        a2, b2 = 2 * vxy + c2, vx + vy + c2
        if j == levels - 1:
            a1, b1 = 2 * mx * my + c1, mx * mx + my * my + c1
            f = (a1 * a2) / (b1 * b2)
            beta = -f / b2
            gamma = 2 * a1 / (b1 * b2)
            alpha = 2 * my * a2 / (b1 * b2) - 2 * mx * f / b1 - my * gamma - 2 * mx * beta
        else:
            f = a2 / b2
            beta = -f / b2
            gamma = 2 / b2
            alpha = -my * gamma - 2 * mx * beta
        hw = xj.shape[2:]
        gs.append(S._gauss_t(alpha, w, hw) + 2 * xj * S._gauss_t(beta, w, hw) + yj * S._gauss_t(gamma, w, hw))
        cs.append(f.mean(dim=(2, 3)))
    dead = torch.stack([c <= 0 for c in cs]).any(0)
    ms = torch.stack([c.clamp(min=0) ** wj for c, wj in zip(cs, weights)]).prod(0)
    d = None
    for j in reversed(range(levels)):
        windows = (xs[j].shape[2] - 2 * S.RADIUS) * (xs[j].shape[3] - 2 * S.RADIUS)
        fac = torch.where(dead, torch.zeros_like(ms), weights[j] * ms / (cs[j] * windows * planes))
        t = fac[:, :, None, None] * gs[j]
        if d is not None:
            up = d.repeat_interleave(2, 2).repeat_interleave(2, 3) * 0.25
            t[:, :, :up.shape[2], :up.shape[3]] += up
        d = t
    return d


def autograd_grad(x, y, weights=WEIGHTS, data_range=1.0, scale=1.0):
    """(per-plane values, value, d (scale * value) / d x) of the oracle by autograd, in x's dtype"""
    x = x.detach().clone().requires_grad_(True)
    per, v = ms_ssim(x, y, weights, data_range)
    (g,) = torch.autograd.grad(scale * v, x)
    return per.detach(), v.detach(), g


# (shape, scales, noise): the smallest shapes at which the pyramid and the tiling can go wrong
CASES = [((2, 1, 22, 23), 2, 0.05),      # the coarse scale is one window; the odd width drops a column
         ((1, 3, 44, 87), 3, 0.05),      # odd width at two successive scales (87 -> 43 -> 21); one window row at the last
         ((1, 1, 176, 176), 5, 0.05),    # the smallest five-scale image; the last scale is a single window
         ((2, 3, 183, 201), 5, 0.05),    # odd sides at several scales; 173 x 191 windows: several tiles per plane
         ((2, 3, 183, 201), 5, 0.002)]   # near convergence
CASE_IDS = ["%dx%dx%dx%d-%d-%g" % (s + (m, n)) for s, m, n in CASES]


def checker_pair(shape=(1, 1, 22, 22), amplitude=0.2):
    """(sr, y), float32: a smooth ramp plus / minus a one-pixel checkerboard.  On scale 0 the two are anti-correlated
    (covariance about -amplitude^2, c_0 < 0); a 2 x 2 mean removes the checkerboard, so from scale 1 on they are the same
    ramp and c_j = 1.  With weights (0, 1) the plain product max(c_0, 0)^0 * c_1 would be 1 (the oracle above gives that,
    0^0 = 1); the operator, the kernel and metrics.ms_ssim give 0, because a c_j <= 0 zeroes the plane whatever w_j is."""
    b, c, h, w = shape
    i, j = torch.arange(h, dtype=torch.float64)[:, None], torch.arange(w, dtype=torch.float64)[None, :]
    ramp = 0.4 + 0.2 * (i + j) / (h + w)
    sign = 1.0 - 2.0 * ((i + j) % 2)
    y = (ramp + amplitude * sign).float().expand(b, c, h, w).contiguous()
    sr = (ramp - amplitude * sign).float().expand(b, c, h, w).contiguous()
    return sr, y


def make_case(case):
    """(sr, y, weights) of a case: fp32 on the host, the first `scales` of WEIGHTS"""
    shape, levels, noise = case
    sr, y = S.make_pair(shape, noise)
    return sr, y, WEIGHTS[:levels]
