"""Structural (SSIM) loss testing (helper module, not collected; torch only, no HIP import).

The oracle: mean SSIM of two (B, C, H, W) batches by grouped F.conv2d in the operands' dtype -- float64 for the references,
float32 for the stock-torch yardstick -- with the semantics of ops.ssim_mean: every plane alone, no clipping, the 11-tap
Gaussian (sigma 1.5) applied separably, population covariance, the (H - 10) x (W - 10) windows inside the image.  Beside it
the criterion restatement, the analytic gradient the kernels implement, and the input makers.
"""
import math

import torch
import torch.nn.functional as F

RADIUS = 5
WINDOW = 2 * RADIUS + 1


def taps(dtype=torch.float64, device="cpu"):
    """scipy.ndimage's _gaussian_kernel1d(1.5, 0, 5) in float64, then converted (metrics.ssim_taps, restated)"""
    x = torch.arange(-RADIUS, RADIUS + 1, dtype=torch.float64)
    phi = torch.exp(-0.5 / (1.5 * 1.5) * x * x)
    return (phi / phi.sum()).to(device=device, dtype=dtype)


def _gauss(t, w):
    """separable valid correlation of every plane of (B, C, H, W) with the taps: rows, then columns"""
    c = t.shape[1]
    t = F.conv2d(t, w.view(1, 1, WINDOW, 1).expand(c, 1, WINDOW, 1), groups=c)
    return F.conv2d(t, w.view(1, 1, 1, WINDOW).expand(c, 1, 1, WINDOW), groups=c)


def window_maps(x, y, data_range=1.0):
    """mx, my, Exx, Eyy, Exy, C1, C2 on the window grid, in x's dtype"""
    w = taps(x.dtype, x.device)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    return _gauss(x, w), _gauss(y, w), _gauss(x * x, w), _gauss(y * y, w), _gauss(x * y, w), c1, c2


def ssim_map(x, y, data_range=1.0):
    mx, my, exx, eyy, exy, c1, c2 = window_maps(x, y, data_range)
    vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
    a1, a2 = 2 * mx * my + c1, 2 * vxy + c2
    b1, b2 = mx * mx + my * my + c1, vx + vy + c2
    return (a1 * a2) / (b1 * b2)


def ssim_mean(x, y, data_range=1.0):
    """the oracle: mean of S over all windows of all planes, in the operands' dtype"""
    return ssim_map(x, y, data_range).mean()


def criterion(sr, y, base, alpha, data_range=1.0):
    """base(sr, y) + alpha * (1 - SSIM(sr, y)) in sr's dtype; base: 'l1' or 'mse'"""
    pix = (sr - y).abs().mean() if base == "l1" else ((sr - y) ** 2).mean()
    return pix + alpha * (1 - ssim_mean(sr, y, data_range))


def _gauss_t(m, w, hw):
    """the transposed ("full") separable correlation: window grid -> (H, W) pixel grid"""
    c = m.shape[1]
    t = F.conv_transpose2d(m, w.view(1, 1, 1, WINDOW).expand(c, 1, 1, WINDOW), groups=c)
    t = F.conv_transpose2d(t, w.view(1, 1, WINDOW, 1).expand(c, 1, WINDOW, 1), groups=c)
    assert tuple(t.shape[2:]) == tuple(hw)
    return t


def analytic_grad(x, y, data_range=1.0):
    """d ssim_mean / d x by the formula the kernels implement:
         beta = dS/dExx = -S / B2, gamma = dS/dExy = 2 A1 / (B1 B2),
         alpha = dS/dmx = 2 my A2 / (B1 B2) - 2 mx S / B1 - my gamma - 2 mx beta,
         grad = (G^T alpha + 2 x G^T beta + y G^T gamma) / count"""
    mx, my, exx, eyy, exy, c1, c2 = window_maps(x, y, data_range)
    vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
    a1, a2 = 2 * mx * my + c1, 2 * vxy + c2
    b1, b2 = mx * mx + my * my + c1, vx + vy + c2
    s = (a1 * a2) / (b1 * b2)
    beta = -s / b2
    gamma = 2 * a1 / (b1 * b2)
    alpha = 2 * my * a2 / (b1 * b2) - 2 * mx * s / b1 - my * gamma - 2 * mx * beta
    w = taps(x.dtype, x.device)
    hw = x.shape[2:]
    return (_gauss_t(alpha, w, hw) + 2 * x * _gauss_t(beta, w, hw) + y * _gauss_t(gamma, w, hw)) / s.numel()


def autograd_grad(x, y, data_range=1.0, scale=1.0):
    """(value, d (scale * value) / d x) of the oracle by autograd, in x's dtype"""
    x = x.detach().clone().requires_grad_(True)
    v = ssim_mean(x, y, data_range)
    (g,) = torch.autograd.grad(scale * v, x)
    return v.detach(), g


def rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / ref.norm())


# the smallest shapes at which the tiling (64 window columns x 32 window rows per wave; 64 x 32 pixels in the gradient) can
# go wrong, and the noise levels: 0.05 everywhere, 0.002 (near convergence) on the last
SHAPES = [(2, 3, 11, 11),   # one window
          (1, 1, 11, 85),   # one window row, 75 columns: a second column tile of 11, the right-edge clamp
          (2, 1, 42, 74),   # exactly one 32 x 64 tile
          (1, 3, 43, 75)]   # 33 x 65 windows: two row tiles and two column tiles of one, ring wrap-around
CASES = [(s, 0.05) for s in SHAPES] + [(SHAPES[-1], 0.002)]


def make_pair(shape, noise, seed=None):
    """y = rand, sr = y + noise * randn, unclamped, fp32 on the host"""
    g = torch.Generator().manual_seed(1000 + math.prod(shape) if seed is None else seed)
    y = torch.rand(shape, generator=g)
    return y + noise * torch.randn(shape, generator=g), y


def kink_free_pair(shape, seed=100):
    """sr = y + n with 0.01 <= |n| <= 0.05 (L1's gradient is a sign: every pixel difference stays away from the kink)"""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(shape, generator=g)
    n = (torch.rand(shape, generator=g) * 0.04 + 0.01) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return y + n, y
