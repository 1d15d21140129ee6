"""On-the-fly LR synthesis (`online_degradations`): random Gaussian blur + bicubic down-sampling of
the HR image on the device, with the blur-kernel PCA code as the sample's metadata.

ref: Code/sr_tools/gaussian_utils.py:218-303 (random kernels), :193-198 (PCA), :332-343 (PCAEncoder), :346-368
     (BatchBlur), :371-424 (SRMDPreprocessing); Code/sr_tools/data_handler.py:222-238 (degrader set-up: PCA basis from
     30 000 random kernels), :446-456 (per image: degrader -> ToPILImage -> downsample -> metadata);
     Code/sr_tools/image_manipulation.py:32-53 (downsample = centre crop to a multiple of the scale + PIL BICUBIC).

Split of labour.  Everything random or tiny stays on the host, in the reference's call order and on the same numpy
global stream (np.random.random draws per kernel; torch.svd for the PCA basis; the 1 x 441 by 441 x 10 code product).
Pixels stay on the device: csrc/degrade.hip blurs the planar fp32 HR image with reflection padding and quantises it
as ToPILImage does (`mul(255).byte()`), then runs PIL's two 8-bit fixed-point resample passes with coefficient tables
computed here exactly as libImaging/Resample.c computes them -- the LR image is bit-identical to PIL's for the same
uint8 input.  There is no CPU path: the tensors must live on a HIP device.

The same resampler run the other way (`pil_bicubic_upsample`, csrc/interp.hip) is the evaluator's bicubic pre-up-sampling
of an LR batch for the interpolated-input models (ref: Code/SISR/evaluation/standard_eval.py:146-164).

JPEG compression (`jpeg_roundtrip`, csrc/jpeg.hip; ref: Code/data_converter.py jpeg_compress, `save(buf, "JPEG",
subsampling=0, quality=q)` + `open`) is the optional last stage on the LR bytes: libjpeg's integer arithmetic per 8 x 8
block, bit-identical to PIL's decoded image.  `jpeg_roundtrip_host` states the same arithmetic in numpy for images that
are on the host anyway (tools/make_jpeg_set.py without a GPU) and is what the CPU tests hold against PIL.

Tile-level mode (`degrade_tiles`, csrc/degrade_tiles.hip; `[data] degrade_tiles = true`): the same stages on the HR window a
batch's tiles depend on instead of on whole images -- one launch per batch, bit-identical tiles -- with the noise from a
counter-based field (`normal_field`, numpy mirror `normal_field_host`) and JPEG on the tile.  OnlineDegrader.draw() makes an
access's random draws, apply() the whole-image pixel work; the tile loader (data.DeviceTileLoader) uses draw() alone.

Interpolated-input and Y-channel models (`input = 'interp'`, `colorspace = 'ycbcr'`; no reference counterpart: the reference
prepares such sets offline, data_converter.py `downscale` then `upscale`): OnlineDegrader(interp=True) up-samples the LR bytes
back to the HR size with Pillow's bicubic resize (pil_bicubic_upsample), `ycbcr` converts to BT.601 'jpg' YCbCr or Y.  In the
tile-level mode `interp_window` names the LR window a tile of the up-sampled image depends on, degrade_tiles makes that
window's bytes and `upsample_tiles` (csrc/interp_tiles.hip) turns a batch's windows into its tiles; `rgb_to_ycbcr` converts
the HR tiles.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import hip

PRECISION_BITS = 32 - 8 - 2  # libImaging/Resample.c


# ----------------------------------------------------------------------------- random blur kernels (host, np.random)
def isotropic_gaussian_kernel(l, sigma):
    ax = np.arange(-l // 2 + 1., l // 2 + 1.)
    xx, yy = np.meshgrid(ax, ax)
    kernel = np.exp(-(xx ** 2 + yy ** 2) / (2. * sigma ** 2))
    return kernel / np.sum(kernel)


def cal_sigma(sig_x, sig_y, radians):
    D = np.array([[sig_x ** 2, 0], [0, sig_y ** 2]])
    U = np.array([[np.cos(radians), -np.sin(radians)], [np.sin(radians), 1 * np.cos(radians)]])
    return np.dot(U, np.dot(D, U.T))


def anisotropic_gaussian_kernel(l, sigma_matrix):
    ax = np.arange(-l // 2 + 1., l // 2 + 1.)
    xx, yy = np.meshgrid(ax, ax)
    xy = np.hstack((xx.reshape((l * l, 1)), yy.reshape(l * l, 1))).reshape(l, l, 2)
    inverse_sigma = np.linalg.inv(sigma_matrix)
    kernel = np.exp(-0.5 * np.sum(np.dot(xy, inverse_sigma) * xy, 2))
    return kernel / np.sum(kernel)


def random_gaussian_kernel(l=21, sig_min=0.2, sig_max=4.0, rate_iso=1.0, scaling=3):
    """One kernel; consumes np.random exactly as gaussian_utils.random_gaussian_kernel (:278-282)."""
    if np.random.random() < rate_iso:
        x = np.random.random() * (sig_max - sig_min) + sig_min
        return isotropic_gaussian_kernel(l, x)
    pi = np.random.random() * math.pi * 2 - math.pi
    x = np.random.random() * (sig_max - sig_min) + sig_min
    y = np.clip(np.random.random() * scaling * x, sig_min, sig_max)
    return anisotropic_gaussian_kernel(l, cal_sigma(x, y, pi))


def random_batch_kernel(batch, l=21, sig_min=0.2, sig_max=4.0, rate_iso=1.0, scaling=3):
    out = np.zeros((batch, l, l))
    for i in range(batch):
        out[i] = random_gaussian_kernel(l=l, sig_min=sig_min, sig_max=sig_max, rate_iso=rate_iso, scaling=scaling)
    return out


def pca_matrix(batch=30000, k=10):
    """The kernel-code basis the dataset builds at construction (data_handler.py:228-231): `batch` random default
    kernels from the np.random stream, centred, torch.svd of the transposed data, first k left singular vectors."""
    data = random_batch_kernel(batch=batch).reshape((batch, -1))
    X = torch.from_numpy(data)
    X = X - torch.mean(X, 0).expand_as(X)
    U, S, V = torch.svd(torch.t(X))
    return U[:, :k].float()


def encode_kernel(kernel_f32, pca):
    """PCAEncoder (:332-343): (l, l) float32 kernel -> (k,) code."""
    kt = torch.as_tensor(kernel_f32, dtype=torch.float32)
    return torch.bmm(kt.reshape(1, 1, -1), pca.expand((1,) + tuple(pca.shape))).view(-1)


# ----------------------------------------------------------------------------- PIL's bicubic coefficient tables (host)
def _bicubic_filter(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def pil_bicubic_table(in_size, out_size):
    """libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc for a full-extent box:
    -> (bounds int32 [out][2] = (first tap, taps), coef int32 [out][ksize], ksize)."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [_bicubic_filter((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, coef, ksize


_tables = {}


def _device_table(in_size, out_size, device):
    key = (in_size, out_size, device.index)
    t = _tables.get(key)
    if t is None:
        b, c, ks = pil_bicubic_table(in_size, out_size)
        t = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), ks)
        _tables[key] = t
    return t


_host_tables = {}


def _host_table(in_size, out_size):
    t = _host_tables.get((in_size, out_size))
    if t is None:
        t = _host_tables[(in_size, out_size)] = pil_bicubic_table(in_size, out_size)
    return t


def interp_window_edge(crop, scale):
    """Edge of the LR window behind a `crop`-pixel tile of the x `scale` up-sampled image: output o reads the LR pixels
    floor((o + 0.5) / s - 1.5) .. floor((o + 0.5) / s + 2.5) - 1 (clipped to the image), so `crop` consecutive outputs read at
    most floor((crop - 1) / s) + 5 of them, whatever the tile's origin is modulo s."""
    return (int(crop) - 1) // int(scale) + 5


def interp_window(size, scale, crop, origin):
    """Along one axis: the LR window that outputs origin .. origin + crop - 1 of the bicubic up-sampling (size -> size * scale)
    depend on -> (first, edge).  `edge` = interp_window_edge(crop, scale) for every origin, so one batch has one window edge;
    `first` is the first tap of output `origin` in the whole-image table, moved back where the window would leave the image."""
    size, scale, crop, origin = int(size), int(scale), int(crop), int(origin)
    edge = interp_window_edge(crop, scale)
    if not 0 <= origin <= size * scale - crop:
        raise ValueError(f"a {crop}-pixel tile at {origin} leaves the {size * scale}-pixel up-sampled image")
    if size < edge:
        raise ValueError(f"LR image side {size} is smaller than the {edge}-pixel window of a {crop}-pixel tile at x {scale}")
    bounds = _host_table(size, size * scale)[0]
    return min(int(bounds[origin, 0]), size - edge), edge


# ----------------------------------------------------------------------------- the degradation as one linear operator (host, float64)
# Away from the image border Pillow's bicubic down-sampling by an integer factor is shift-invariant: every output row from
# index 2 to out - 3 has the same taps relative to s * i, and they are mirror-symmetric (first + last = s - 1).  Blur and both
# tap passes are then ONE stride-s cross-correlation with a composed kernel; csrc/consistency.hip applies it
# and its adjoint to float images -- the differentiable form of the 8-bit pipeline above (ops.degrade_valid).
CONSISTENCY_SCALES = (2, 3, 4)


def bicubic_interior_taps(scale):
    """-> (first, weights): the non-zero taps of an interior output i of Pillow's bicubic down-sampling by `scale`, at input
    indices scale * i + first ..., float64, normalised as precompute_coeffs does (w / ww) BEFORE the fixed-point rounding of
    normalize_coeffs_8bpc.  Scale 4: 16 taps from -6; 3: 11 taps from -4; 2: 8 taps from -3."""
    if isinstance(scale, bool) or scale not in CONSISTENCY_SCALES:
        raise ValueError(f"bicubic_interior_taps: scale must be one of {CONSISTENCY_SCALES}; got {scale!r}")
    s, xx = int(scale), 8  # any interior row: precompute_coeffs' own arithmetic at row 8 of a 64-row output
    support = 2.0 * s
    center = (xx + 0.5) * s
    xmin = int(center - support + 0.5)
    xmax = int(center + support + 0.5) - xmin
    w = [_bicubic_filter((x + xmin - center + 0.5) * (1.0 / s)) for x in range(xmax)]
    ww = 0.0
    for v in w:
        ww += v
    w = np.array([v / ww for v in w], np.float64)
    keep = np.flatnonzero(w)
    return xmin + int(keep[0]) - s * xx, w[keep[0]:keep[-1] + 1].copy()


def flip_kernels(kernels, flips):
    """(B, l, l) kernels under each sample's (hflip, vflip, transpose) flags, applied as random_flip_rotate applies them to an
    image: T D_k(x) = D_{T k}(T x) (the taps are mirror-symmetric and centred on the s-pixel cell)."""
    out = np.array(kernels, np.float64, copy=True)
    if flips is None:
        return out
    flips = np.asarray(flips)
    if flips.shape != (out.shape[0], 3):
        raise ValueError(f"flips must be a (B, 3) table of (hflip, vflip, transpose) flags; got shape {flips.shape}")
    for b, (hf, vf, tr) in enumerate(flips):
        k = out[b]
        if hf:
            k = k[:, ::-1]
        if vf:
            k = k[::-1, :]
        if tr:
            k = k.T
        out[b] = k
    return out


def compose_degradation(kernels, scale, flips=None):
    """-> (K, first): K (B, n, n) float64, n = taps + l - 1, with D_k(x)[i, j] = sum_ef K[e, f] x[s i + first + e, s j + first + f]
    for every output whose footprint lies inside x: K = (w w^T) * k, BatchBlur's cross-correlation (blurred[p, q] = sum_uv
    k[u, v] x[p - l // 2 + u, q - l // 2 + v]) followed by the two tap passes.  kernels: (B, l, l), l odd and at most 21
    ([[1]]: bicubic alone); flips: (B, 3) flags of the augmentation the tiles went through, or None."""
    k = np.asarray(kernels, np.float64)
    if k.ndim != 3 or k.shape[1] != k.shape[2] or k.shape[1] % 2 != 1 or k.shape[1] > 21 or k.shape[0] < 1:
        raise ValueError(f"compose_degradation takes (B, l, l) blur kernels with l odd and at most 21; got shape {k.shape}")
    first, w = bicubic_interior_taps(scale)
    k = flip_kernels(k, flips)
    l, taps = k.shape[1], len(w)
    n = taps + l - 1
    full = np.zeros((n, l), np.float64)  # full[e, u] = w[e - u]: the full convolution with w as a matrix
    for u in range(l):
        full[u:u + taps, u] = w
    return np.matmul(np.matmul(full, k), full.T), first - l // 2


def consistency_margin(scale, l):
    """LR rows / columns cut at each side of a tile: output i of an h-row tile is kept when its whole footprint (taps plus blur
    radius) lies inside the s h HR rows of the tile, i.e. m <= i < h - m.  4, 5, 7 for s = 4, 3, 2 at l = 21; 2 at s = 4, l = 1."""
    first, _ = bicubic_interior_taps(scale)
    l = int(l)
    if l < 1 or l % 2 != 1 or l > 21:
        raise ValueError(f"consistency_margin: the blur kernel edge must be odd and at most 21; got {l}")
    return -((first - l // 2) // int(scale))  # ceil((l // 2 - first) / s), the same at both sides by the taps' symmetry


def consistency_geometry(scale, n):
    """From the edge n of a composed kernel: (l, m, off) -- the blur edge, the margin and the HR index s m + first - l // 2 >= 0
    of the first input of kept output 0."""
    first, w = bicubic_interior_taps(scale)
    l = int(n) - len(w) + 1
    if l < 1 or l % 2 != 1 or l > 21:
        raise ValueError(f"a composed kernel of edge {n} belongs to no odd blur edge 1..21 at scale {scale}")
    m = consistency_margin(scale, l)
    return l, m, int(scale) * m + first - l // 2


class DegradeValid(torch.autograd.Function):
    """The node behind ops.degrade_valid (which checks the operands and derives the geometry): y = D_K(x) by
    sisr_degrade_valid_fwd, dx = D_K^T(g) by sisr_degrade_valid_bwd.  One differentiable input, no parameter and no gradient
    buffer of its own; K (B, n, n) float64 on x's device takes no gradient; an x that needs none costs no backward launch."""

    @staticmethod
    def forward(ctx, x, K, scale, off, ho, wo):
        x = x.contiguous()
        B, C, H, W = x.shape
        n = K.shape[1]
        y = torch.empty((B, C, ho, wo), device=x.device, dtype=torch.float32)
        hip.check(hip.lib().sisr_degrade_valid_fwd(hip.ptr(x), K.data_ptr(), hip.ptr(y), B, C, H, W, n, scale, off, ho, wo,
                                                   hip.stream()), "sisr_degrade_valid_fwd")
        ctx.save_for_backward(K)
        ctx.geometry = (B, C, H, W, n, scale, off, ho, wo)
        return y

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        (K,) = ctx.saved_tensors
        B, C, H, W, n, scale, off, ho, wo = ctx.geometry
        g = g.contiguous()
        dx = torch.empty((B, C, H, W), device=g.device, dtype=torch.float32)  # the kernel writes every element
        hip.check(hip.lib().sisr_degrade_valid_bwd(hip.ptr(g), K.data_ptr(), hip.ptr(dx), B, C, H, W, n, scale, off, ho, wo,
                                                   hip.stream()), "sisr_degrade_valid_bwd")
        return dx, None, None, None, None, None


# ----------------------------------------------------------------------------- device pipeline
def blur_quant(hr, kernel, want_float=False, want_u8=True):
    """(C, H, W) fp32 on the device, (l, l) kernel -> uint8 (C, H, W) = byte(255 * BatchBlur(hr)); want_float: also
    the unquantised blur (want_u8 False: only that)."""
    if not hr.is_cuda:
        raise RuntimeError("degrade.blur_quant: the image must be on a HIP device (no CPU path)")
    C, H, W = hr.shape
    k = torch.as_tensor(kernel, dtype=torch.float32).to(hr.device).contiguous()
    l = k.shape[-1]
    y = torch.empty((C, H, W), device=hr.device, dtype=torch.uint8) if want_u8 else None
    yf = torch.empty((C, H, W), device=hr.device, dtype=torch.float32) if want_float else None
    hip.check(hip.lib().sisr_blur_quant(hip.ptr(hr.contiguous()), hip.ptr(k), y.data_ptr() if y is not None else None,
                                        hip.ptr(yf), C, H, W, l, hip.stream()), "sisr_blur_quant")
    return (y, yf) if want_float else y


def random_batch_noise(batch, high, rate_cln=1.0):
    """Noise level per sample; consumes np.random exactly as gaussian_utils.random_batch_noise (:299-304)."""
    noise_level = np.random.uniform(size=(batch, 1)) * high
    noise_mask = np.random.uniform(size=(batch, 1))
    noise_mask[noise_mask < rate_cln] = 0
    noise_mask[noise_mask >= rate_cln] = 1
    return noise_level * noise_mask


def noise_quant(blur, sigma, field=None):
    """(C, H, W) fp32 blurred image on the device -> uint8 byte(255 * clamp(N(0,1) * sigma + blur, 0, 1)).  The N(0,1) field
    comes from numpy's global stream on the host, as in the reference (b_GaussianNoising, :306-312), and is uploaded;
    `field`: one drawn already (host or device tensor of blur's size), nothing is drawn here."""
    C, H, W = blur.shape
    if field is None:
        field = torch.FloatTensor(np.random.normal(loc=0.0, scale=1.0, size=(1, C, H, W)))
    field = field.to(blur.device).contiguous()
    if field.numel() != blur.numel():
        raise ValueError(f"noise field of {field.numel()} values for an image of {blur.numel()}")
    y = torch.empty((C, H, W), device=blur.device, dtype=torch.uint8)
    hip.check(hip.lib().sisr_noise_quant(hip.ptr(blur), hip.ptr(field), float(sigma), y.data_ptr(), blur.numel(), hip.stream()),
              "sisr_noise_quant")
    return y


def pil_bicubic_downsample(u8, scale, to_float=True):
    """PIL `resize((W // s, H // s), BICUBIC)` of a planar uint8 (C, H, W) device image whose sides are multiples of s
    -> (C, H / s, W / s): fp32 / 255 (ToTensor) or uint8."""
    C, H, W = u8.shape
    if H % scale or W % scale:
        raise ValueError("centre-crop the image to a multiple of the scale first (image_manipulation.downsample)")
    h, w = H // scale, W // scale
    dev = u8.device
    bh, ch, ksh = _device_table(W, w, dev)
    bv, cv, ksv = _device_table(H, h, dev)
    tmp = torch.empty((C, H, w), device=dev, dtype=torch.uint8)
    L = hip.lib()
    hip.check(L.sisr_pil_resample(u8.contiguous().data_ptr(), tmp.data_ptr(), bh.data_ptr(), ch.data_ptr(), ksh, C, H, W, H, w,
                                  0, 0, hip.stream()), "sisr_pil_resample(h)")
    out = torch.empty((C, h, w), device=dev, dtype=torch.float32 if to_float else torch.uint8)
    hip.check(L.sisr_pil_resample(tmp.data_ptr(), out.data_ptr(), bv.data_ptr(), cv.data_ptr(), ksv, C, H, w, h, w, 1,
                                  int(to_float), hip.stream()), "sisr_pil_resample(v)")
    return out


def pil_bicubic_upsample(lr, scale, rgb=True, ycbcr=False):
    """The evaluator's pre-up-sampling (ref: evaluation/standard_eval.py:146-164) of a (B, 3, h, w) fp32 device batch, one
    launch: per image ToPILImage -> `resize((w * s, h * s), BICUBIC)` -> ToTensor, bit for bit, and / or that image in
    BT.601 'jpg' YCbCr with the fp32 roundings of metrics.rgb_to_ycbcr_jpg.  -> the requested (B, 3, s h, s w) device
    tensors: one tensor, or (rgb, ycbcr) when both are asked for."""
    if not lr.is_cuda:
        raise RuntimeError("degrade.pil_bicubic_upsample: the batch must be on a HIP device (no CPU path)")
    if lr.dim() != 4 or lr.dtype != torch.float32:
        raise ValueError(f"pil_bicubic_upsample takes a (B, C, h, w) fp32 batch; got {lr.dtype} {tuple(lr.shape)}")
    if not (rgb or ycbcr):
        raise ValueError("pil_bicubic_upsample: ask for rgb, ycbcr or both")
    scale = int(scale)
    B, C, h, w = lr.shape
    H, W = h * scale, w * scale
    dev = lr.device
    lr = lr.contiguous()
    with torch.cuda.device(dev):
        bh, ch, ksh = _device_table(w, W, dev)
        bv, cv, ksv = _device_table(h, H, dev)
        assert ksh == ksv
        out_rgb = torch.empty((B, C, H, W), device=dev, dtype=torch.float32) if rgb else None
        out_ycc = torch.empty((B, C, H, W), device=dev, dtype=torch.float32) if ycbcr else None
        hip.check(hip.lib().sisr_pil_upsample(hip.ptr(lr), hip.ptr(out_rgb), hip.ptr(out_ycc), bh.data_ptr(), ch.data_ptr(),
                                              bv.data_ptr(), cv.data_ptr(), ksh, B, C, h, w, H, W, hip.stream()),
                  "sisr_pil_upsample")
    return (out_rgb, out_ycc) if rgb and ycbcr else (out_rgb if rgb else out_ycc)


def rgb_to_ycbcr(rgb, y_only=True):
    """data.rgb_to_ycbcr(im_type='jpg') on the device, bit for bit: (3, H, W) or (B, 3, H, W) fp32 RGB -> the same with 3
    (YCbCr) or 1 (Y alone) planes.  One launch."""
    if not rgb.is_cuda:
        raise RuntimeError("degrade.rgb_to_ycbcr: the image must be on a HIP device (data.rgb_to_ycbcr is the host form)")
    if rgb.dtype != torch.float32 or rgb.dim() not in (3, 4) or rgb.shape[-3] != 3:
        raise ValueError(f"rgb_to_ycbcr takes a (3, H, W) or (B, 3, H, W) fp32 image; got {rgb.dtype} {tuple(rgb.shape)}")
    rgb = rgb.contiguous()
    B = rgb.shape[0] if rgb.dim() == 4 else 1
    H, W = rgb.shape[-2:]
    with torch.cuda.device(rgb.device):
        out = torch.empty(tuple(rgb.shape[:-3]) + (1 if y_only else 3, H, W), device=rgb.device, dtype=torch.float32)
        hip.check(hip.lib().sisr_rgb_to_ycbcr(hip.ptr(rgb), hip.ptr(out), B, H * W, int(bool(y_only)), hip.stream()),
                  "sisr_rgb_to_ycbcr")
    return out


# ----------------------------------------------------------------------------- JPEG round trip (libjpeg's integer arithmetic)
_JPEG_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]).reshape(8, 8)
_JPEG_CHROMA = np.full((8, 8), 99)
_JPEG_CHROMA[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]


def _check_quality(quality):
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= quality <= 100:
        raise ValueError(f"JPEG quality must be an integer in 1..100; got {quality!r}")
    return int(quality)


def jpeg_tables(quality):
    """jcparam.c jpeg_set_quality: the Annex-K luminance and chrominance tables scaled for `quality` (1..100), each an
    (8, 8) int array in natural (row-major) order."""
    q = _check_quality(quality)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (_JPEG_LUMA, _JPEG_CHROMA))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _jpeg_odd_part(t4, t5, t6, t7):
    """The odd half shared by jfdctint.c and jidctint.c: -> (from t4, from t5, from t6, from t7) before the descale."""
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    return t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4


def _jpeg_fdct_pass(d, second):
    """One pass of jfdctint.c over the LAST axis (length 8) of an integer array."""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 15 if second else 11
    o = [None] * 8
    o[0] = _descale(t10 + t11, 2) if second else (t10 + t11) << 2
    o[4] = _descale(t10 - t11, 2) if second else (t10 - t11) << 2
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    o[7], o[5], o[3], o[1] = (_descale(v, n) for v in _jpeg_odd_part(t4, t5, t6, t7))
    return np.stack(o, axis=-1)


def _jpeg_idct_pass(c, second):
    """One pass of jidctint.c over the LAST axis (length 8) of an integer array."""
    c = [c[..., i] for i in range(8)]
    z1 = (c[2] + c[6]) * 4433
    t2, t3 = z1 - c[6] * 15137, z1 + c[2] * 6270
    t0, t1 = (c[0] + c[4]) << 13, (c[0] - c[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = _jpeg_odd_part(c[7], c[5], c[3], c[1])
    n = 18 if second else 11
    return np.stack([_descale(v, n) for v in (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)],
                    axis=-1)


def _jpeg_plane(plane, table):
    """One component (H, W), samples 0..255 in an integer dtype -> the decoded component, same shape and dtype."""
    H, W = plane.shape
    x = np.pad(plane, ((0, -H % 8), (0, -W % 8)), mode="edge") - 128
    x = x.reshape(x.shape[0] // 8, 8, x.shape[1] // 8, 8).transpose(0, 2, 1, 3)  # (by, bx, row, column)
    x = _jpeg_fdct_pass(x, False)                                           # along the rows
    x = _jpeg_fdct_pass(x.swapaxes(-1, -2), True).swapaxes(-1, -2)          # along the columns
    d = table.astype(x.dtype) * 8
    x = np.sign(x) * ((np.abs(x) + d // 2) // d) * table.astype(x.dtype)    # jcdctmgr quantise, jdcoefct dequantise
    x = _jpeg_idct_pass(x.swapaxes(-1, -2), False).swapaxes(-1, -2)         # along the columns
    x = _jpeg_idct_pass(x, True)                                            # along the rows
    x = np.clip(x + 128, 0, 255)
    return x.transpose(0, 2, 1, 3).reshape(H + -H % 8, W + -W % 8)[:H, :W]


def jpeg_roundtrip_host(u8, quality, acc=np.int64):
    """The image `PIL.Image.open` returns after `save(buf, "JPEG", subsampling=0, quality=quality)`, from libjpeg's
    arithmetic in numpy: (C, H, W) uint8 array, C = 3 (RGB) or 1 (PIL mode L) -> (C, H, W) uint8.  `acc`: the integer type
    everything is computed in (the device kernel uses 32 bits; np.int32 here shows that they suffice)."""
    u8 = np.asarray(u8)
    if u8.dtype != np.uint8 or u8.ndim != 3 or u8.shape[0] not in (1, 3) or u8.shape[1] < 1 or u8.shape[2] < 1:
        raise ValueError(f"jpeg_roundtrip_host takes a (1 or 3, H, W) uint8 image; got {u8.dtype} {u8.shape}")
    luma, chroma = jpeg_tables(quality)
    x = u8.astype(acc)
    if x.shape[0] == 1:
        return _jpeg_plane(x[0], luma)[None].astype(np.uint8)
    r, g, b = x
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16                                   # jccolor.c
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    y, cb, cr = _jpeg_plane(y, luma), _jpeg_plane(cb, chroma) - 128, _jpeg_plane(cr, chroma) - 128
    out = (y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb + 32768 - 46802 * cr) >> 16),  # jdcolor.c
           y + ((116130 * cb + 32768) >> 16))
    return np.clip(np.stack(out), 0, 255).astype(np.uint8)


def jpeg_roundtrip(u8, quality, to_float=True):
    """The same round trip on the device, one launch: planar uint8 (C, H, W), C = 3 or 1, as
    `pil_bicubic_downsample(..., to_float=False)` returns it -> (C, H, W) fp32 / 255 (ToTensor) or uint8."""
    if not u8.is_cuda:
        raise RuntimeError("degrade.jpeg_roundtrip: the image must be on a HIP device (no CPU path; jpeg_roundtrip_host is "
                           "the numpy form)")
    if u8.dtype != torch.uint8 or u8.dim() != 3:
        raise ValueError(f"jpeg_roundtrip takes a (C, H, W) uint8 image; got {u8.dtype} {tuple(u8.shape)}")
    quality = _check_quality(quality)
    C, H, W = u8.shape
    u8 = u8.contiguous()
    with torch.cuda.device(u8.device):
        out = torch.empty((C, H, W), device=u8.device, dtype=torch.float32 if to_float else torch.uint8)
        hip.check(hip.lib().sisr_jpeg_roundtrip(u8.data_ptr(), out.data_ptr(), C, H, W, quality, int(bool(to_float)),
                                                hip.stream()), "sisr_jpeg_roundtrip")
    return out


def center_crop_box(height, width, scale):
    """image_manipulation.downsample's crop: (top, left, r_height, r_width), rounding as center_crop does."""
    rh, rw = (height // scale) * scale, (width // scale) * scale
    return int(round((height - rh) / 2.)), int(round((width - rw) / 2.)), rh, rw


# ----------------------------------------------------------------------------- the counter-based N(0,1) field (tile-level noise)
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: counter (..., 4), key (..., 2) uint32 -> (..., 4) uint32."""
    c = [np.asarray(counter, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key, dtype=np.uint32)[..., i].astype(np.uint64) for i in range(2)]
    mask = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(0x9E3779B9)) & mask, (k[1] + np.uint64(0xBB67AE85)) & mask]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def normal_field_words_host(seed, C, H, W):
    """The Philox words behind normal_field: uint32 (C, H, ceil(W / 4), 4) = philox(counter = (column >> 2, row, channel, 0),
    key = (seed, 0))."""
    q = (W + 3) // 4
    ctr = np.zeros((C, H, q, 4), np.uint32)
    ctr[..., 0] = np.arange(q, dtype=np.uint32)[None, None, :]
    ctr[..., 1] = np.arange(H, dtype=np.uint32)[None, :, None]
    ctr[..., 2] = np.arange(C, dtype=np.uint32)[:, None, None]
    return philox4x32_10(ctr, np.array([seed & 0xffffffff, 0], dtype=np.uint32))


def normal_field_host(seed, C, H, W):
    """numpy mirror of normal_field (csrc/noise_field.h): the same words, the same fp32 uniforms u = (float32(word >> 8) +
    0.5) * 2^-24, Box-Muller on them in float64 -> (C, H, W) float64.  Columns 4q, 4q + 1 take r cos(a), r sin(a) of words
    0, 1; columns 4q + 2, 4q + 3 those of words 2, 3."""
    words = normal_field_words_host(seed, C, H, W)
    u = ((words >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    u = u.astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u[..., 0::2]))
    a = 2.0 * np.pi * u[..., 1::2]
    out = np.stack([r * np.cos(a), r * np.sin(a)], axis=-1)  # (C, H, q, pair, cos | sin)
    return out.reshape(C, H, -1)[:, :, :W]


def normal_field(seed, C, H, W, device, words=False):
    """The N(0,1) field the tile-level path adds (times the noise level) to the blurred image: a pure function of (seed,
    channel, row, column) -> (C, H, W) fp32 on the device; words: also the raw Philox words, int32 bit patterns
    (C, H, ceil(W / 4), 4)."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("degrade.normal_field runs on a HIP device (normal_field_host is the numpy form)")
    seed = int(seed)
    if not 0 <= seed < 1 << 32:
        raise ValueError(f"the noise seed is a 32-bit unsigned integer; got {seed}")
    with torch.cuda.device(device):
        field = torch.empty((C, H, W), device=device, dtype=torch.float32)
        w = torch.empty((C, H, (W + 3) // 4, 4), device=device, dtype=torch.int32) if words else None
        hip.check(hip.lib().sisr_normal_field(seed, hip.ptr(field), w.data_ptr() if words else None, C, H, W, hip.stream()),
                  "sisr_normal_field")
    return (field, w) if words else field


# ----------------------------------------------------------------------------- tile-level degradation (csrc/degrade_tiles.hip)
def _upload(parts, device):
    """Several small host arrays as ONE host-to-device copy -> their device addresses (16-byte aligned) and the buffer that
    keeps them alive."""
    offs, total = [], 0
    for p in parts:
        offs.append(total)
        total += (p.nbytes + 15) // 16 * 16
    host = np.zeros(max(total, 16), np.uint8)
    for p, o in zip(parts, offs):
        host[o:o + p.nbytes] = np.frombuffer(p.tobytes(), np.uint8)
    dev = torch.from_numpy(host).to(device)
    return [dev.data_ptr() + o for o in offs], dev


def degrade_tiles(images, kernels, origins, crop, scale, flips=None, sigmas=None, seeds=None, qualities=None, to_float=True):
    """LR tiles of a batch straight from the device-resident HR images: sample b's tile is the `crop` x `crop` square with
    origin origins[b] = (ty, tx) of the LR image the whole-image path would make of images[b] with kernels[b] -- blur_quant
    [+ noise on the unquantised blur], centre crop, pil_bicubic_downsample -- bit for bit, without that image ever existing.

    images: B (C, H, W) fp32 device tensors (sizes may differ); kernels: (B, l, l); flips: B (hflip, vflip, transpose), applied
    to the finished tile as sisr_crop_augment's index map does; sigmas: B noise levels (None: no noise stage; a level of 0 keeps
    the stage's clamp) with seeds: B 32-bit seeds of the counter-based field (normal_field); qualities: B JPEG qualities
    (None: no JPEG stage) -- the round trip of the TILE in source orientation, block grid at the tile's origin, before the
    flips: jpeg_roundtrip of the tile's bytes, not a crop of the whole image's round trip.
    -> (B, C, crop, crop) fp32 / 255 or uint8.  One launch (two with JPEG) and one small upload, whatever B is."""
    B = len(images)
    crop, scale = int(crop), int(scale)
    if B < 1 or len(origins) != B:
        raise ValueError("degrade_tiles needs one tile origin per image")
    if qualities is not None:
        if len(qualities) != B:
            raise ValueError("degrade_tiles needs one JPEG quality per image")
        qualities = [_check_quality(q) for q in qualities]
    if sigmas is not None and (seeds is None or len(sigmas) != B or len(seeds) != B):
        raise ValueError("degrade_tiles needs one noise level and one seed per image")
    if flips is not None and len(flips) != B:
        raise ValueError("degrade_tiles needs one (hflip, vflip, transpose) per image")
    dev = images[0].device
    if any((not im.is_cuda) or im.device != dev or im.dtype != torch.float32 or im.dim() != 3 or not im.is_contiguous()
           for im in images):
        raise RuntimeError("degrade.degrade_tiles: contiguous (C, H, W) fp32 images on one HIP device (no CPU path)")
    C = images[0].shape[0]
    if any(im.shape[0] != C for im in images):
        raise ValueError("degrade_tiles: the images differ in their channel count")
    k = np.ascontiguousarray(torch.as_tensor(kernels, dtype=torch.float32).numpy().reshape(B, -1))
    l = int(round(math.sqrt(k.shape[1])))
    if l * l != k.shape[1]:
        raise ValueError("degrade_tiles takes (B, l, l) blur kernels")
    recs = (hip.DegradeTile * B)()
    bits = []
    for b, im in enumerate(images):
        _, H, W = im.shape
        t0, l0, rh, rw = center_crop_box(H, W, scale)
        bh, ch, ksh = _device_table(rw, rw // scale, dev)
        bv, cv, ksv = _device_table(rh, rh // scale, dev)
        r = recs[b]
        r.image, r.bounds_h, r.coef_h, r.bounds_v, r.coef_v = im.data_ptr(), bh.data_ptr(), ch.data_ptr(), bv.data_ptr(), cv.data_ptr()
        r.H, r.W, r.t0, r.l0, r.rh, r.rw = H, W, t0, l0, rh, rw
        r.ty, r.tx = int(origins[b][0]), int(origins[b][1])
        r.ksize_h, r.ksize_v = ksh, ksv
        f = flips[b] if flips is not None else (0, 0, 0)
        bits.append(int(bool(f[0])) | int(bool(f[1])) << 1 | int(bool(f[2])) << 2)
        r.flips = 0 if qualities is not None else bits[-1]  # with JPEG the flips wait for the round trip's store
        r.noise = int(sigmas is not None)
        r.sigma = float(sigmas[b]) if sigmas is not None else 0.0
        r.seed = int(seeds[b]) & 0xffffffff if sigmas is not None else 0
    L = hip.lib()
    with torch.cuda.device(dev):
        parts = [np.frombuffer(bytes(recs), np.uint8), k]
        if qualities is not None:
            parts += [np.asarray(qualities, np.int32), np.asarray(bits, np.int32)]
        addr, keep = _upload(parts, dev)
        direct = qualities is None
        out = torch.empty((B, C, crop, crop), device=dev, dtype=torch.float32 if (to_float and direct) else torch.uint8)
        hip.check(L.sisr_degrade_tiles(ctypes.addressof(recs), addr[0], addr[1], out.data_ptr(), B, C, crop, l, scale,
                                       int(bool(to_float and direct)), hip.stream()), "sisr_degrade_tiles")
        if not direct:
            u8, out = out, torch.empty((B, C, crop, crop), device=dev, dtype=torch.float32 if to_float else torch.uint8)
            hip.check(L.sisr_jpeg_roundtrip_batch(u8.data_ptr(), out.data_ptr(), addr[2], addr[3], B, C, crop,
                                                  int(bool(to_float)), hip.stream()), "sisr_jpeg_roundtrip_batch")
        del keep  # freed in stream order behind the launches that read it (torch's caching allocator)
    return out


UPSAMPLE_FORMS = {"rgb": 0, "ycbcr": 1, "y": 2}


def upsample_tiles(windows, lr_sizes, scale, window_origins, tile_origins, crop, flips=None, form="rgb"):
    """Tiles of the bicubic pre-up-sampled LR images from their LR windows: sample b's tile is the `crop` x `crop` square with
    origin tile_origins[b] = (ty, tx) of the image that pil_bicubic_upsample makes of the WHOLE (h, w) = lr_sizes[b] LR image,
    bit for bit, computed from windows[b] -- the (C, cw, cw) uint8 square of that LR image at window_origins[b] = (wy, wx), as
    degrade_tiles(..., crop=cw, flips=None, to_float=False) returns it (interp_window names the window a tile needs).
    flips: B (hflip, vflip, transpose), applied on the store as degrade_tiles' are; form: 'rgb' -> (B, C, crop, crop), 'ycbcr'
    -> (B, 3, crop, crop) BT.601 'jpg', 'y' -> (B, 1, crop, crop), fp32.  One launch and one small upload, whatever B is."""
    if form not in UPSAMPLE_FORMS:
        raise ValueError(f"upsample_tiles: form must be one of {sorted(UPSAMPLE_FORMS)}; got {form!r}")
    if not windows.is_cuda:
        raise RuntimeError("degrade.upsample_tiles: the windows must be on a HIP device (no CPU path)")
    if windows.dtype != torch.uint8 or windows.dim() != 4 or windows.shape[2] != windows.shape[3]:
        raise ValueError(f"upsample_tiles takes (B, C, cw, cw) uint8 windows; got {windows.dtype} {tuple(windows.shape)}")
    B, C, cw, _ = windows.shape
    crop, scale = int(crop), int(scale)
    if not (len(lr_sizes) == len(window_origins) == len(tile_origins) == B) or (flips is not None and len(flips) != B):
        raise ValueError("upsample_tiles needs one LR size, window origin, tile origin and (hflip, vflip, transpose) per window")
    dev = windows.device
    windows = windows.contiguous()
    recs = (hip.UpsampleTile * B)()
    ks = 5
    with torch.cuda.device(dev):
        for b in range(B):
            h, w = int(lr_sizes[b][0]), int(lr_sizes[b][1])
            bh, ch, ksh = _device_table(w, w * scale, dev)
            bv, cv, ksv = _device_table(h, h * scale, dev)
            ks = ksh if ksh == ksv else 0
            r = recs[b]
            r.bounds_h, r.coef_h, r.bounds_v, r.coef_v = bh.data_ptr(), ch.data_ptr(), bv.data_ptr(), cv.data_ptr()
            r.h, r.w, r.H, r.W = h, w, h * scale, w * scale
            r.wy, r.wx = int(window_origins[b][0]), int(window_origins[b][1])
            r.ty, r.tx = int(tile_origins[b][0]), int(tile_origins[b][1])
            f = flips[b] if flips is not None else (0, 0, 0)
            r.flips = int(bool(f[0])) | int(bool(f[1])) << 1 | int(bool(f[2])) << 2
        addr, keep = _upload([np.frombuffer(bytes(recs), np.uint8)], dev)
        out = torch.empty((B, {"rgb": C, "ycbcr": 3, "y": 1}[form], crop, crop), device=dev, dtype=torch.float32)
        hip.check(hip.lib().sisr_upsample_tiles(ctypes.addressof(recs), addr[0], windows.data_ptr(), hip.ptr(out), ks, B, C, crop,
                                                cw, UPSAMPLE_FORMS[form], hip.stream()), "sisr_upsample_tiles")
        del keep  # freed in stream order behind the launch that reads it
    return out


DegraderDraw = collections.namedtuple("DegraderDraw", "kernel code level seed field quality")


class OnlineDegrader:
    """SRMDPreprocessing(pca, random=True[, noise]) + ToPILImage + downsample for one image at a time, as
    SuperResImages.__getitem__ applies it (data_handler.py:446-456); returns device tensors.  With `noise` (ref
    gaussian_utils.py:371-424; the reference's own default for SRMDPreprocessing, off in the dataset's default set-up):
    a noise level per image (random_batch_noise: uniform * noise_high, zero with probability rate_cln), Gaussian noise of
    that level on the BLURRED full-size image, clamped to [0, 1], and 10 * level appended to the kernel code.
    With `jpeg` (not a reference option; its offline counterpart is data_converter.py's jpeg_compress): the LR bytes go
    through a JPEG round trip at a quality drawn per image from `jpeg_quality` = q or [lo, hi] (inclusive) -- the last draw
    of the call, one np.random.randint -- and (q - a) / (b - a) is appended to the code, [a, b] = `jpeg_norm` (default: the
    quality range; [0, 100] for a single quality): the min-max normalisation the reference applies to an integer CSV column.
    With `interp` (no reference counterpart online; offline it is data_converter.py's `downscale` then `upscale`): the LR bytes
    are up-sampled back by the same factor with Pillow's `resize((w * s, h * s), BICUBIC)` and ToTensor, so the image has the
    size of the centre-cropped HR image.  `degradation_scale`: the down (and up) factor when it is not the data set's `scale`
    -- interpolated-input sets that crop pair LR and HR by scale = 1.  `ycbcr` (likewise no reference counterpart online): the
    image in BT.601 'jpg' YCbCr, bit for bit data.rgb_to_ycbcr's; `y_only`: its plane 0 alone."""

    def __init__(self, scale=4, pca=None, kernel=21, sig_min=0.2, sig_max=4.0, rate_iso=1.0, scaling=3, noise=False,
                 random=True, sig=2.6, para_input=10, rate_cln=0.2, noise_high=0.08, jpeg=False, jpeg_quality=(30, 95),
                 jpeg_norm=None, interp=False, degradation_scale=None, ycbcr=False, y_only=True, **unused):
        self.interp, self.ycbcr, self.y_only = bool(interp), bool(ycbcr), bool(y_only)
        if degradation_scale is not None:
            if isinstance(degradation_scale, bool) or int(degradation_scale) != degradation_scale or degradation_scale < 1:
                raise ValueError(f"degradation_scale must be a positive integer; got {degradation_scale!r}")
            if not self.interp and int(degradation_scale) != int(scale):
                raise ValueError(f"degradation_scale = {degradation_scale} differs from scale = {scale}: LR and HR crops are "
                                 "paired by `scale`, so only input = 'interp' can degrade by another factor")
            scale = int(degradation_scale)
        elif self.interp and int(scale) <= 1:
            raise ValueError("online degradations with input = 'interp' and scale = 1 need the down- and up-sampling factor: "
                             "online_degradation_params = { degradation_scale = s }")
        self.jpeg = bool(jpeg)
        if self.jpeg:
            lo, hi = (jpeg_quality, jpeg_quality) if np.isscalar(jpeg_quality) else jpeg_quality
            self.jpeg_lo, self.jpeg_hi = _check_quality(lo), _check_quality(hi)
            if self.jpeg_lo > self.jpeg_hi:
                raise ValueError(f"jpeg_quality = [lo, hi] needs lo <= hi; got {jpeg_quality!r}")
            if jpeg_norm is None:
                jpeg_norm = (self.jpeg_lo, self.jpeg_hi) if self.jpeg_lo < self.jpeg_hi else (0, 100)
            self.jpeg_norm = (float(jpeg_norm[0]), float(jpeg_norm[1]))
            if not self.jpeg_norm[0] < self.jpeg_norm[1]:
                raise ValueError(f"jpeg_norm = [a, b] needs a < b; got {jpeg_norm!r}")
        self.noise, self.rate_cln, self.noise_high = bool(noise), rate_cln, noise_high
        self.scale, self.l, self.random, self.sig = int(scale), int(kernel), bool(random), 2.6 if sig is None else sig
        self.sig_min, self.sig_max, self.rate_iso, self.scaling = sig_min, sig_max, rate_iso, scaling
        self.pca = pca if pca is not None else pca_matrix()
        self.para_in = para_input

    def metadata_keys(self):
        """The keys of the code's entries.  Without `jpeg`: the reference's list, 'blur_kernel' per kernel-code entry (the
        noise level, when on, has none: data_handler.py:293-297).  With it every value has a key."""
        keys = ['blur_kernel'] * self.para_in
        if self.jpeg:
            keys += (['noise'] if self.noise else []) + ['jpeg_quality']
        return keys

    def draw_kernel(self):
        if self.random:
            k = random_gaussian_kernel(l=self.l, sig_min=self.sig_min, sig_max=self.sig_max, rate_iso=self.rate_iso,
                                       scaling=self.scaling)
        else:
            k = isotropic_gaussian_kernel(self.l, self.sig)
        return torch.FloatTensor(k)  # the reference converts the float64 kernel to float32 here (:303)

    def draw(self, field_shape=None):
        """Every random draw of one access, on numpy's global stream in the reference's order, and nothing else: the kernel
        draws; with `noise` the level and its clean mask (random_batch_noise) and then EITHER the host N(0,1) field of
        `field_shape` = (C, H, W) (the whole-image path: np.random.normal, as b_GaussianNoising) OR, without a shape, one
        np.random.randint for the 32-bit seed of the counter-based field (the tile-level path, normal_field); with `jpeg` one
        np.random.randint for the quality, last.  -> DegraderDraw(kernel, code, level, seed, field, quality): kernel (l, l)
        and code float32 CPU tensors (code complete: kernel code [+ 10 * level] [+ normalised quality]), level a float or
        None, seed an int or None, field a (1, C, H, W) float32 CPU tensor or None, quality an int or None."""
        kernel = self.draw_kernel()
        code = encode_kernel(kernel, self.pca)
        level = seed = field = quality = None
        if self.noise:
            lv = torch.FloatTensor(random_batch_noise(1, self.noise_high, self.rate_cln))  # (1, 1) float32, as the reference
            level = float(lv[0, 0])
            if field_shape is not None:
                field = torch.FloatTensor(np.random.normal(loc=0.0, scale=1.0, size=(1,) + tuple(field_shape)))
            else:
                seed = int(np.random.randint(0, 1 << 32, dtype=np.int64))
            code = torch.cat([code, (lv * 10).view(-1)])
        if self.jpeg:
            quality = int(np.random.randint(self.jpeg_lo, self.jpeg_hi + 1))
            a, b = self.jpeg_norm
            code = torch.cat([code, torch.tensor([(quality - a) / (b - a)], dtype=torch.float32)])
        return DegraderDraw(kernel, code, level, seed, field, quality)

    def apply(self, hr, d):
        """The pixel work of the whole-image path for the draws `d` (of draw(field_shape=hr.shape)) -> (lr, box); lr in its
        final form (finish)."""
        if self.noise:
            _, blurred = blur_quant(hr, d.kernel, want_float=True, want_u8=False)
            u8 = noise_quant(blurred, d.level, field=d.field)
        else:
            u8 = blur_quant(hr, d.kernel)
        top, left, rh, rw = center_crop_box(hr.shape[1], hr.shape[2], self.scale)
        if (rh, rw) != (hr.shape[1], hr.shape[2]):
            u8 = u8[:, top:top + rh, left:left + rw].contiguous()
        if not self.jpeg:
            lr = pil_bicubic_downsample(u8, self.scale)
        else:
            lr = jpeg_roundtrip(pil_bicubic_downsample(u8, self.scale, to_float=False), d.quality)
        return self.finish(lr), (top, left, rh, rw)

    def lr_form(self):
        """What finish() and upsample_tiles write: 'rgb', 'ycbcr' or 'y'."""
        return ("y" if self.y_only else "ycbcr") if self.ycbcr else "rgb"

    def finish(self, lr):
        """The fp32 LR image (C, h, w) -> the sample's 'lr' before flips and crops: up-sampled with `interp`, colour-converted
        with `ycbcr`.  float32(b / 255) * 255 truncates back to b for every byte b, so pil_bicubic_upsample's ToPILImage gives
        the LR bytes back and its result is Pillow's resize of them."""
        if self.ycbcr and lr.shape[0] != 3:
            raise ValueError(f"colorspace = 'ycbcr' needs RGB images; got {lr.shape[0]} channel(s)")
        if self.interp:
            out = pil_bicubic_upsample(lr[None], self.scale, rgb=not self.ycbcr, ycbcr=self.ycbcr)[0]
            return out[:1].contiguous() if self.ycbcr and self.y_only else out
        return rgb_to_ycbcr(lr, self.y_only) if self.ycbcr else lr

    def __call__(self, hr):
        """hr: (3, H, W) fp32 in [0, 1] on the device -> (lr (3, h, w) fp32 device -- (3 or 1, rh, rw) with `interp`, 1 plane
        with `ycbcr` and `y_only` --, code (k,) float32 CPU tensor, kernel (l, l) float32 CPU tensor, (top, left, rh, rw) the HR
        centre crop that matches lr)."""
        d = self.draw(field_shape=tuple(hr.shape))
        lr, box = self.apply(hr, d)
        return lr, d.code, d.kernel, box
