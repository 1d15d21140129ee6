"""PSNR and SSIM on the BT.601 'jpg' luma, the reference's validation / evaluation metrics.

`psnr` is host-side numpy.  SSIM has a host float64 form (`ssim`, numpy only) and a device form (csrc/metrics.hip,
`sisr_ssim`) that `batch_ssim` uses for tensors on a HIP device.  The output stage of evaluation -- Y-PSNR of a batch
against its HR batch, with the papers' border crop (`shave`), and the 8-bit HWC image a PNG is written from -- has a device
form too (csrc/eval_output.hip, `sisr_eval_output`: one streaming pass for either or both): `batch_psnr`, `batch_rgb8` and
`eval_output` use it for tensors on a HIP device and the host expressions of this file otherwise.  The device bytes of a
Y-channel output saturate (0 / 255) where the host's `astype(uint8)` of an out-of-gamut value wraps.

ref: Code/sr_tools/metrics.py:6-17 (psnr), :64-91 (ssim: skimage.metrics.structural_similarity with gaussian_weights=True,
     sigma=1.5, use_sample_covariance=False, on Y planes one image at a time), Code/sr_tools/image_manipulation.py:65-89
     (rgb_to_ycbcr 'jpg'), Code/SISR/models/__init__.py:158-169 (clip to [0,1] before conversion).
"""
import numpy as np


def psnr(img1, img2, max_value=255.0):
    mse = np.mean((np.array(img1, dtype=np.float32) - np.array(img2, dtype=np.float32)) ** 2)
    if mse == 0:
        return 100
    return 20 * np.log10(max_value / (np.sqrt(mse)))


SSIM_SIGMA, SSIM_TRUNCATE = 1.5, 3.5
SSIM_RADIUS = int(SSIM_TRUNCATE * SSIM_SIGMA + 0.5)  # 5: an 11 x 11 window


def ssim_taps():
    """The 11 Gaussian taps, computed as scipy.ndimage's _gaussian_kernel1d(1.5, 0, 5) computes them."""
    x = np.arange(-SSIM_RADIUS, SSIM_RADIUS + 1)
    phi = np.exp(-0.5 / (SSIM_SIGMA * SSIM_SIGMA) * x ** 2)
    return phi / phi.sum()


def _valid_gauss(m, taps):
    """Separable correlation with `taps` over the windows that lie inside the 2-D map `m` (rows, then columns)."""
    k = len(taps)
    h, w = m.shape[0] - k + 1, m.shape[1] - k + 1
    t = taps[0] * m[0:h]
    for i in range(1, k):
        t = t + taps[i] * m[i:i + h]
    u = taps[0] * t[:, 0:w]
    for i in range(1, k):
        u = u + taps[i] * t[:, i:i + w]
    return u


def ssim(img1, img2, max_value=1):
    """Mean SSIM of two 2-D images in float64: skimage.metrics.structural_similarity(img1, img2, data_range=max_value,
    gaussian_weights=True, sigma=1.5, use_sample_covariance=False) as scikit-image 0.16-0.18 computes it.  Its map is cropped
    by the filter radius, so only windows inside the image count and the filter's padding mode never shows."""
    x = np.asarray(img1, dtype=np.float64)
    y = np.asarray(img2, dtype=np.float64)
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError(f"ssim takes two 2-D images of one shape; got {x.shape} and {y.shape}")
    win = 2 * SSIM_RADIUS + 1
    if min(x.shape) < win:
        raise ValueError("win_size exceeds image extent.  Either ensure that your images are at least 11x11; or pass "
                         "win_size explicitly in the function call, with an odd value less than or equal to the smaller "
                         "side of your images.")
    taps = ssim_taps()
    ux, uy = _valid_gauss(x, taps), _valid_gauss(y, taps)
    uxx, uyy, uxy = _valid_gauss(x * x, taps), _valid_gauss(y * y, taps), _valid_gauss(x * y, taps)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    c1, c2 = (0.01 * max_value) ** 2, (0.03 * max_value) ** 2
    a1, a2 = 2 * ux * uy + c1, 2 * vxy + c2
    b1, b2 = ux ** 2 + uy ** 2 + c1, vx + vy + c2
    return float(((a1 * a2) / (b1 * b2)).mean(dtype=np.float64))


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)  # Wang et al. 2003, as given (they sum to 1.0001)


MS_SSIM_MAX_LEVELS = 8


def ms_ssim_weights(weights):
    """the weights as a tuple of floats, checked: 1 .. 8 of them, each finite and >= 0 (the one check of the host form, the
    operator, the criterion and the handlers)"""
    try:
        w = tuple(float(v) for v in weights)
    except TypeError:
        raise ValueError(f"ms_ssim_weights must be a sequence of 1 to {MS_SSIM_MAX_LEVELS} numbers; got {weights!r}") from None
    if not 1 <= len(w) <= MS_SSIM_MAX_LEVELS or not all(np.isfinite(v) and v >= 0 for v in w):
        raise ValueError(f"ms_ssim_weights must be 1 to {MS_SSIM_MAX_LEVELS} finite numbers >= 0; got {weights!r}")
    return w


def ms_ssim_min_side(levels):
    """the smallest image side `levels` scales take: the coarsest scale must hold one 11 x 11 window"""
    return (2 * SSIM_RADIUS + 1) << (levels - 1)


def ms_ssim_check_size(what, hw, levels):
    win, least = 2 * SSIM_RADIUS + 1, ms_ssim_min_side(levels)
    if min(hw) < least:
        raise ValueError(f"{what}: with {levels} scales both image sides must be at least {least} (one {win} x {win} window "
                         f"on the coarsest scale); got {tuple(hw)}.  Smaller images take fewer scales: pass fewer weights in "
                         f"ms_ssim_weights (each one less halves the minimum)")


def _ms_ssim_levels(weights, hw):
    """the weights as floats, after the checks of the device form: 1 .. 8 finite numbers >= 0, and an image whose coarsest
    scale holds one window"""
    w = ms_ssim_weights(weights)
    ms_ssim_check_size("ms_ssim", hw, len(w))
    return w


def ms_ssim(img1, img2, max_value=1, weights=MS_SSIM_WEIGHTS):
    """Multi-scale SSIM of two 2-D images in float64 (Wang, Simoncelli, Bovik 2003): prod_j c_j^weights[j], c_j the mean over
    the windows inside scale j of the contrast-structure term A2 / B2, at the last scale of the full SSIM; every scale with the
    window and constants of `ssim`.  Scale j + 1 is the 2 x 2 mean of scale j with stride 2, a trailing odd row or column
    dropped (pytorch_msssim zero-pads odd sides instead: its values differ on such images).  0 when any c_j <= 0, a scale of weight 0 included: the
    rule looks at the means, not at the weights, as the device form does."""
    x = np.asarray(img1, dtype=np.float64)
    y = np.asarray(img2, dtype=np.float64)
    if x.ndim != 2 or x.shape != y.shape:
        raise ValueError(f"ms_ssim takes two 2-D images of one shape; got {x.shape} and {y.shape}")
    weights = _ms_ssim_levels(weights, x.shape)
    taps = ssim_taps()
    c1, c2 = (0.01 * max_value) ** 2, (0.03 * max_value) ** 2
    value = 1.0
    for j, wj in enumerate(weights):
        if j:
            h2, w2 = x.shape[0] // 2 * 2, x.shape[1] // 2 * 2
            x, y = ((((t[0:h2:2, 0:w2:2] + t[0:h2:2, 1:w2:2]) + t[1:h2:2, 0:w2:2]) + t[1:h2:2, 1:w2:2]) * 0.25
                    for t in (x, y))
        ux, uy = _valid_gauss(x, taps), _valid_gauss(y, taps)
        uxx, uyy, uxy = _valid_gauss(x * x, taps), _valid_gauss(y * y, taps), _valid_gauss(x * y, taps)
        vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
        a2, b2 = 2 * vxy + c2, vx + vy + c2
        if j == len(weights) - 1:
            a1, b1 = 2 * ux * uy + c1, ux ** 2 + uy ** 2 + c1
            c = float(((a1 * a2) / (b1 * b2)).mean(dtype=np.float64))
        else:
            c = float((a2 / b2).mean(dtype=np.float64))
        if c <= 0:
            return 0.0
        value *= c ** wj
    return float(value)


def rgb_to_ycbcr_jpg(img, max_val=1):
    """C,H,W RGB -> (Y, Cb, Cr), full-range BT.601 without luma offset."""
    bias_c = 128. * (max_val / 255)
    y = 0.299 * img[0] + 0.587 * img[1] + 0.114 * img[2]
    cb = bias_c + (-0.168736 * img[0] - 0.331264 * img[1] + 0.5 * img[2])
    cr = bias_c + (0.5 * img[0] - 0.418688 * img[1] - 0.081312 * img[2])
    return np.array([y, cb, cr])


def ycbcr_to_rgb_jpg(img, max_val=1):
    """C,H,W YCbCr -> (R, G, B): the inverse of rgb_to_ycbcr_jpg (ref: sr_tools/image_manipulation.py:100-105)."""
    bias = 128. * (max_val / 255)
    r = img[0] + 1.402 * img[2] - 1.402 * bias
    g = img[0] - 0.344136 * img[1] - 0.714136 * img[2] + (0.714136 + 0.344136) * bias
    b = img[0] + 1.772 * img[1] - 1.772 * bias
    return np.array([r, g, b])


def standard_image_formatting(im, min_value=0, max_value=1):
    return np.clip(np.copy(im), min_value, max_value)


def batch_rgb_to_ycbcr(batch):
    """(N,3,H,W) in [0,1] (clipped first) -> (N,3,H,W) YCbCr."""
    out = standard_image_formatting(np.asarray(batch))
    for i in range(out.shape[0]):
        out[i] = rgb_to_ycbcr_jpg(out[i])
    return out


def batch_ycbcr_to_rgb(batch):
    """(N,3,H,W) YCbCr in [0,1] (clipped first) -> (N,3,H,W) RGB (ref: models/__init__.py:158-163, colorspace='ycbcr')."""
    out = standard_image_formatting(np.asarray(batch))
    for i in range(out.shape[0]):
        out[i] = ycbcr_to_rgb_jpg(out[i])
    return out


def y_psnr(sr, hr, max_value=1):
    """PSNR between the Y channels of a clipped SR image and its HR reference (both C,H,W RGB in [0,1])."""
    a = rgb_to_ycbcr_jpg(standard_image_formatting(np.asarray(sr)))[0]
    b = rgb_to_ycbcr_jpg(standard_image_formatting(np.asarray(hr)))[0]
    return psnr(a, b, max_value=max_value)


def y_ssim(sr, hr, max_value=1):
    """SSIM between the Y channels of a clipped SR image and its HR reference (both C,H,W RGB in [0,1])."""
    a = rgb_to_ycbcr_jpg(standard_image_formatting(np.asarray(sr)))[0]
    b = rgb_to_ycbcr_jpg(standard_image_formatting(np.asarray(hr)))[0]
    return ssim(a, b, max_value=max_value)


def _batch_pair(name, sr, hr):
    """The front half of batch_ssim / batch_ms_ssim: two (N, 1|3, H, W) batches of one shape -> (device, a, b).  If either is a
    tensor on a HIP device, both as fp32 contiguous tensors on it; otherwise device None and numpy arrays whose plane 0 is Y
    (C == 3: of the clipped RGB, batch_rgb_to_ycbcr)."""
    import torch
    dev = next((t.device for t in (sr, hr) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is None:
        a, b = (t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (sr, hr))
        if a.ndim != 4 or a.shape != b.shape or a.shape[1] not in (1, 3):
            raise ValueError(f"{name} takes two (N, 1|3, H, W) batches of one shape; got {a.shape} and {b.shape}")
        if a.shape[1] == 3:
            a, b = batch_rgb_to_ycbcr(a), batch_rgb_to_ycbcr(b)
        return None, a, b
    a, b = (torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous() for t in (sr, hr))
    if a.dim() != 4 or a.shape != b.shape or a.shape[1] not in (1, 3):
        raise ValueError(f"{name} takes two (N, 1|3, H, W) batches of one shape; got {tuple(a.shape)} and {tuple(b.shape)}")
    return dev, a, b


def batch_ssim(sr, hr, max_value=1):
    """Per-image SSIM of two (N, C, H, W) batches -> list of N floats.  C == 3: clipped RGB compared on Y (as y_ssim);
    C == 1: Y planes used as given.  If either batch is a tensor on a HIP device, both go to the device kernel (sisr_ssim,
    fp32 contiguous copies made here); anything else takes the host float64 form."""
    dev, a, b = _batch_pair("batch_ssim", sr, hr)
    if dev is None:
        return [ssim(a[i, 0], b[i, 0], max_value=max_value) for i in range(a.shape[0])]
    import torch
    from . import hip
    n, c, h, w = a.shape
    L = hip.lib()
    nbytes = L.sisr_ssim_workspace_bytes(n, h, w)
    if nbytes == 0:
        raise ValueError("win_size exceeds image extent.  Images must be at least 11x11.")
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        hip.check(L.sisr_ssim(hip.ptr(a), hip.ptr(b), n, c, h, w, float(max_value), out.data_ptr(), ws.data_ptr(), nbytes,
                              hip.stream()), "sisr_ssim")
    return out.cpu().tolist()


def batch_ms_ssim(sr, hr, max_value=1, weights=MS_SSIM_WEIGHTS):
    """Per-image multi-scale SSIM of two (N, C, H, W) batches -> list of N floats, as batch_ssim: C == 3 is clipped RGB
    compared on Y, C == 1 Y planes used as given.  If either batch is a tensor on a HIP device, both go to the device
    kernels (sisr_luma_clip for C == 3, then sisr_ms_ssim's per-plane output); anything else takes the host form `ms_ssim`.
    An image with a side under 11 * 2^(len(weights) - 1) raises."""
    dev, a, b = _batch_pair("batch_ms_ssim", sr, hr)
    if dev is None:
        return [ms_ssim(a[i, 0], b[i, 0], max_value=max_value, weights=weights) for i in range(a.shape[0])]
    import ctypes
    import torch
    from . import hip
    n, c, h, w = a.shape
    weights = _ms_ssim_levels(weights, (h, w))
    if n == 0:
        return []
    L = hip.lib()
    with torch.cuda.device(dev):
        if c == 3:
            planes = []
            for t in (a, b):
                yp = torch.empty((n, 1, h, w), dtype=torch.float32, device=dev)
                hip.check(L.sisr_luma_clip(hip.ptr(t), n, h, w, hip.ptr(yp), hip.stream()), "sisr_luma_clip")
                planes.append(yp)
            a, b = planes
        nbytes = L.sisr_ms_ssim_workspace_bytes(n, h, w, len(weights), 0)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(n, dtype=torch.float64, device=dev)
        wv = (ctypes.c_double * len(weights))(*weights)
        hip.check(L.sisr_ms_ssim(hip.ptr(a), hip.ptr(b), n, h, w, float(max_value), wv, len(weights), out.data_ptr(), None,
                                 None, ws.data_ptr(), nbytes, hip.stream()), "sisr_ms_ssim")
    return out.cpu().tolist()


def _host(t):
    import torch
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def eval_output(sr, hr=None, chroma=None, max_value=1, shave=0, want_psnr=True, want_rgb8=False, hr_form=None):
    """The output stage of evaluation in one pass -> (psnr, rgb8), each None when not asked for.
    sr: (N, 3, H, W) RGB, or (N, 1, H, W) Y planes with `chroma` (N, 3, H, W) YCbCr when bytes are wanted (planes 1 and 2 used).
    hr: (N, C, H, W); hr_form 0: RGB, compared on the Y of its clip; hr_form 1: plane 0 is Y (clipped).  None: 0 when sr and hr
    both have three planes and sr is RGB, otherwise 1.
    psnr: N floats, 100 if mse == 0 else 20 log10(max_value / sqrt(mse)) in float64; mse the mean over the pixels at least
    `shave` away from every border of the squared fp32 difference of the Y planes, squared and summed in float64.
    rgb8: (N, H, W, 3) uint8.  Three planes: (clip(x) * 255).round().  One plane: batch_ycbcr_to_rgb of (sr, chroma[:, 1:]), times
    255, rounded and SATURATED to 0 .. 255 (the existing host path's astype(uint8) wraps there).
    If any of the three is a tensor on a HIP device, all go to it and one sisr_eval_output call makes both results (rgb8 is then
    a tensor on that device); anything else takes the host forms (rgb8 a numpy array)."""
    import torch
    if not (want_psnr or want_rgb8):
        return None, None
    if want_psnr and hr is None:
        raise RuntimeError('Need a reference to calculate PSNR.')
    shape = tuple(sr.shape)
    if len(shape) != 4 or shape[1] not in (1, 3):
        raise ValueError(f"eval_output takes an (N, 1|3, H, W) batch; got {shape}")
    n, c, h, w = shape
    if want_psnr:
        hs = tuple(hr.shape)
        if len(hs) != 4 or hs[0] != n or hs[2:] != (h, w) or hs[1] < 1:
            raise ValueError(f"eval_output: hr must be (N, C, H, W) with the batch's N, H, W; got {hs} for {shape}")
        if hr_form is None:
            hr_form = 0 if (c == 3 and hs[1] == 3) else 1
        if hr_form not in (0, 1) or (hr_form == 0 and hs[1] < 3):
            raise ValueError(f"eval_output: hr_form {hr_form!r} does not fit an HR batch of {hs[1]} planes")
        shave = int(shave)
        if shave < 0 or 2 * shave >= min(h, w):
            raise ValueError(f"psnr_shave = {shave} leaves nothing of a {h} x {w} image")
    if want_rgb8 and c == 1:
        if chroma is None or tuple(chroma.shape) != (n, 3, h, w):
            raise ValueError("eval_output: bytes of a one-plane batch need `chroma`, an (N, 3, H, W) YCbCr batch of its size")
    dev = next((t.device for t in (sr, hr, chroma) if isinstance(t, torch.Tensor) and t.is_cuda), None)
    if dev is None:
        values = rgb8 = None
        a = _host(sr).astype(np.float32, copy=False)
        if want_psnr:
            b = _host(hr).astype(np.float32, copy=False)
            ya = batch_rgb_to_ycbcr(a)[:, 0] if c == 3 else standard_image_formatting(a[:, 0])
            yb = batch_rgb_to_ycbcr(b[:, :3])[:, 0] if hr_form == 0 else standard_image_formatting(b[:, 0])
            values = [psnr(ya[i, shave:h - shave, shave:w - shave], yb[i, shave:h - shave, shave:w - shave],
                           max_value=max_value) for i in range(n)]
        if want_rgb8:
            if c == 3:
                v = (standard_image_formatting(a) * 255).round()
            else:
                ch = _host(chroma).astype(np.float32, copy=False)
                v = (batch_ycbcr_to_rgb(np.stack([a[:, 0], ch[:, 1], ch[:, 2]], 1)) * 255).round()
            rgb8 = np.ascontiguousarray(np.clip(np.nan_to_num(v, nan=0.0), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1))
        return values, rgb8
    from . import hip
    L = hip.lib()
    to_dev = lambda t: torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
    a = to_dev(sr)
    b = to_dev(hr) if want_psnr else None
    ch = to_dev(chroma) if want_rgb8 and c == 1 else None
    if n == 0:
        return ([] if want_psnr else None), (torch.empty((0, h, w, 3), dtype=torch.uint8, device=dev) if want_rgb8 else None)
    with torch.cuda.device(dev):
        mse = ws = rgb8 = None
        nbytes = 0
        if want_psnr:
            nbytes = L.sisr_eval_output_workspace_bytes(n, h, w)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            mse = torch.empty(n, dtype=torch.float64, device=dev)
        if want_rgb8:
            rgb8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
        hip.check(L.sisr_eval_output(hip.ptr(a), c, hip.ptr(ch), hip.ptr(b), int(hr_form or 0), b.shape[1] if want_psnr else 1,
                                     n, h, w, shave if want_psnr else 0, None if mse is None else mse.data_ptr(),
                                     None if rgb8 is None else rgb8.data_ptr(), None if ws is None else ws.data_ptr(), nbytes,
                                     hip.stream()), "sisr_eval_output")
    values = None
    if want_psnr:
        values = [100 if m == 0 else float(20 * np.log10(max_value / np.sqrt(m))) for m in mse.cpu().tolist()]
    return values, rgb8


def batch_psnr(sr, hr, max_value=1, shave=0):
    """Per-image Y-PSNR of two (N, C, H, W) batches -> list of N floats, with the argument forms of batch_ssim: C == 3 is clipped
    RGB compared on Y (as y_psnr), C == 1 Y planes (clipped).  `shave` crops that many pixels from every border first (the
    papers' protocol, typically the scale).  If either batch is a tensor on a HIP device both go to the device kernel
    (sisr_eval_output: the squares and their sum in float64); anything else takes the host `psnr` on the cropped Y planes."""
    dev, a, b = _batch_pair("batch_psnr", sr, hr)
    if dev is None:
        n, _, h, w = a.shape
        shave = int(shave)
        if shave < 0 or 2 * shave >= min(h, w):
            raise ValueError(f"psnr_shave = {shave} leaves nothing of a {h} x {w} image")
        if a.shape[1] == 1:  # Y planes as given are clipped, as the device form clips them; C == 3 arrives as the Y of the clip
            a, b = standard_image_formatting(a), standard_image_formatting(b)
        a, b = a[:, 0], b[:, 0]
        return [psnr(a[i, shave:h - shave, shave:w - shave], b[i, shave:h - shave, shave:w - shave], max_value=max_value)
                for i in range(n)]
    return eval_output(a, b, max_value=max_value, shave=shave, hr_form=0 if a.shape[1] == 3 else 1)[0]


def batch_rgb8(sr, chroma=None):
    """The 8-bit image of a batch -> (N, H, W, 3) uint8: `(clip(x) * 255).round()` of an (N, 3, H, W) RGB batch, or of an
    (N, 1, H, W) Y batch with `chroma` (N, 3, H, W; its Cb and Cr) the clipped YCbCr through batch_ycbcr_to_rgb, times 255,
    rounded and saturated to 0 .. 255.  A tensor on the HIP device when an input is one (sisr_eval_output), else numpy."""
    return eval_output(sr, chroma=chroma, want_psnr=False, want_rgb8=True)[1]
