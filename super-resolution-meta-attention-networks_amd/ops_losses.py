"""Loss terms on the HIP path: L1, MSE, mean SSIM (csrc/ssim_loss.hip), multi-scale SSIM (csrc/ms_ssim.hip) and the
spectral L1 (csrc/freq_loss.hip).  Each node computes its value and, in the same call, the gradient it will return.
degrade_valid (csrc/consistency.hip) is the one operator here that returns a map: the degradation of a float image; its node,
with the adjoint kernel as its backward, is degrade.DegradeValid, beside the host mathematics it depends on.
The nodes have one differentiable input and no gradient buffers of their own, so they use nothing of ops.py's core; ops
re-exports the operators."""
import collections
import ctypes

import torch
from torch.autograd import Function

from . import degrade, hip
# the default weights (Wang et al. 2003, as given: they sum to 1.0001) and the checks of the weights and of the image size,
# shared with the host form
from .metrics import MS_SSIM_WEIGHTS, ms_ssim_check_size, ms_ssim_weights


# ----------------------------------------------------------------------------- L1 loss
class _L1Loss(Function):
    @staticmethod
    def forward(ctx, a, b, rounded_once=False):
        a, b = a.contiguous(), b.contiguous()
        if a.shape != b.shape:
            raise RuntimeError(f"l1_loss shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
        L = hip.lib()
        loss = torch.empty((), device=a.device, dtype=torch.float32)
        grad = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        fn, nbytes = ((L.sisr_l1_loss_mean, L.sisr_l1_loss_mean_workspace_bytes()) if rounded_once else
                      (L.sisr_l1_loss, L.sisr_l1_loss_workspace_bytes()))
        ws = hip.workspace(a.device, nbytes)
        hip.check(fn(hip.ptr(a), hip.ptr(b), a.numel(), hip.ptr(loss), hip.ptr(grad), hip.ptr(ws), hip.stream()),
                  "sisr_l1_loss")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, go):
        (grad,) = ctx.saved_tensors
        return grad * go, None, None


def l1_loss(a, b, rounded_once=False):
    """mean |a - b|.  rounded_once: the sums are kept in double and divided by n, so the value is the mean rounded to fp32 once;
    otherwise an fp32 sum times a rounded 1 / n (up to 1.5 fp32 units further off).  The gradient is the same either way."""
    return _L1Loss.apply(a, b, rounded_once)


# ----------------------------------------------------------------------------- mean SSIM (csrc/ssim_loss.hip)
SSIM_WINDOW = 11  # the Gaussian window's side: the smallest image side the loss term takes


def _value_and_grad(ctx, sr, y, data_range, want_grad, entry, ws_args=(), args=()):
    """The forward half of a node whose entry point computes the fp32 mean and, in the same call, its gradient with respect to
    `sr` when `sr` needs one (want_grad: torch.is_grad_enabled() at the call); the gradient is saved and backward returns
    grad * go.  `entry` names the entry point; `ws_args` go between (planes, H, W) and want_grad of its workspace query, `args`
    between data_range and `value` of the call."""
    sr, y = sr.contiguous(), y.contiguous()
    B, C, H, W = sr.shape
    L = hip.lib()
    value = torch.empty((), device=sr.device, dtype=torch.float32)
    grad = torch.empty_like(sr) if want_grad and ctx.needs_input_grad[0] else None
    nbytes = getattr(L, entry + "_workspace_bytes")(B * C, H, W, *ws_args, int(grad is not None))
    ws = hip.workspace(sr.device, nbytes)
    hip.check(getattr(L, entry)(hip.ptr(sr), hip.ptr(y), B * C, H, W, float(data_range), *args, hip.ptr(value), hip.ptr(grad),
                                hip.ptr(ws), nbytes, hip.stream()), entry)
    ctx.save_for_backward(grad)
    return value


class _SsimMean(Function):
    @staticmethod
    def forward(ctx, sr, y, data_range, want_grad):
        return _value_and_grad(ctx, sr, y, data_range, want_grad, "sisr_ssim_loss")

    @staticmethod
    def backward(ctx, go):
        (grad,) = ctx.saved_tensors
        return grad * go, None, None, None


def _ssim_operands(name, sr, y, sized):
    """The operand checks of ssim_mean and ms_ssim_mean, in their order: two 4-D batches of one shape, the form's own size
    check `sized(hw)` (whose result is returned), a batch that is not empty, fp32 tensors on a device, a target that takes no
    gradient."""
    if sr.dim() != 4 or sr.shape != y.shape:
        raise RuntimeError(f"{name} takes two (B, C, H, W) batches of one shape; got {tuple(sr.shape)} and {tuple(y.shape)}")
    out = sized(sr.shape[2:])
    if sr.numel() == 0:
        raise RuntimeError(f"{name}: empty batch {tuple(sr.shape)}")
    hip.ptr(sr), hip.ptr(y)  # raises on CPU or non-fp32 tensors: there is no CPU path
    if y.requires_grad:
        raise RuntimeError(f"{name}: the target takes no gradient; detach it")
    return out


def ssim_mean(sr, y, data_range=1.0):
    """Mean SSIM over all (H - 10) x (W - 10) windows of all B * C planes of two (B, C, H, W) fp32 batches: Gaussian window
    (11 taps, sigma 1.5), population covariance, every plane as given (no clipping, no Y conversion), float64 statistics, the
    value rounded to fp32 once.  The gradient goes to `sr` only and is computed with the value."""
    def sized(hw):
        if min(hw) < SSIM_WINDOW:
            raise ValueError(f"ssim_mean: the {SSIM_WINDOW} x {SSIM_WINDOW} window exceeds the image extent {tuple(hw)}; "
                             f"both sides must be at least {SSIM_WINDOW}")

    _ssim_operands("ssim_mean", sr, y, sized)
    # needs_input_grad is set under no_grad as well (run_eval(request_loss=True)): the gradient launch and its maps are skipped there
    return _SsimMean.apply(sr, y, data_range, torch.is_grad_enabled())


class _MsSsimMean(Function):
    """_SsimMean bound to sisr_ms_ssim, with the scale weights and no per-plane output"""

    @staticmethod
    def forward(ctx, sr, y, data_range, weights, want_grad):
        wv = (ctypes.c_double * len(weights))(*weights)  # host memory, read by the call and not kept
        return _value_and_grad(ctx, sr, y, data_range, want_grad, "sisr_ms_ssim", (len(weights),), (wv, len(weights), None))

    @staticmethod
    def backward(ctx, go):
        (grad,) = ctx.saved_tensors
        return grad * go, None, None, None, None


def ms_ssim_mean(sr, y, data_range=1.0, weights=MS_SSIM_WEIGHTS):
    """Mean over all B * C planes of the multi-scale SSIM of two (B, C, H, W) fp32 batches: per plane prod_j c_j^w_j with c_j
    the mean contrast-structure term A2 / B2 of scale j (full SSIM at the last), scale j + 1 = F.avg_pool2d(scale j, 2), the
    window of ssim_mean on every scale, every plane as given; exactly 0 for a plane with a c_j <= 0 (whatever that scale's
    weight, 0 included).  Float64 throughout, the
    value rounded to fp32 once.  The gradient goes to `sr` only and is computed with the value."""
    def sized(hw):
        w = ms_ssim_weights(weights)
        ms_ssim_check_size("ms_ssim_mean", hw, len(w))
        return w

    weights = _ssim_operands("ms_ssim_mean", sr, y, sized)
    # needs_input_grad is set under no_grad as well (run_eval(request_loss=True)): the gradient launches and the maps are skipped there
    return _MsSsimMean.apply(sr, y, data_range, weights, torch.is_grad_enabled())


# ----------------------------------------------------------------------------- spectral L1 (csrc/freq_loss.hip)
SPECTRAL_MIN_SIDE, SPECTRAL_MAX_SIDE = 2, 4096
SPECTRAL_TABLE_SLOTS = 8  # (H, W) pairs kept per device: training uses one, validation images vary in size
_spectral_tables = {}     # device index -> OrderedDict((H, W) -> the four DFT tables in one fp32 tensor), least recent first
_spectral_held = {}       # device index -> {(H, W): tables a captured graph reads}: never evicted


def spectral_tables(device, H, W):
    """Ch, Sh (H x H), Cw, Sw ((W // 2 + 1) x W) of sisr_freq_loss, in that order in one flat fp32 tensor on `device`; built by
    the table kernel on a miss and kept in a per-device LRU cache (tables that a captured graph reads are kept for good).  A miss needs an allocation, so it cannot happen while the
    stream is capturing: run the operator once eagerly at that shape first (handlers._graphed_step's warm-up pass does)."""
    cache = _spectral_tables.setdefault(device.index, collections.OrderedDict())
    held = _spectral_held.setdefault(device.index, {})
    capturing = torch.cuda.is_current_stream_capturing()
    t = held.get((H, W))
    if t is not None:
        return t
    t = cache.get((H, W))
    if t is not None:
        if capturing:  # a captured graph keeps the address: this entry leaves the LRU list for good
            held[(H, W)] = cache.pop((H, W))
        else:
            cache.move_to_end((H, W))
        return t
    if capturing:
        raise RuntimeError(f"spectral_l1: the DFT tables of a {H} x {W} image are not cached and cannot be built while the "
                           f"stream is capturing; call it once eagerly at this shape before the capture")
    L = hip.lib()
    t = torch.empty(L.sisr_freq_loss_table_bytes(H, W) // 4, device=device, dtype=torch.float32)
    hip.check(L.sisr_freq_loss_tables(H, W, hip.ptr(t), hip.stream()), "sisr_freq_loss_tables")
    cache[(H, W)] = t
    while len(cache) > SPECTRAL_TABLE_SLOTS:
        cache.popitem(last=False)
    return t


class _SpectralL1(Function):
    @staticmethod
    def forward(ctx, sr, y, want_grad):
        sr, y = sr.contiguous(), y.contiguous()
        B, C, H, W = sr.shape
        L = hip.lib()
        tables = spectral_tables(sr.device, H, W)
        value = torch.empty((), device=sr.device, dtype=torch.float32)
        grad = torch.empty_like(sr) if want_grad and ctx.needs_input_grad[0] else None
        nbytes = L.sisr_freq_loss_workspace_bytes(B * C, H, W, int(grad is not None))
        ws = hip.workspace(sr.device, nbytes)
        hip.check(L.sisr_freq_loss(hip.ptr(sr), hip.ptr(y), B * C, H, W, hip.ptr(tables), hip.ptr(value), hip.ptr(grad),
                                   hip.ptr(ws), nbytes, hip.stream()), "sisr_freq_loss")
        ctx.save_for_backward(grad)
        return value

    @staticmethod
    def backward(ctx, go):
        (grad,) = ctx.saved_tensors
        return grad * go, None, None


def spectral_l1(sr, y):
    """Mean of |Re F| and |Im F| over F = rfft2(sr - y, norm='ortho') of two (B, C, H, W) fp32 batches: the mean of
    view_as_real(F).abs(), the structurally zero imaginary parts counted.  The transform runs as matrix products on the fp32
    MFMA, the sums in float64 in a fixed order, the value rounded to fp32 once.  The gradient goes to `sr` only, takes
    sign(0) = 0 and is computed with the value."""
    if sr.dim() != 4 or sr.shape != y.shape:
        raise RuntimeError(f"spectral_l1 takes two (B, C, H, W) batches of one shape; got {tuple(sr.shape)} and {tuple(y.shape)}")
    if sr.numel() == 0:
        raise ValueError(f"spectral_l1: empty batch {tuple(sr.shape)}")
    if min(sr.shape[2:]) < SPECTRAL_MIN_SIDE or max(sr.shape[2:]) > SPECTRAL_MAX_SIDE:
        raise ValueError(f"spectral_l1: image extent {tuple(sr.shape[2:])} is outside the supported sides "
                         f"[{SPECTRAL_MIN_SIDE}, {SPECTRAL_MAX_SIDE}]")
    hip.ptr(sr), hip.ptr(y)  # raises on CPU or non-fp32 tensors: there is no CPU path
    if y.requires_grad:
        raise RuntimeError("spectral_l1: the target takes no gradient; detach it")
    # needs_input_grad is set under no_grad as well (run_eval(request_loss=True)): the gradient launches and the sign map are skipped there
    return _SpectralL1.apply(sr, y, torch.is_grad_enabled())


# ----------------------------------------------------------------------------- blur + bicubic down-sampling of a float image
def degrade_valid_tile(backward=False):
    """Edge of a workgroup's tile of sisr_degrade_valid_fwd (LR outputs) or, backward, of sisr_degrade_valid_bwd (HR pixels)."""
    return hip.lib().sisr_degrade_valid_tile(int(bool(backward)))


def degrade_valid(x, K, scale):
    """The LR image the degradation pipeline would make of the float HR tiles x (B, C, s h, s w) -- blur with each sample's
    kernel, then Pillow's bicubic down-sampling by s = `scale` -- without its 8-bit roundings, at the outputs whose whole
    footprint lies inside the tile: (B, C, h - 2m, w - 2m), m = degrade.consistency_margin(scale, l), the map to compare with
    lr[:, :, m:h - m, m:w - m].  K: the composed kernels (B, n, n) of degrade.compose_degradation, float64 on x's device
    (a tensor elsewhere or of another float type is converted); it takes no gradient.  One launch forward, one (the adjoint, a
    gather) backward; float64 accumulation, so both are the fp32 numbers nearest the exact sums."""
    if x.dim() != 4 or K.dim() != 3 or K.shape[1] != K.shape[2] or K.shape[0] != x.shape[0]:
        raise RuntimeError(f"degrade_valid takes x (B, C, H, W) and K (B, n, n); got {tuple(x.shape)} and {tuple(K.shape)}")
    if x.numel() == 0:
        raise ValueError(f"degrade_valid: empty batch {tuple(x.shape)}")
    scale = int(scale)
    l, m, off = degrade.consistency_geometry(scale, K.shape[1])
    H, W = x.shape[2:]
    if H % scale or W % scale:
        raise ValueError(f"degrade_valid: the image extent {(H, W)} is not a multiple of the scale {scale}")
    h, w = H // scale, W // scale
    if h <= 2 * m or w <= 2 * m:
        raise ValueError(f"degrade_valid: no output of a {h} x {w} LR tile keeps its footprint inside the {H} x {W} HR tile at "
                         f"scale {scale} with a {l} x {l} blur kernel: both LR sides must exceed 2 m = {2 * m}")
    hip.ptr(x)  # raises on CPU or non-fp32 tensors: there is no CPU path
    if K.requires_grad:
        raise RuntimeError("degrade_valid: the composed kernel takes no gradient; detach it")
    K = K.to(device=x.device, dtype=torch.float64).contiguous()
    return degrade.DegradeValid.apply(x, K, scale, off, h - 2 * m, w - 2 * m)


# ----------------------------------------------------------------------------- MSE loss
class _MSELoss(Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        if a.shape != b.shape:
            raise RuntimeError(f"mse_loss shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
        L = hip.lib()
        pa, pb = hip.ptr(a), hip.ptr(b)  # (refuses CPU tensors before anything touches a device)
        loss = torch.empty((), device=a.device, dtype=torch.float32)
        grad = torch.empty_like(a) if ctx.needs_input_grad[0] else None
        ws = hip.workspace(a.device, L.sisr_mse_loss_workspace_bytes())
        hip.check(L.sisr_mse_loss(pa, pb, a.numel(), hip.ptr(loss), hip.ptr(grad), hip.ptr(ws),
                                  hip.stream()), "sisr_mse_loss")
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, go):
        (grad,) = ctx.saved_tensors
        return grad * go, None


def mse_loss(a, b):
    return _MSELoss.apply(a, b)
