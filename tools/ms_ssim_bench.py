"""The multi-scale SSIM loss term on one GPU: ops.ms_ssim_mean beside the same quantity composed from stock torch ops, and
what it adds to an RCAN train step, in one call.

python tools/ms_ssim_bench.py [--window 1.0] [--rounds 3] [--out profiles/ms_ssim_bench.json]

1. The term alone -- mean MS-SSIM(sr, y), forward + backward to sr -- at 8 x 3 x 512^2 and 32 x 3 x 512^2 (five scales) and
   32 x 1 x 128^2 (four scales): ops.ms_ssim_mean (csrc/ms_ssim.hip, float64 throughout) against the stock composition (per
   scale five grouped 11 x 1 / 1 x 11 conv2d pairs and the pointwise map, avg_pool2d between the scales, pow and prod over
   the scales, autograd backward) in fp32 and in float64 on the same GPU.  The forms alternate window by window (each window
   at least `window` seconds of device time between two device events, after a warm-up of every shape); medians are
   reported.  The HIP value-only call (no gradient: 2 M + 1 of the 3 M + 1 launches) is timed as well.
2. An RCAN x4 train step at 8 tiles of 128^2, with ms_ssim_loss=0.2 and without.
Bytes and float64 operations per call are computed from the shapes (what the algorithm needs, not what was counted).
Prints one JSON line and, with --out, writes it.  Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SHAPES = (((8, 3, 512, 512), 5), ((32, 3, 512, 512), 5), ((32, 1, 128, 128), 4))


def window(fn, seconds):
    """run fn() repeatedly for at least `seconds` of device time -> ms per call"""
    n, total_ms, calls = 1, 0.0, 0
    while total_ms < seconds * 1e3:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= seconds * 1e3:
            return ms / n
        total_ms, calls = ms, n
        n = max(n + 1, int(n * min(10.0, 1.2 * seconds * 1e3 / max(ms, 1e-3))))
    return total_ms / calls


def alternate(fns, seconds, rounds):
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(ts, fns):
            t.append(window(fn, seconds))
    return ts


def taps(dtype):
    x = torch.arange(-5, 6, dtype=torch.float64)
    phi = torch.exp(-0.5 / (1.5 * 1.5) * x * x)
    return (phi / phi.sum()).to(device="cuda", dtype=dtype)


def stock_ms_ssim_mean(x, y, w, weights, data_range=1.0):
    """the term from stock torch ops in the operands' dtype"""
    c = x.shape[1]
    wv, wh = w.view(1, 1, 11, 1).expand(c, 1, 11, 1), w.view(1, 1, 1, 11).expand(c, 1, 1, 11)

    def gauss(t):
        return F.conv2d(F.conv2d(t, wv, groups=c), wh, groups=c)

    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    per = None
    for j, wj in enumerate(weights):
        if j:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
        mx, my, exx, eyy, exy = gauss(x), gauss(y), gauss(x * x), gauss(y * y), gauss(x * y)
        vx, vy, vxy = exx - mx * mx, eyy - my * my, exy - mx * my
        m = (2 * vxy + c2) / (vx + vy + c2)
        if j == len(weights) - 1:
            m = m * ((2 * mx * my + c1) / (mx * mx + my * my + c1))
        t = m.mean(dim=(2, 3)).clamp(min=0) ** wj
        per = t if per is None else per * t
    return per.mean()


def model(shape, levels):
    """what one forward + backward call needs, from the shape, summed over the scales: HBM bytes (scale 0: fp32 operands read
    by the forward, the pooling and the gradient launch, one fp32 gradient written; scales >= 1: float64 operands written once
    and read by the forward, the pooling and the gradient launch, a float64 gradient written and read; every scale: three
    float64 maps written and read; halo re-reads are cache hits and not counted) and float64 multiply-adds (5 x 11 horizontal
    and 5 x 11 vertical taps per window, 3 x 11 + 3 x 11 per pixel in the transposed filter; the pointwise map, the pooling
    and the conversions come on top)"""
    B, C, H, W = shape
    nbytes = fma = pixels = windows = 0
    for j in range(levels):
        h, w = H >> j, W >> j
        pix, win = B * C * h * w, B * C * (h - 10) * (w - 10)
        pixels, windows = pixels + pix, windows + win
        fma += 110 * win + 66 * pix
        nbytes += 2 * 3 * 8 * win
        if j == 0:
            nbytes += 2 * 4 * pix * (3 if levels > 1 else 2) + 4 * pix
        else:
            nbytes += 2 * 8 * pix * (4 if j < levels - 1 else 3) + 2 * 8 * pix
    return {"levels": levels, "bytes": nbytes, "f64_fma": fma, "pixels": pixels, "windows": windows}


def bench_term(shape, levels, args):
    from sisr_amd import ops
    weights = WEIGHTS[:levels]
    g = torch.Generator().manual_seed(8)
    y = torch.rand(shape, generator=g).cuda()
    sr = (y + 0.05 * torch.randn(shape, generator=g).cuda()).requires_grad_(True)
    y64 = y.double()
    sr64 = sr.detach().double().requires_grad_(True)
    w32, w64 = taps(torch.float32), taps(torch.float64)

    def hip_call():
        sr.grad = None
        ops.ms_ssim_mean(sr, y, weights=weights).backward()

    def hip_value_call():
        with torch.no_grad():
            ops.ms_ssim_mean(sr, y, weights=weights)

    def stock32_call():
        sr.grad = None
        stock_ms_ssim_mean(sr, y, w32, weights).backward()

    def stock64_call():
        sr64.grad = None
        stock_ms_ssim_mean(sr64, y64, w64, weights).backward()

    out = {"shape": list(shape), **model(shape, levels)}
    calls = {"hip": hip_call, "hip_value_only": hip_value_call, "stock_fp32": stock32_call, "stock_float64": stock64_call}
    for fn in calls.values():  # every form warmed up: code objects, library algorithm search, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # what the three compute: the same gradient (HIP and stock fp32 against the float64 composition)
    hip_call()
    stock64_call()
    out["hip_gradient_rel_l2_vs_stock_float64"] = float((sr.grad.double() - sr64.grad).norm() / sr64.grad.norm())
    stock32_call()
    out["stock_fp32_gradient_rel_l2_vs_stock_float64"] = float((sr.grad.double() - sr64.grad).norm() / sr64.grad.norm())
    ts = dict(zip(calls, alternate(list(calls.values()), args.window, args.rounds)))
    med = statistics.median
    for k, v in ts.items():
        out[k + "_ms"] = med(v)
        out[k + "_windows_ms"] = v
    out["speedup_over_stock_fp32"] = out["stock_fp32_ms"] / out["hip_ms"]
    out["speedup_over_stock_float64"] = out["stock_float64_ms"] / out["hip_ms"]
    out["hip_tb_per_s"] = out["bytes"] / (out["hip_ms"] * 1e-3) / 1e12
    out["hip_f64_tfma_per_s"] = out["f64_fma"] / (out["hip_ms"] * 1e-3) / 1e12
    return out


def bench_rcan(args):
    import sisr_amd as sisr
    B, S = 8, 128
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(B, 3, S, S, generator=g).cuda(), torch.rand(B, 3, 4 * S, 4 * S, generator=g).cuda()
    hs = {}
    for name, kw in (("l1", {}), ("ms_ssim", {"ms_ssim_loss": 0.2})):
        torch.manual_seed(8)
        hs[name] = sisr.handlers.RCANHandler(device=0, model_save_dir=tempfile.gettempdir(), eval_mode=False, lr=1e-4, scale=4, **kw)
    steps = {k: (lambda h=h: h.train_step(x, y)) for k, h in hs.items()}
    for fn in steps.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = alternate((steps["l1"], steps["ms_ssim"]), args.window, args.rounds)
    med = statistics.median
    return {"batch": B, "lr_size": S, "scale": 4, "l1_step_ms": med(a), "ms_ssim_step_ms": med(b), "l1_step_windows_ms": a,
            "ms_ssim_step_windows_ms": b, "ms_ssim_step_over_l1_step": med(b) / med(a), "added_ms": med(b) - med(a),
            "l1_tiles_per_s": 1e3 * B / med(a), "ms_ssim_tiles_per_s": 1e3 * B / med(b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ms_ssim_bench needs a GPU: nothing here can be measured without one")
    doc = {"metric": "ms_ssim_loss", "device": torch.cuda.get_device_name(0), "term": []}
    for shape, levels in SHAPES:
        doc["term"].append(bench_term(shape, levels, args))
        torch.cuda.empty_cache()
    doc["rcan_x4_step"] = bench_rcan(args)
    line = json.dumps(doc)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
