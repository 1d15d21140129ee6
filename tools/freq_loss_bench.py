"""The frequency-domain (FFT L1) loss term on one GPU: ops.spectral_l1 beside the same quantity composed from torch.fft.rfft2,
and what it adds to an RCAN train step, in one call.

python tools/freq_loss_bench.py [--window 1.0] [--rounds 3] [--out profiles/freq_loss_bench.json]

1. The term alone -- mean |Re F| + |Im F| of F = rfft2(sr - y, norm='ortho'), forward + backward to sr -- at 8 x 3 x 512^2,
   32 x 3 x 512^2, 8 x 3 x 384^2, 32 x 1 x 128^2 and 1 x 3 x 1356 x 2040: ops.spectral_l1 (csrc/freq_loss.hip: the DFT as
   matrix products on the fp32 MFMA) against view_as_real(torch.fft.rfft2(sr - y, norm='ortho')).abs().mean() with autograd
   backward, in fp32 on the same GPU.  The forms alternate window by window (each window at least `window` seconds of device
   time between two device events, after a warm-up of every shape); medians and every window are reported.  The HIP
   value-only call (no gradient: three of the five launches, no sign map) is timed as well.
2. An RCAN x4 train step at 8 tiles of 128^2, with freq_loss=0.1 and without.
Floating-point operations per call are computed from the shapes (the dense products as written, and what the kernels
multiply out after their two halvings; not what was counted); the latter is set against the 157.3 TFLOP/s fp32 matrix peak.  Prints one JSON line and, with --out, writes it.  Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

SHAPES = ((8, 3, 512, 512), (32, 3, 512, 512), (8, 3, 384, 384), (32, 1, 128, 128), (1, 3, 1356, 2040))
FP32_MATRIX_PEAK_TFLOPS = 157.3


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


def stock_spectral_l1(sr, y):
    return torch.view_as_real(torch.fft.rfft2(sr - y, norm="ortho")).abs().mean()


def model(shape):
    """what one call needs, from the shape (2 operations per multiply-add).  `dense`: the products as written -- forward, rows 2
    products of [H x W] x [W x Wh] and columns 4 products of [H x H] x [H x Wh]; backward the same counts transposed.
    `executed`: what the kernels multiply out after the two halvings -- rows with K = Wh (the row folded), columns on the
    H / 2 + 1 rows u <= H / 2, the gradient's last product on the Wh columns j <= W / 2."""
    B, C, H, W = shape
    P, Wh, Hh = B * C, W // 2 + 1, H // 2 + 1
    rows, cols = 2 * 2 * P * H * W * Wh, 4 * 2 * P * H * H * Wh
    rows_x, cols_x = 2 * 2 * P * H * Wh * Wh, 4 * 2 * P * Hh * H * Wh
    return {"planes": P, "flop_dense_forward": rows + cols, "flop_dense_forward_backward": 2 * (rows + cols),
            "flop_executed_forward": rows_x + cols_x, "flop_executed_forward_backward": 2 * (rows_x + cols_x),
            "workspace_bytes": 2 * 4 * P * H * Wh + P * H * Wh}


def bench_term(shape, args):
    from sisr_amd import ops
    g = torch.Generator().manual_seed(8)
    y = torch.rand(shape, generator=g).cuda()
    sr = (y + 0.05 * torch.randn(shape, generator=g).cuda()).requires_grad_(True)

    def hip_call():
        sr.grad = None
        ops.spectral_l1(sr, y).backward()

    def hip_value_call():
        with torch.no_grad():
            ops.spectral_l1(sr, y)

    def stock_call():
        sr.grad = None
        stock_spectral_l1(sr, y).backward()

    out = {"shape": list(shape), **model(shape)}
    calls = {"hip": hip_call, "hip_value_only": hip_value_call, "stock_fft_fp32": stock_call}
    for fn in calls.values():  # every form warmed up: code objects, FFT plans, the table cache, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    # what the two compute: value and gradient of the HIP form against torch.fft in float64 on the same device, and the stock
    # fp32 form against the same (its gradient can carry spurious signs at the self-conjugate bins: see DESIGN.md 6r)
    sr64 = sr.detach().double().requires_grad_(True)
    v64 = stock_spectral_l1(sr64, y.double())
    v64.backward()
    hip_call()
    with torch.no_grad():
        vh = ops.spectral_l1(sr, y)
    out["hip_value_rel_err_vs_fft_float64"] = abs(float(vh) - float(v64.detach())) / float(v64.detach())
    out["hip_gradient_rel_l2_vs_fft_float64"] = float((sr.grad.double() - sr64.grad).norm() / sr64.grad.norm())
    stock_call()
    out["stock_fp32_gradient_rel_l2_vs_fft_float64"] = float((sr.grad.double() - sr64.grad).norm() / sr64.grad.norm())
    del sr64, v64
    ts = dict(zip(calls, alternate(list(calls.values()), args.window, args.rounds)))
    med = statistics.median
    for k, v in ts.items():
        out[k + "_ms"] = med(v)
        out[k + "_windows_ms"] = v
    out["speedup_over_stock_fft_fp32"] = out["stock_fft_fp32_ms"] / out["hip_ms"]
    sec = out["hip_ms"] * 1e-3
    out["hip_executed_tflops"] = out["flop_executed_forward_backward"] / sec / 1e12  # what the matrix pipe did
    out["hip_share_of_fp32_matrix_peak"] = out["hip_executed_tflops"] / FP32_MATRIX_PEAK_TFLOPS
    out["hip_dense_equivalent_tflops"] = out["flop_dense_forward_backward"] / sec / 1e12
    out["hip_value_only_executed_tflops"] = out["flop_executed_forward"] / (out["hip_value_only_ms"] * 1e-3) / 1e12
    return out


def bench_rcan(args):
    import sisr_amd as sisr
    B, S = 8, 128
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(B, 3, S, S, generator=g).cuda(), torch.rand(B, 3, 4 * S, 4 * S, generator=g).cuda()
    hs = {}
    for name, kw in (("l1", {}), ("freq", {"freq_loss": 0.1})):
        torch.manual_seed(8)
        hs[name] = sisr.handlers.RCANHandler(device=0, model_save_dir=tempfile.gettempdir(), eval_mode=False, lr=1e-4, scale=4, **kw)
    steps = {k: (lambda h=h: h.train_step(x, y)) for k, h in hs.items()}
    for fn in steps.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = alternate((steps["l1"], steps["freq"]), args.window, args.rounds)
    med = statistics.median
    return {"batch": B, "lr_size": S, "scale": 4, "l1_step_ms": med(a), "freq_step_ms": med(b), "l1_step_windows_ms": a,
            "freq_step_windows_ms": b, "freq_step_over_l1_step": med(b) / med(a), "added_ms": med(b) - med(a),
            "l1_tiles_per_s": 1e3 * B / med(a), "freq_tiles_per_s": 1e3 * B / med(b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("freq_loss_bench needs a GPU: nothing here can be measured without one")
    doc = {"metric": "freq_loss", "device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK_TFLOPS,
           "term": []}
    for shape in SHAPES:
        doc["term"].append(bench_term(shape, args))
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
