"""The degradation-consistency loss term on one GPU: ops.degrade_valid (forward + adjoint) beside the same operator composed
from stock torch, and what the term adds to an RCAN train step, in one call.

python tools/consistency_bench.py [--window 1.0] [--rounds 3] [--out profiles/consistency_bench.json]

1. The operator alone -- blur with each sample's 21 x 21 kernel + Pillow's bicubic down-sampling by 4 of a float HR batch at the
   outputs whose footprint lies inside the tile, forward + backward to the input -- at 8 x 3 x 512^2 and 32 x 3 x 256^2 HR:
   ops.degrade_valid (csrc/consistency.hip: one strided correlation with the composed 36 x 36 kernel, float64 accumulation)
   against the stock-torch composition in fp32 on the same GPU: a per-sample grouped conv2d, then the two tap passes as
   strided convolutions, autograd backward.  The forms alternate window by window (each window at least `window` seconds of
   device time between two device events, after a warm-up of every shape); medians and every window are reported, with the
   relative L2 and max-abs errors of both forms, forward and gradient, against the same composition in float64.
2. An RCAN x4 train step at 8 tiles of 128^2, with consistency_loss = 0.1 (kernels and flags in the batch, K composed on the host
   every step) and without.
Multiply-adds per call are computed from the shapes.  Prints one JSON line and, with --out, writes it.  Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = ((8, 3, 512, 512), (32, 3, 256, 256))
SCALE, EDGE = 4, 21
FP64_VECTOR_PEAK_TFLOPS = 78.6


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


def stock_degrade_valid(x, kernels, scale):
    """blur -> horizontal taps -> vertical taps in x's dtype: grouped conv2d, then two strided convolutions, kept outputs only"""
    from sisr_amd import degrade
    B, C, H, W = x.shape
    l = kernels.shape[-1]
    first, taps = degrade.bicubic_interior_taps(scale)
    m = degrade.consistency_margin(scale, l)
    off = scale * m + first - l // 2
    ho, wo = H // scale - 2 * m, W // scale - 2 * m
    t = torch.as_tensor(taps).to(x)
    b = F.conv2d(x.reshape(1, B * C, H, W), kernels.to(x).repeat_interleave(C, 0)[:, None], groups=B * C)
    b = b.reshape(B * C, 1, H - l + 1, W - l + 1)[:, :, :, off:off + scale * (wo - 1) + len(taps)]
    b = F.conv2d(b, t.reshape(1, 1, 1, -1), stride=(1, scale))[:, :, off:off + scale * (ho - 1) + len(taps)]
    return F.conv2d(b, t.reshape(1, 1, -1, 1), stride=(scale, 1)).reshape(B, C, ho, wo)


def random_kernels(B, seed):
    from sisr_amd import degrade
    state = np.random.get_state()
    np.random.seed(seed)
    k = degrade.random_batch_kernel(B, l=EDGE, rate_iso=0.0)  # anisotropic, as OnlineDegrader draws them
    np.random.set_state(state)
    return torch.from_numpy(k).float()


def bench_operator(shape, args):
    from sisr_amd import degrade, ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(8)
    x = torch.rand(shape, generator=g).cuda().requires_grad_(True)
    k = random_kernels(B, 8)
    K = torch.from_numpy(degrade.compose_degradation(k.double().numpy(), SCALE)[0]).cuda()
    n = K.shape[1]
    m = degrade.consistency_margin(SCALE, EDGE)
    ho, wo = H // SCALE - 2 * m, W // SCALE - 2 * m
    go = torch.randn(B, C, ho, wo, generator=g).cuda()
    kd = k.cuda()

    def hip_call():
        x.grad = None
        ops.degrade_valid(x, K, SCALE).backward(go)

    def stock_call():
        x.grad = None
        stock_degrade_valid(x, kd, SCALE).backward(go)

    macs = B * C * ho * wo * n * n
    out = {"shape": list(shape), "scale": SCALE, "blur_edge": EDGE, "composed_edge": n, "margin": m, "outputs": [B, C, ho, wo],
           "mac_forward": macs, "mac_forward_backward": 2 * macs,
           "mac_stock_forward": B * C * ((H - EDGE + 1) * (W - EDGE + 1) * EDGE * EDGE + (H - EDGE + 1) * wo * 16 + ho * wo * 16)}
    calls = {"hip": hip_call, "stock_torch_fp32": stock_call}
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    x64 = x.detach().double().requires_grad_(True)
    y64 = stock_degrade_valid(x64, k.double().cuda(), SCALE)
    y64.backward(go.double())

    def errors(y, grad):
        return {"forward_rel_l2": float((y.double() - y64).norm() / y64.norm()), "forward_max_abs": float((y.double() - y64).abs().max()),
                "gradient_rel_l2": float((grad.double() - x64.grad).norm() / x64.grad.norm()),
                "gradient_max_abs": float((grad.double() - x64.grad).abs().max())}
    hip_call()
    out["hip_error_vs_float64"] = errors(ops.degrade_valid(x, K, SCALE).detach(), x.grad)
    stock_call()
    out["stock_error_vs_float64"] = errors(stock_degrade_valid(x, kd, SCALE).detach(), x.grad)
    del x64, y64
    ts = dict(zip(calls, alternate(list(calls.values()), args.window, args.rounds)))
    for name, v in ts.items():
        out[name + "_ms"] = statistics.median(v)
        out[name + "_windows_ms"] = v
    out["speedup_over_stock_torch_fp32"] = out["stock_torch_fp32_ms"] / out["hip_ms"]
    out["hip_fp64_tflops"] = 2 * out["mac_forward_backward"] / (out["hip_ms"] * 1e-3) / 1e12
    out["hip_share_of_fp64_vector_peak"] = out["hip_fp64_tflops"] / FP64_VECTOR_PEAK_TFLOPS
    return out


def bench_rcan(args):
    import sisr_amd as sisr
    B, S = 8, 128
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(B, 3, S, S, generator=g).cuda(), torch.rand(B, 3, SCALE * S, SCALE * S, generator=g).cuda()
    batch = {"blur_kernels": random_kernels(B, 9), "flips": torch.randint(0, 2, (B, 3), generator=g)}
    hs = {}
    for name, kw in (("l1", {}), ("consistency", {"consistency_loss": 0.1})):
        torch.manual_seed(8)
        hs[name] = sisr.handlers.RCANHandler(device=0, model_save_dir=tempfile.gettempdir(), eval_mode=False, lr=1e-4, scale=SCALE, **kw)
    steps = {"l1": lambda: hs["l1"].train_step(x, y), "consistency": lambda: hs["consistency"].train_step(x, y, **batch)}
    for fn in steps.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = alternate((steps["l1"], steps["consistency"]), args.window, args.rounds)
    med = statistics.median
    return {"batch": B, "lr_size": S, "scale": SCALE, "gamma": 0.1, "l1_step_ms": med(a), "consistency_step_ms": med(b),
            "l1_step_windows_ms": a, "consistency_step_windows_ms": b, "consistency_step_over_l1_step": med(b) / med(a),
            "added_ms": med(b) - med(a), "l1_tiles_per_s": 1e3 * B / med(a), "consistency_tiles_per_s": 1e3 * B / med(b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("consistency_bench needs a GPU: nothing here can be measured without one")
    doc = {"metric": "consistency_loss", "device": torch.cuda.get_device_name(0), "fp64_vector_peak_tflops": FP64_VECTOR_PEAK_TFLOPS,
           "operator": []}
    for shape in SHAPES:
        doc["operator"].append(bench_operator(shape, args))
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
