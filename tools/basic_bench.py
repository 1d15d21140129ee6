"""SRCNN / VDSR on one GPU: the HIP path beside the same architecture in stock torch.nn modules, in one call.

python tools/basic_bench.py [--batch 32] [--size 128] [--window 1.0] [--rounds 3] [--nets srcnn,vdsr]

For each net: one train step (forward + MSE + backward + Adam; VDSR with its gradient clip) and the forward alone, on
`batch` tiles of 1 x size x size.  The two versions alternate, window by window (each window at least `window` seconds of
device time between two device events, after a warm-up of every shape), and the median window is reported.  Also: the time of
every launch family of one HIP SRCNN step (device events around each library call, one extra step) and the achieved fp32
TFLOP/s of the 5 x 5 64 -> 32 MFMA conv against the 157.3 TFLOP/s matrix peak.  Prints one JSON line.  Fails without a GPU.
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/basic_bench.py --nets srcnn --steps-only 20`."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
from torch import nn  # noqa: E402
import torch.nn.functional as F  # noqa: E402

FP32_MATRIX_PEAK_TFLOPS = 157.3


class StockNet(nn.Module):
    """the reference's SRCNN / VDSR in plain torch.nn (ref: basic/architectures.py:6-77)"""

    def __init__(self, kernels, channels, residual):
        super().__init__()
        self.convs = nn.ModuleList(nn.Conv2d(channels[i], channels[i + 1], k, padding=k // 2) for i, k in enumerate(kernels))
        self.residual = residual

    def forward(self, x):
        t = x
        for i, c in enumerate(self.convs):
            t = c(t)
            if i != len(self.convs) - 1:
                t = F.relu(t)
        return t + x if self.residual else t


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


def alternate(a, b, seconds, rounds):
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(a, seconds))
        tb.append(window(b, seconds))
    return ta, tb


def bench_net(name, args):
    import sisr_amd as sisr
    B, S = args.batch, args.size
    torch.manual_seed(8)
    h = sisr.available_models[name](device=0, model_save_dir="/tmp", eval_mode=False, lr=1e-4)
    kernels = [m.kernel_size[0] for m in h.net.layer_dict.values()]
    channels = [1] + [m.out_channels for m in h.net.layer_dict.values()]
    torch.manual_seed(8)
    stock = StockNet(kernels, channels, name == "vdsr").cuda()
    opt = torch.optim.Adam(stock.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(B, 1, S, S, generator=g).cuda(), torch.rand(B, 1, S, S, generator=g).cuda()

    def hip_step():
        h.train_step(x, y)

    def stock_step():
        opt.zero_grad(set_to_none=True)
        F.mse_loss(stock(x), y).backward()
        if h.grad_clip is not None:
            nn.utils.clip_grad_norm_(stock.parameters(), h.grad_clip)
        opt.step()

    def hip_fwd():
        with torch.no_grad():
            h.net(x)

    def stock_fwd():
        with torch.no_grad():
            stock(x)

    for fn in (hip_step, stock_step, hip_fwd, stock_fwd):  # every shape warmed up: code objects, library algorithm search
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    hs, ss = alternate(hip_step, stock_step, args.window, args.rounds)
    hf, sf = alternate(hip_fwd, stock_fwd, args.window, args.rounds)
    med = statistics.median
    return {"batch": B, "size": S, "hip_step_ms": med(hs), "stock_step_ms": med(ss), "hip_forward_ms": med(hf),
            "stock_forward_ms": med(sf), "hip_step_windows_ms": hs, "stock_step_windows_ms": ss,
            "hip_tiles_per_s": 1e3 * B / med(hs), "stock_tiles_per_s": 1e3 * B / med(ss),
            "step_speedup_over_stock": med(ss) / med(hs), "forward_speedup_over_stock": med(sf) / med(hf)}, h


def families(h, args):
    """one more eager SRCNN / VDSR step with every library call between two device events"""
    from sisr_amd import hip, ops
    g = torch.Generator().manual_seed(8)
    x = torch.rand(args.batch, 1, args.size, args.size, generator=g).cuda()
    y = torch.rand(args.batch, 1, args.size, args.size, generator=g).cuda()
    events = {}
    real = hip.lib
    inner = real()

    class Wrap:
        def __getattr__(self, name):
            fn = getattr(inner, name)
            if name.endswith("_bytes") or name.endswith("_parts") or name.endswith("_max"):
                return fn

            def call(*a):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(*a)
                e1.record()
                events.setdefault(name + (" (bwd)" if ops.IN_BACKWARD else ""), []).append((e0, e1))
                return rc
            return call

    wrapped = Wrap()
    hip.lib = lambda: wrapped
    side, ops.WGRAD_SIDE_STREAM = ops.WGRAD_SIDE_STREAM, False
    try:
        h.train_step(x, y)
        torch.cuda.synchronize()
    finally:
        hip.lib, ops.WGRAD_SIDE_STREAM = real, side
    out = [{"call": k, "launches": len(v), "ms_per_step": round(sum(a.elapsed_time(b) for a, b in v), 3)} for k, v in events.items()]
    return sorted(out, key=lambda d: -d["ms_per_step"])


def conv5x5(args):
    """the 5 x 5 64 -> 32 conv alone: forward, input gradient and weight gradient launches"""
    from sisr_amd import hip, ops
    B, S = args.batch, args.size
    L = hip.lib()
    g = torch.Generator().manual_seed(8)
    x = torch.rand(B, 64, S, S, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    dy = torch.rand(B, 32, S, S, generator=g).cuda().contiguous(memory_format=torch.channels_last)
    w = (torch.rand(32, 64, 5, 5, generator=g) - 0.5).cuda()
    b = torch.zeros(32).cuda()
    pf, pd = ops.pack_convk(w)
    y, dx, dw, db = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w), torch.empty_like(b)
    nb = L.sisr_wgradk_mfma_workspace_bytes(B, S, S, 5, 64, 32)
    ws = hip.workspace(x.device, nb)
    flop = 2.0 * B * S * S * 64 * 32 * 25
    runs = {"forward": lambda: ops.convk_mfma(x, pf, b, 32, y, B, S, S, 5, 64, 32, relu=True),
            "input_gradient": lambda: ops.convk_mfma(dy, pd, None, 0, dx, B, S, S, 5, 32, 64, in_mask=y),
            "weight_gradient": lambda: hip.check(L.sisr_wgradk_mfma(hip.ptr(x), hip.ptr(dy), hip.ptr(y), hip.ptr(dw), hip.ptr(db),
                                                                    B, S, S, 5, 32, 64, 32, 64, hip.ptr(ws), nb, hip.stream()),
                                                 "sisr_wgradk_mfma")}
    out = {}
    for k, fn in runs.items():
        for _ in range(3):
            fn()
        ms = window(fn, args.window)
        out[k] = {"ms": ms, "tflops": flop / (ms * 1e-3) / 1e12, "share_of_fp32_matrix_peak": flop / (ms * 1e-3) / 1e12 / FP32_MATRIX_PEAK_TFLOPS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--nets", default="srcnn,vdsr")
    ap.add_argument("--steps-only", type=int, default=0, metavar="N",
                    help="run N HIP train steps of each net and nothing else: the target of `rocprofv3 --kernel-trace --stats`")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("basic_bench needs a GPU: nothing here can be measured without one")
    if args.steps_only:
        import sisr_amd as sisr
        for name in args.nets.split(","):
            torch.manual_seed(8)
            h = sisr.available_models[name](device=0, model_save_dir="/tmp", eval_mode=False, lr=1e-4)
            g = torch.Generator().manual_seed(8)
            x = torch.rand(args.batch, 1, args.size, args.size, generator=g).cuda()
            y = torch.rand(args.batch, 1, args.size, args.size, generator=g).cuda()
            for _ in range(args.steps_only):
                h.train_step(x, y)
            torch.cuda.synchronize()
        print(json.dumps({"metric": "basic_steps_only", "steps": args.steps_only, "nets": args.nets}))
        return
    doc = {"metric": "basic_train_step", "device": torch.cuda.get_device_name(0)}
    for name in args.nets.split(","):
        doc[name], h = bench_net(name, args)
        doc[name]["hip_step_calls"] = families(h, args)
    doc["conv5x5_64_32"] = conv5x5(args)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
