"""The perceptual (VGG19 feature) loss on one GPU: the HIP criterion beside the same VGG in stock torch.nn, and what it adds to
an RCAN train step, in one call.

python tools/perceptual_bench.py [--batch 8] [--size 512] [--window 1.0] [--rounds 3] [--out profiles/perceptual_bench.json]

1. The criterion alone -- lambda_pixel L1(sr, y) + lambda_per L1(phi(sr), phi(y)), forward + backward to sr -- on `batch`
   images of 3 x size x size: perceptual.PerceptualMechanism against the reference's formulation on torchvision's layer stack
   in stock torch.nn (the same frozen weights, the same GPU), in both memory layouts the stock convs take: contiguous NCHW,
   as the reference runs it, and channels_last.  The three alternate window by window (each window at least
   `window` seconds of device time between two device events, after a warm-up of every shape); medians are reported.
2. An RCAN x4 train step at `batch` tiles of (size / 4)^2, with perceptual=0.01 and without.
3. One more HIP criterion call with every library call between two device events: the time per launch family.
The weights are seeded He-normal tensors written to a temporary file (timing does not depend on their values; the published
file is not needed).  Prints one JSON line and, with --out, writes it.  Fails without a GPU."""
import argparse
import copy
import json
import math
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


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


def seeded_weights(path):
    from sisr_amd import perceptual
    g = torch.Generator().manual_seed(0)
    m = perceptual.VGGFeatureExtractor()
    sd = {}
    for k, v in m.state_dict().items():
        if k.endswith("weight"):
            sd[k] = torch.randn(v.shape, generator=g) * math.sqrt(2.0 / (9 * v.shape[1]))
        else:
            sd[k] = (torch.rand(v.shape, generator=g) * 2 - 1) * 0.05
    torch.save(sd, path)


def vgg_flop(B, S):
    """forward multiply-adds x 2 of the sixteen convs (real channel counts)"""
    from sisr_amd import perceptual
    flop, cin, s = 0.0, 3, S
    for bi, block in enumerate(perceptual.VGG19_54_BLOCKS):
        if bi:
            s //= 2
        for cout in block:
            flop += 2.0 * B * s * s * 9 * cin * cout
            cin = cout
    return flop


def bench_criterion(path, args):
    from sisr_amd import perceptual
    B, S = args.batch, args.size
    crit = perceptual.PerceptualMechanism(lambda_per=0.01)
    perceptual.load_vgg19_weights(crit.vgg_extractor, path)
    crit.cuda()
    ext = crit.vgg_extractor
    g = torch.Generator().manual_seed(8)
    y = torch.rand(B, 3, S, S, generator=g).cuda()
    sr = (y + 0.05 * torch.randn(B, 3, S, S, generator=g).cuda()).requires_grad_(True)

    def hip_call():
        sr.grad = None
        crit(sr, y).backward()

    def stock(stack, layout):  # ref: sr_tools/loss_functions.py:18-22 on feature_extractors/VGGNets.py:127-131
        def call():
            sr.grad = None
            gen = stack(((sr - ext.mean) / ext.std).contiguous(memory_format=layout))
            with torch.no_grad():
                real = stack(((y - ext.mean) / ext.std).contiguous(memory_format=layout))
            (F.l1_loss(sr, y) + 0.01 * F.l1_loss(gen, real)).backward()
        return call

    stock_call = stock(ext.vgg19_54, torch.contiguous_format)
    stock_cl_call = stock(copy.deepcopy(ext.vgg19_54).to(memory_format=torch.channels_last), torch.channels_last)
    calls = (hip_call, stock_call, stock_cl_call)
    for fn in calls:  # every shape warmed up: code objects, weight packing, library algorithm search
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    hs, ss, cs = alternate(calls, args.window, args.rounds)
    med = statistics.median
    # phi(sr) forward + its input gradient + phi(y) forward: three passes of the conv stack, no weight gradients
    tflops = 3 * vgg_flop(B, S) / (med(hs) * 1e-3) / 1e12
    return {"batch": B, "size": S, "hip_ms": med(hs), "stock_ms": med(ss), "hip_windows_ms": hs, "stock_windows_ms": ss,
            "stock_channels_last_ms": med(cs), "stock_channels_last_windows_ms": cs,
            "speedup_over_stock": min(med(ss), med(cs)) / med(hs), "conv_flop_per_call": 3 * vgg_flop(B, S), "hip_conv_tflops": tflops}, hip_call


def families(call):
    """one more HIP criterion call with every library call between two device events"""
    from sisr_amd import hip, ops
    events = {}
    real = hip.lib
    inner = real()

    class Wrap:
        def __getattr__(self, name):
            fn = getattr(inner, name)
            if name.endswith("_bytes") or name.endswith("_parts") or name.endswith("_max"):
                return fn

            def run(*a):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = fn(*a)
                e1.record()
                key = name + (" (bwd)" if ops.IN_BACKWARD else "")
                if name == "sisr_conv3x3_c64":
                    key += " %d->%d @%dx%d" % (a[22], a[23], a[20], a[21])
                events.setdefault(key, []).append((e0, e1))
                return rc
            return run

    wrapped = Wrap()
    hip.lib = lambda: wrapped
    try:
        call()
        torch.cuda.synchronize()
    finally:
        hip.lib = real
    out = [{"call": k, "launches": len(v), "ms": round(sum(a.elapsed_time(b) for a, b in v), 3)} for k, v in events.items()]
    return sorted(out, key=lambda d: -d["ms"])


def bench_rcan(path, args):
    import sisr_amd as sisr
    B, S = args.batch, args.size // 4
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(B, 3, S, S, generator=g).cuda(), torch.rand(B, 3, 4 * S, 4 * S, generator=g).cuda()
    hs = {}
    for name, kw in (("l1", {}), ("perceptual", {"perceptual": 0.01, "perceptual_weights": path})):
        torch.manual_seed(8)
        hs[name] = sisr.handlers.RCANHandler(device=0, model_save_dir=tempfile.gettempdir(), eval_mode=False, lr=1e-4, scale=4, **kw)
    steps = {k: (lambda h=h: h.train_step(x, y)) for k, h in hs.items()}
    for fn in steps.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = alternate((steps["l1"], steps["perceptual"]), args.window, args.rounds)
    med = statistics.median
    return {"batch": B, "lr_size": S, "scale": 4, "l1_step_ms": med(a), "perceptual_step_ms": med(b), "l1_step_windows_ms": a,
            "perceptual_step_windows_ms": b, "perceptual_step_over_l1_step": med(b) / med(a),
            "l1_tiles_per_s": 1e3 * B / med(a), "perceptual_tiles_per_s": 1e3 * B / med(b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512, help="HR edge; the RCAN tiles are size / 4")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perceptual_bench needs a GPU: nothing here can be measured without one")
    doc = {"metric": "perceptual_loss", "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "vgg19_seeded.pth")
        seeded_weights(path)
        doc["criterion"], call = bench_criterion(path, args)
        doc["criterion"]["hip_calls"] = families(call)
        del call
        torch.cuda.empty_cache()
        doc["rcan_x4_step"] = bench_rcan(path, args)
    line = json.dumps(doc)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
