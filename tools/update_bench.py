"""The update step on one GPU: gradient clipping by clip_grad_norm_ beside the clip fused into optim.FlatAdam's pass, the
weight average (EMA) inside that pass beside one made with torch._foreach_lerp_, decoupled weight decay, and what the average
adds to an RCAN train step, in one call.

python tools/update_bench.py [--window 0.5] [--rounds 3] [--out profiles/update_bench.json]

1. The parameter set of a full-depth QRCAN x4 (its ~2 400 tensors in FlatAdam's arenas, gradients filled from a seed and
   sitting in the gradient arena, as after a backward pass), five forms of one update:
     clip_torch      nn.utils.clip_grad_norm_ + FlatAdam.step()        (grad_clip as the handlers run it without fused_clip)
     clip_fused      FlatAdam(max_norm).step()                         (fused_clip=True)
     fused_ema       FlatAdam(max_norm, ema_decay).step()
     foreach_ema     FlatAdam(max_norm).step() + torch._foreach_lerp_ over the parameter tensors
     fused_decay     FlatAdam(max_norm, weight_decay).step()
   Stream time: the forms alternate window by window (each window at least `window` seconds between two device events,
   after a warm-up of every form); medians are reported.  Where the host issues slower than the device executes, this is
   the host's pace.  Host time: the wall time the host needs to ISSUE one update (no synchronisation inside; the queue is
   drained before and after), median over the rounds.  Device time: the same update captured once into a hipGraph (the
   step never synchronises, so it can be) and replayed back to back in the same alternating windows -- the launches
   without the host between them.
   Bytes per update from the arena length (what the algorithm needs): 4 per float for the norm pass, 28 for Adam (p, g, m, v
   read, p, m, v written), 8 more with the average; achieved bytes / s against the HBM figures of the MI355X
   microarchitecture guide (8.0 TB/s spec, 6.29 TB/s measured float4 copy).
2. An RCAN x4 train step at 8 tiles of 128^2, with ema_decay=0.999 and without.
Prints one JSON line and, with --out, writes it.  Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29
MAX_NORM, EMA_DECAY, WEIGHT_DECAY = 0.1, 0.999, 1e-4


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


def captured(fn):
    """fn() captured into a graph -> its replay"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def host_ms(fn, calls=5):
    """wall time to issue one fn(), the stream empty before the first call and drained after the last"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return 1e3 * (t1 - t0) / calls


def make_form(shapes, seed, **options):
    """fresh parameters of the given shapes in a FlatAdam with `options`, the gradient arena filled from the seed and every
    .grad a view of it (no gather copy in step(): the state after a backward pass whose kernels write into the arena)"""
    from sisr_amd.optim import FlatAdam
    gen = torch.Generator(device="cuda").manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen) * 0.05) for s in shapes]
    opt = FlatAdam(ps, lr=1e-4, **options)
    opt.flat_g.copy_(torch.randn(opt.total, device="cuda", generator=gen) * 1e-3)
    pad = torch.ones(opt.total, dtype=torch.bool, device="cuda")
    for p in ps:
        pad[opt.offsets[p]:opt.offsets[p] + p.numel()] = False
        p.grad = opt.grad_views[p]
    opt.flat_g[pad] = 0.0
    return ps, opt


def bench_update(args):
    import sisr_amd as sisr
    net = sisr.architectures.QRCAN(scale=4, n_feats=64, style="standard", num_metadata=10, include_q_layer=True)
    shapes = [tuple(p.shape) for p in net.parameters() if p.requires_grad]
    del net
    forms = {}
    ps, opt = make_form(shapes, 8)
    forms["clip_torch"] = lambda ps=ps, opt=opt: (torch.nn.utils.clip_grad_norm_(ps, MAX_NORM), opt.step())
    ps, opt = make_form(shapes, 8, max_norm=MAX_NORM)
    total = opt.total
    forms["clip_fused"] = opt.step
    ps, opt = make_form(shapes, 8, max_norm=MAX_NORM, ema_decay=EMA_DECAY)
    forms["fused_ema"] = opt.step
    ps, opt = make_form(shapes, 8, max_norm=MAX_NORM)
    avg = [p.detach().clone() for p in ps]
    datas = [p.data for p in ps]
    forms["foreach_ema"] = lambda opt=opt, avg=avg, datas=datas: (opt.step(), torch._foreach_lerp_(avg, datas, 1.0 - EMA_DECAY))
    ps, opt = make_form(shapes, 8, max_norm=MAX_NORM, weight_decay=WEIGHT_DECAY)
    forms["fused_decay"] = opt.step
    for fn in forms.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    med = statistics.median
    dev = dict(zip(forms, alternate(list(forms.values()), args.window, args.rounds)))
    host = {k: [host_ms(fn) for _ in range(max(args.rounds, 3))] for k, fn in forms.items()}
    try:
        replays = {k: captured(fn) for k, fn in forms.items()}
        for fn in replays.values():
            fn()
        torch.cuda.synchronize()
        graph = dict(zip(replays, alternate(list(replays.values()), args.window, args.rounds)))
    except Exception as e:  # the capture is a measuring device only: say so and keep the other figures
        graph, out_error = None, "%s: %s" % (type(e).__name__, e)
    bytes_per_float = {"clip_torch": None, "clip_fused": 4 + 28, "fused_ema": 4 + 28 + 8, "foreach_ema": None, "fused_decay": 4 + 28}
    out = {"tensors": len(shapes), "arena_floats": total, "max_norm": MAX_NORM, "ema_decay": EMA_DECAY,
           "weight_decay": WEIGHT_DECAY, "hbm_spec_tb_per_s": HBM_SPEC_TBS, "hbm_copy_tb_per_s": HBM_COPY_TBS, "forms": {}}
    for k in forms:
        row = {"stream_ms": med(dev[k]), "stream_windows_ms": dev[k], "host_ms": med(host[k]), "host_rounds_ms": host[k]}
        if graph is None:
            row["device_ms"] = "not measured (graph capture failed: %s)" % out_error
        else:
            row["device_ms"], row["device_windows_ms"] = med(graph[k]), graph[k]
            if bytes_per_float[k] is not None:
                row["bytes"] = bytes_per_float[k] * total
                row["tb_per_s"] = row["bytes"] / (row["device_ms"] * 1e-3) / 1e12
                row["fraction_of_hbm_copy_rate"] = row["tb_per_s"] / HBM_COPY_TBS
            row["bound"] = ("host: issuing the update takes longer than the device needs for it" if row["host_ms"] > row["device_ms"]
                            else "device: HBM traffic and launch boundaries")
        out["forms"][k] = row
    f = out["forms"]
    for key in ("stream_ms", "host_ms") + (("device_ms",) if graph is not None else ()):
        out["clip_torch_over_clip_fused_" + key[:-3]] = f["clip_torch"][key] / f["clip_fused"][key]
        out["foreach_ema_over_fused_ema_" + key[:-3]] = f["foreach_ema"][key] / f["fused_ema"][key]
    return out


def bench_rcan(args):
    import sisr_amd as sisr
    B, S = 8, 128
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(B, 3, S, S, generator=g).cuda(), torch.rand(B, 3, 4 * S, 4 * S, generator=g).cuda()
    hs = {}
    for name, kw in (("plain", {}), ("ema", {"ema_decay": EMA_DECAY})):
        torch.manual_seed(8)
        hs[name] = sisr.handlers.RCANHandler(device=0, model_save_dir=tempfile.gettempdir(), eval_mode=False, lr=1e-4, scale=4, **kw)
    steps = {k: (lambda h=h: h.train_step(x, y)) for k, h in hs.items()}
    for fn in steps.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = alternate((steps["plain"], steps["ema"]), args.window, args.rounds)
    med = statistics.median
    return {"batch": B, "lr_size": S, "scale": 4, "ema_decay": EMA_DECAY, "plain_step_ms": med(a), "ema_step_ms": med(b),
            "plain_step_windows_ms": a, "ema_step_windows_ms": b, "ema_step_over_plain_step": med(b) / med(a),
            "added_ms": med(b) - med(a), "plain_tiles_per_s": 1e3 * B / med(a), "ema_tiles_per_s": 1e3 * B / med(b)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("update_bench needs a GPU: nothing here can be measured without one")
    doc = {"metric": "update_step", "device": torch.cuda.get_device_name(0), "qrcan_x4_update": bench_update(args)}
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
