"""RRDBNet on one GPU: the dense-block kernels alone, one RRDB, and the full x4 net, beside the same modules in stock torch.nn.

python tools/rrdb_bench.py [--window 0.5] [--rounds 3] [--blocks 23] [--out profiles/rrdb_bench.json]

  kernels   sisr_dense3x3_fwd / _dgrad (accumulating) / _wgrad in place in a 192-channel stack at 32 x 64^2 and 8 x 128^2 pixels
            for cin = 64 .. 160: median microseconds of `rounds` windows, the spread of the windows, algorithmic fp32 TFLOP/s
            (2 * 9 * cin * 32 per pixel) and its fraction of the 157.3 TFLOP/s matrix peak; the forward also beside
            F.conv2d(cin -> 32) on a channels-last map (which has no concatenation to build here either).
  rrdb      one RRDB (three dense blocks + skip), forward + backward at both shapes, against tests/_dense.RRDBTwin.
  net       RRDBHandler's train step (L1 + FlatAdam, hipGraph replay) and forward at 8 tiles of 128^2, against the twin with
            F.l1_loss and torch.optim.Adam; torch.cuda.max_memory_allocated of one eager train step of each.
The two sides alternate window by window (tools/basic_bench.py).  Writes one JSON document.  Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from basic_bench import FP32_MATRIX_PEAK_TFLOPS, alternate, window  # noqa: E402
import _dense as D  # noqa: E402

SHAPES = [(32, 64, 64), (8, 128, 128)]
CL = torch.channels_last
med = statistics.median


def _entry(ms_windows, flop):
    ms = med(ms_windows)
    tf = flop / (ms * 1e-3) / 1e12
    return {"us": ms * 1e3, "windows_us": [w * 1e3 for w in ms_windows], "tflops": tf, "fraction_of_peak": tf / FP32_MATRIX_PEAK_TFLOPS}


def kernels(args):
    from sisr_amd import hip, ops
    L, out = hip.lib(), []
    for B, H, W in SHAPES:
        g = torch.Generator().manual_seed(8)
        S = torch.randn((B, 192, H, W), generator=g).cuda().contiguous(memory_format=CL)
        dS = torch.randn((B, 192, H, W), generator=g).cuda().contiguous(memory_format=CL)
        for cin in D.CINS:
            w = (torch.randn((32, cin, 3, 3), generator=g) * 0.05).cuda()
            b = torch.zeros(32).cuda()
            pf, pd = ops.dense_pack(w)
            dw, db = torch.empty_like(w), torch.empty_like(b)
            nb = L.sisr_dense3x3_wgrad_workspace_bytes(B, H, W, cin)
            ws = hip.workspace(S.device, nb)
            sp, dsp, st = hip.ptr(S), hip.ptr(dS), hip.stream()
            xs = S[:, :cin].contiguous(memory_format=CL)

            def fwd():
                hip.check(L.sisr_dense3x3_fwd(sp, 192, cin, hip.ptr(pf), hip.ptr(b), 1, 0.2, sp + 4 * cin, 192, B, H, W, st), "fwd")

            def dgrad():
                hip.check(L.sisr_dense3x3_dgrad(dsp + 4 * cin, 192, sp + 4 * cin, 192, 0.2, hip.ptr(pd), dsp, 192, cin, 1, B, H, W,
                                                st), "dgrad")

            def wgrad():
                hip.check(L.sisr_dense3x3_wgrad(sp, 192, cin, dsp + 4 * cin, 192, sp + 4 * cin, 192, 0.2, hip.ptr(dw), hip.ptr(db),
                                                hip.ptr(ws), nb, B, H, W, st), "wgrad")

            def stock():
                F.leaky_relu(F.conv2d(xs, w, b, padding=1), 0.2)

            flop = 2.0 * 9 * cin * 32 * B * H * W
            rec = {"batch": B, "height": H, "width": W, "cin": cin}
            for name, fn in (("fwd", fwd), ("dgrad", dgrad), ("wgrad", wgrad), ("stock_conv2d_lrelu", stock)):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                rec[name] = _entry([window(fn, args.window * 0.4) for _ in range(args.rounds)], flop)
                dS.normal_(generator=None)  # (the accumulating input gradient grows dS; keep it finite)
            out.append(rec)
    return out


def _pair(hip_fn, stock_fn, args, what):
    for fn in (hip_fn, stock_fn):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    a, b = alternate(hip_fn, stock_fn, args.window, args.rounds)
    return {"hip_%s_ms" % what: med(a), "stock_%s_ms" % what: med(b), "hip_%s_windows_ms" % what: a,
            "stock_%s_windows_ms" % what: b, "%s_speedup_over_stock" % what: med(b) / med(a)}


def one_rrdb(args):
    import sisr_amd as sisr
    out = []
    for B, H, W in SHAPES:
        torch.manual_seed(8)
        blk = sisr.rrdb.RRDB().cuda()
        twin = D.RRDBTwin().cuda().to(memory_format=CL)
        twin.load_state_dict(blk.state_dict())
        g = torch.Generator().manual_seed(8)
        x = torch.randn((B, 64, H, W), generator=g).cuda().contiguous(memory_format=CL).requires_grad_(True)
        cot = torch.randn((B, 64, H, W), generator=g).cuda().contiguous(memory_format=CL)

        def run(m):
            def fn():
                x.grad = None
                for p in m.parameters():
                    p.grad = None
                m(x).backward(cot)
            return fn

        rec = {"batch": B, "height": H, "width": W}
        rec.update(_pair(run(blk), run(twin), args, "forward_backward"))
        out.append(rec)
    return out


def full_net(args):
    import sisr_amd as sisr
    B, S = 8, 128
    torch.manual_seed(8)
    h = sisr.available_models["rrdb"](device=0, model_save_dir="/tmp", eval_mode=False, lr=1e-4, num_blocks=args.blocks)
    twin = D.RRDBNetTwin(num_blocks=args.blocks).cuda().to(memory_format=CL)
    twin.load_state_dict(h.net.state_dict())
    opt = torch.optim.Adam(twin.parameters(), lr=1e-4)
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(B, 3, S, S, generator=g).cuda(), torch.rand(B, 3, 4 * S, 4 * S, generator=g).cuda()

    def hip_step():
        h.train_step(x, y)

    def stock_step():
        opt.zero_grad(set_to_none=True)
        F.l1_loss(twin(x), y).backward()
        opt.step()

    def hip_fwd():
        h.run_eval(x, keep_on_device=True)

    def stock_fwd():
        with torch.no_grad():
            twin(x)

    rec = {"batch": B, "lr_size": S, "num_blocks": args.blocks, "parameters": sum(p.numel() for p in h.net.parameters())}
    peak = {}
    h.use_graph = False  # memory of ONE EAGER step on both sides: a captured graph keeps its maps in a private pool that
    for name, fn in (("hip", hip_step), ("stock", stock_step)):  # max_memory_allocated does not see after the capture
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        rec["%s_step_memory_allocated_before_bytes" % name] = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated()
        rec["%s_eager_step_max_memory_allocated_bytes" % name] = peak[name]
    rec["step_memory_stock_over_hip"] = peak["stock"] / peak["hip"]
    h.use_graph = True
    rec.update(_pair(hip_step, stock_step, args, "step"))
    twin.eval()
    rec.update(_pair(hip_fwd, stock_fwd, args, "forward"))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=23)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rrdb_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rrdb_bench needs a GPU"
    doc = {"device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK_TFLOPS,
           "window_seconds": args.window, "rounds": args.rounds}
    doc["kernels"] = kernels(args)
    doc["rrdb"] = one_rrdb(args)
    doc["net"] = full_net(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    for r in doc["kernels"]:
        print("%2d x %3d^2 cin %3d  " % (r["batch"], r["height"], r["cin"]) + "  ".join(
            "%s %7.1f us %5.1f TF" % (k, r[k]["us"], r[k]["tflops"]) for k in ("fwd", "dgrad", "wgrad", "stock_conv2d_lrelu")))
    for r in doc["rrdb"]:
        print("RRDB %d x %d^2 fwd+bwd: hip %.2f ms, stock %.2f ms" % (r["batch"], r["height"], r["hip_forward_backward_ms"],
                                                                      r["stock_forward_backward_ms"]))
    n = doc["net"]
    print("net step: hip %.1f ms, stock %.1f ms; forward: hip %.1f ms, stock %.1f ms; step memory hip %.2f GB, stock %.2f GB"
          % (n["hip_step_ms"], n["stock_step_ms"], n["hip_forward_ms"], n["stock_forward_ms"],
             n["hip_eager_step_max_memory_allocated_bytes"] / 2 ** 30, n["stock_eager_step_max_memory_allocated_bytes"] / 2 ** 30))


if __name__ == "__main__":
    main()
