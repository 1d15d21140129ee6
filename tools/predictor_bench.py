"""The degradation predictor on one GPU: the HIP path beside the same net in stock torch.nn, in one call.

python tools/predictor_bench.py [--window 1.0] [--rounds 3] [--learn 400] [--out profiles/predictor_bench.json]

Default predictor (6 layers of 5 x 5, 64 wide, LeakyReLU 0.2, global mean) with M = 12 outputs, at 32 x 3 x 64^2 and
8 x 3 x 128^2 (forward, and train step = forward + MSE + backward + Adam) and 1 x 3 x 339 x 510 (forward only).  The two
versions alternate window by window (tools/basic_bench.py: each window at least `window` seconds of device time between two
device events, after a warm-up of every shape) and the median window is reported.  Also, per shape, one more HIP step with
every library call between two device events: the time of each layer's forward, input-gradient and weight-gradient launch, the
first layer's share of the forward, the mean kernels, and the executed fp32 TFLOP/s of the forward convs (padded widths: what
the matrix cores run) against the 157.3 TFLOP/s matrix peak.  `parity`: distances of the HIP net and of the stock fp32 net on
the same GPU from the float64 twin (tests/_predictor.py; each with the LeakyReLU branches of its own forward inside the kink
band).  `learning`: `--learn` steps on 32 x 32 LR tiles of the Set5 HR images under tests/golden/set5 with blur + noise + JPEG
drawn online, val-MAE every 25 steps on 20 fixed degraded Set5 images beside the trivial predictor that answers the mean
code of the tiles trained on so far.  Writes one JSON document.  Fails without a GPU.
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/predictor_bench.py --steps-only 20`."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from basic_bench import FP32_MATRIX_PEAK_TFLOPS, alternate, window  # noqa: E402
import _predictor as P  # noqa: E402

SHAPES = [(32, 64, 64, True), (8, 128, 128, True), (1, 339, 510, False)]
M = 12


def handler(lr=1e-4):
    import sisr_amd as sisr
    torch.manual_seed(8)
    return sisr.available_models["predictor"](device=0, model_save_dir="/tmp", eval_mode=False, lr=lr, metadata=list(P.KEYS))


def bench_shape(h, stock, opt, B, H, W, train, args):
    g = torch.Generator().manual_seed(8)
    x, y = torch.rand(B, 3, H, W, generator=g).cuda(), torch.rand(B, M, generator=g).cuda()

    def hip_step():
        h.train_step(x, y)

    def stock_step():
        opt.zero_grad(set_to_none=True)
        F.mse_loss(stock(x), y).backward()
        opt.step()

    def hip_fwd():
        with torch.no_grad():
            h.net(x)

    def stock_fwd():
        with torch.no_grad():
            stock(x)

    fns = (hip_step, stock_step, hip_fwd, stock_fwd) if train else (hip_fwd, stock_fwd)
    for fn in fns:  # every shape warmed up: code objects, library algorithm search
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    med = statistics.median
    hf, sf = alternate(hip_fwd, stock_fwd, args.window, args.rounds)
    out = {"batch": B, "height": H, "width": W, "hip_forward_ms": med(hf), "stock_forward_ms": med(sf),
           "hip_forward_windows_ms": hf, "stock_forward_windows_ms": sf, "forward_speedup_over_stock": med(sf) / med(hf)}
    if train:
        hs, ss = alternate(hip_step, stock_step, args.window, args.rounds)
        out.update({"hip_step_ms": med(hs), "stock_step_ms": med(ss), "hip_step_windows_ms": hs, "stock_step_windows_ms": ss,
                    "step_speedup_over_stock": med(ss) / med(hs)})
    out.update(calls(h, x, y, train))
    return out


def calls(h, x, y, train):
    """one more eager step (or forward) with every library call between two device events, in call order"""
    from sisr_amd import hip, ops
    events, real = [], hip.lib
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
                events.append((name, ops.IN_BACKWARD, e0, e1))
                return rc
            return call

    wrapped = Wrap()
    hip.lib = lambda: wrapped
    try:
        if train:
            h.train_step(x, y)
        else:
            with torch.no_grad():
                h.net(x)
        torch.cuda.synchronize()
    finally:
        hip.lib = real
    timed = [(n, bwd, a.elapsed_time(b)) for n, bwd, a, b in events]
    B, _, H, W = x.shape
    convs = [m for m in h.net.layer_dict.values()]
    pad = lambda c: 32 if c <= 32 else 64  # noqa: E731
    flop = [2.0 * B * H * W * m.kernel_size[0] ** 2 * pad(m.in_channels) * pad(m.out_channels) for m in convs]
    fwd = [ms for n, bwd, ms in timed if n == "sisr_convk_mfma_leaky" and not bwd]
    dgrad = [ms for n, bwd, ms in timed if n == "sisr_convk_mfma_leaky" and bwd][::-1]   # backward runs last layer first
    wgrad = [ms for n, bwd, ms in timed if n == "sisr_wgradk_mfma_leaky"][::-1]
    layers = []
    for i, m in enumerate(convs):
        row = {"layer": i, "cin": m.in_channels, "cout": m.out_channels, "forward_ms": fwd[i], "executed_gflop": flop[i] / 1e9,
               "forward_tflops": flop[i] / (fwd[i] * 1e-3) / 1e12,
               "forward_share_of_fp32_matrix_peak": flop[i] / (fwd[i] * 1e-3) / 1e12 / FP32_MATRIX_PEAK_TFLOPS}
        if train:
            row["weight_gradient_ms"] = wgrad[i]
            if i > 0:
                row["input_gradient_ms"] = dgrad[i - 1]  # (the first layer has none)
        layers.append(row)
    others = {}
    for n, bwd, ms in timed:
        if "convk_mfma_leaky" not in n and "wgradk_mfma_leaky" not in n:
            others[n] = others.get(n, 0.0) + ms
    names = [n for n, _, _ in timed]
    end = names.index("sisr_mse_loss") if "sisr_mse_loss" in names else len(names)  # the forward: layout, packs, convs, mean
    fwd_total = sum(ms for _, _, ms in timed[:end])
    inner_ms = statistics.median(fwd[1:-1]) if len(fwd) > 2 else None
    return {"layers": layers, "other_calls_ms": others, "forward_calls_total_ms": fwd_total,
            "first_layer_share_of_forward": fwd[0] / fwd_total, "first_layer_over_inner_layer": fwd[0] / inner_ms,
            "map_mean_ms": others.get("sisr_map_mean"), "map_mean_bwd_ms": others.get("sisr_map_mean_bwd"),
            "forward_convs_tflops": sum(flop) / (sum(fwd) * 1e-3) / 1e12,
            "forward_convs_share_of_fp32_matrix_peak": sum(flop) / (sum(fwd) * 1e-3) / 1e12 / FP32_MATRIX_PEAK_TFLOPS}


def parity():
    """HIP net and stock fp32 net (same GPU) against the float64 twin on the host, at the test's largest shape"""
    import sisr_amd as sisr
    ops = sisr.ops
    rows = []
    for m_out in (1, 12, 33):
        cfg = dict(num_outputs=m_out, num_features=64, num_layers=6)
        net = sisr.predictor.DegradationPredictor(**cfg)
        sd = P.kaiming_state(net, 70 + m_out + 64 + 6)
        net.load_state_dict(sd)
        net.cuda()
        stock = P.Twin(**cfg)
        stock.load_state_dict(sd)
        stock.cuda()
        g = torch.Generator().manual_seed(71)
        x, cot = torch.rand((2, 3, 37, 70), generator=g), torch.randn((2, m_out), generator=g)
        out = net(x.cuda())
        out.backward(cot.cuda())
        sout = stock(x.cuda())
        sout.backward(cot.cuda())
        with torch.no_grad():
            t, hb, sb = ops.nchw_to_nhwc_pad(x.cuda(), cp=32), [], []
            u = x.cuda()
            for i in range(6):
                c = net.layer_dict["conv_%d" % i]
                t = ops.conv_kxk(t, c.weight, c.bias, slope=net.slope)
                hb.append(t[:, :c.out_channels].cpu() > 0)
                u = F.leaky_relu(stock.layer_dict["conv_%d" % i](u), 0.2)
                sb.append(u.cpu() > 0)
        row = {"num_outputs": m_out}
        for name, model, result, branches in (("hip", net, out, hb), ("stock_fp32", stock, sout, sb)):
            ref = P.twin64(sd, **cfg)
            want, decided = P.twin_forward(ref, x, branches)
            want.backward(cot.double())
            row[name] = {"output": P.rel_l2(result, want), "elements_at_the_kink": decided,
                         "worst_gradient": max(P.rel_l2(p.grad, q.grad) for p, q in zip(model.parameters(), ref.parameters()))}
        rows.append(row)
    return rows


def learning(steps, every=25):
    import sisr_amd as sisr
    hr = os.path.join(ROOT, "tests", "golden", "set5", "hr")
    np.random.seed(8)
    torch.manual_seed(8)
    import random
    random.seed(8)
    dev = torch.device("cuda:0")
    ds = lambda **kw: sisr.data.SuperResImages(hr_dir=hr, online_degradations=True, split="all", scale=4,  # noqa: E731
                                                online_degradation_params=dict(P.DEGRADATIONS), **kw)
    loader = sisr.data.DeviceTileLoader([ds(random_crop=32, random_augments=True)], 5, dev, degrade_tiles=True)
    val_set = ds()
    val = [val_set[i % 5] for i in range(20)]  # 20 fixed draws: each Set5 image under four degradations
    keys = [tuple([k]) for k in val_set.metadata_keys]
    h = handler()
    vx = [v["lr"][None].to(dev) for v in val]
    vt = torch.stack([h.target_codes(v["lr"][None], torch.from_numpy(np.asarray(v["metadata"]))[None], keys)[0].cpu() for v in val])
    seen, curve, step = [], [], 0

    def validate():
        pred = torch.cat([h.run_eval(x)[0] for x in vx])
        mean_code = torch.cat(seen).mean(dim=0) if seen else torch.zeros(M)
        curve.append({"step": step, "val_MAE": float((pred.double() - vt.double()).abs().mean()),
                      "val_MAE_mean_code": float((mean_code.double()[None] - vt.double()).abs().mean())})

    while step < steps:
        for batch in loader:
            if step % every == 0:
                validate()
            if step >= steps:
                break
            seen.append(h.target_codes(batch["lr"], batch["metadata"], batch["metadata_keys"]).cpu())
            h.train_step(batch["lr"], None, metadata=batch["metadata"], metadata_keys=batch["metadata_keys"])
            step += 1
    validate()
    return {"steps": steps, "tiles_per_step": 5, "lr_tile": 32, "learning_rate": 1e-4, "degradations": P.DEGRADATIONS,
            "validation_images": len(val), "curve": curve}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--learn", type=int, default=400, help="steps of the recorded learning run (0: skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_bench.json"))
    ap.add_argument("--steps-only", type=int, default=0, metavar="N",
                    help="run N HIP train steps at 32 x 3 x 64 x 64 and nothing else: the target of `rocprofv3 --kernel-trace --stats`")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("predictor_bench needs a GPU: nothing here can be measured without one")
    h = handler()
    if args.steps_only:
        g = torch.Generator().manual_seed(8)
        x, y = torch.rand(32, 3, 64, 64, generator=g).cuda(), torch.rand(32, M, generator=g).cuda()
        for _ in range(args.steps_only):
            h.train_step(x, y)
        torch.cuda.synchronize()
        print(json.dumps({"metric": "predictor_steps_only", "steps": args.steps_only}))
        return
    torch.manual_seed(8)
    stock = P.Twin(num_outputs=M).cuda()
    opt = torch.optim.Adam(stock.parameters(), lr=1e-4)
    doc = {"metric": "predictor_bench", "device": torch.cuda.get_device_name(0), "num_outputs": M,
           "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK_TFLOPS, "shapes": []}
    for B, H, W, train in SHAPES:
        doc["shapes"].append(bench_shape(h, stock, opt, B, H, W, train, args))
    doc["parity_2x3x37x70_six_layers_64_wide"] = parity()
    if args.learn:
        doc["learning"] = learning(args.learn)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
