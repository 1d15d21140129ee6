"""IKC's Corrector on one GPU: the HIP path beside the same net in stock torch.nn (a real torch.cat), in one call.

python tools/corrector_bench.py [--window 1.0] [--rounds 3] [--out profiles/corrector_bench.json]

Default corrector (five 5 x 5 convs of 64 with strides 1, 1, 2, 1, 2, code MLP, three pointwise head layers of 128, global
mean) with M = 12 code entries, on SR-sized images: 32 x 3 x 256^2 (forward, and train step = forward + MSE + backward + the
same torch Adam on both sides) and 1 x 3 x 1356 x 2040 (forward only), the x 4 outputs of 32 x 64^2 and 1 x 339 x 510 LR.
The two versions alternate window by window (tools/basic_bench.py) and the median window is reported.  Also, per shape, one
more HIP pass with every library call between two device events: each call's time in call order, and for the K x K convs and
the stride-2 input gradient the executed fp32 TFLOP/s (padded widths; the outputs' own products only) against the 157.3
TFLOP/s matrix peak.  `parity`: distances of the HIP net and of the stock fp32 net on the same GPU from the float64 twin
(tests/_corrector.py; each with the LeakyReLU branches of its own forward inside the kink band).  `whole_loop_339x510`: IKC's
loop (7 x SFTMD + 7 x corrector) on one 339 x 510 LR image through CorrectorHandler.correct.  `learning`: the recorded
learning run on the Set5 fixtures (see learning()).  `--pointwise-ab LIB`: the 128-output pointwise layers under two builds of
the library.  Writes one JSON document.  Fails without a GPU."""
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

from basic_bench import FP32_MATRIX_PEAK_TFLOPS, alternate  # noqa: E402
import _corrector as T  # noqa: E402
import _predictor as P  # noqa: E402

SHAPES = [(32, 256, 256, True), (1, 1356, 2040, False)]
M = 12
CONV_CALLS = ("sisr_convk_mfma_leaky", "sisr_convk_s2_mfma_leaky")


def nets():
    import sisr_amd as sisr
    torch.manual_seed(8)
    net = sisr.corrector.DegradationCorrector(num_codes=M).cuda()
    stock = T.Twin(num_codes=M)
    stock.load_state_dict(net.state_dict())
    return net, stock.cuda()


def bench_shape(net, stock, B, H, W, train, args):
    import sisr_amd as sisr
    g = torch.Generator().manual_seed(8)
    x, c, y = torch.rand(B, 3, H, W, generator=g).cuda(), torch.rand(B, M, generator=g).cuda(), torch.rand(B, M, generator=g).cuda()
    opts = [torch.optim.Adam(n.parameters(), lr=1e-4) for n in (net, stock)]

    def hip_step():
        opts[0].zero_grad(set_to_none=True)
        sisr.ops.mse_loss(net(x, c), y).backward()
        opts[0].step()

    def stock_step():
        opts[1].zero_grad(set_to_none=True)
        F.mse_loss(stock(x, c), y).backward()
        opts[1].step()

    def hip_fwd():
        with torch.no_grad():
            net(x, c)

    def stock_fwd():
        with torch.no_grad():
            stock(x, c)

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
    out["calls"] = calls(net, hip_step if train else hip_fwd, B, H, W)
    return out


def calls(net, fn, B, H, W):
    """one more pass with every library call between two device events, in call order"""
    from sisr_amd import hip, ops
    events, real = [], hip.lib
    inner = real()

    class Wrap:
        def __getattr__(self, name):
            f = getattr(inner, name)
            if name.endswith("_bytes") or name.endswith("_size"):
                return f

            def call(*a):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = f(*a)
                e1.record()
                events.append((name, ops.IN_BACKWARD, e0, e1))
                return rc
            return call

    wrapped = Wrap()
    hip.lib = lambda: wrapped
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        hip.lib = real
    pad = lambda ch: 32 if ch <= 32 else 64  # noqa: E731
    flop, h, w = [], H, W  # executed flop of each K x K layer: its outputs' own products at the padded widths
    for m, s in zip(net.layer_dict.values(), net.strides):
        if s == 2:
            h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        flop.append(2.0 * B * h * w * m.kernel_size[0] ** 2 * pad(m.in_channels) * pad(m.out_channels))
    rows, layer = [], 0
    dgrads = [i for i in range(len(flop) - 1, 0, -1)]  # the backward runs the last layer first; the first has no dx
    for name, bwd, e0, e1 in events:
        row = {"call": name, "backward": bool(bwd), "ms": e0.elapsed_time(e1)}
        index = None
        if name in CONV_CALLS and not bwd:
            index, layer = layer, layer + 1
        elif bwd and (name == "sisr_dgradk_s2_mfma_leaky" or name == "sisr_convk_mfma_leaky") and dgrads:
            index = dgrads.pop(0)
        if index is not None:
            tflops = flop[index] / (row["ms"] * 1e-3) / 1e12
            row.update({"layer": index, "stride": net.strides[index], "executed_gflop": flop[index] / 1e9, "tflops": tflops,
                        "share_of_fp32_matrix_peak": tflops / FP32_MATRIX_PEAK_TFLOPS})
        rows.append(row)
    return rows


def parity():
    """HIP net and stock fp32 net (same GPU) against the float64 twin on the host, at the test's largest shape"""
    import sisr_amd as sisr
    rows = []
    for m_out, nf in ((1, 64), (12, 64), (12, 48)):
        cfg = dict(num_codes=m_out, num_features=nf)
        net = sisr.corrector.DegradationCorrector(**cfg)
        sd = T.kaiming_state(net, 260 + m_out + nf)
        net.load_state_dict(sd)
        net.cuda()
        stock = T.twin(sd, torch.float32, **cfg).cuda()
        g = torch.Generator().manual_seed(261)
        x, codes = torch.rand((2, 3, 37, 70), generator=g), torch.rand((2, m_out), generator=g)
        cot = torch.randn((2, m_out), generator=g)
        out = net(x.cuda(), codes.cuda())
        out.backward(cot.cuda())
        sout = stock(x.cuda(), codes.cuda())
        sout.backward(cot.cuda())
        hb, _ = T.hip_branches(sisr.ops, net, x.cuda(), codes.cuda())
        sb = [b.cpu() for b in T.fp32_branches(stock, x.cuda(), codes.cuda())]
        row = {"num_codes": m_out, "num_features": nf}
        for name, model, result, branches in (("hip", net, out, hb), ("stock_fp32", stock, sout, sb)):
            ref = T.twin(sd, **cfg)
            want, decided = ref(x.double(), codes.double(), branches=branches)
            want.backward(cot.double())
            row[name] = {"output": P.rel_l2(result, want), "elements_at_the_kink": decided,
                         "worst_gradient": max(P.rel_l2(p.grad, q.grad) for p, q in zip(model.parameters(), ref.parameters()))}
        rows.append(row)
    return rows


def timed(fn, reps=7):
    """median device time (ms) of fn over `reps` calls after two warm-up calls, each between two device events"""
    out = []
    for k in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if k >= 2:
            out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def pointwise_times():
    """the head's 128-output layers alone (forward under no_grad): 64 -> 128 with a per-image bias and 128 -> 128, at the pixel
    counts of the two shapes after the two stride-2 layers.  Run once per library build (SISR_HIP_LIB) by --pointwise-ab."""
    import sisr_amd as sisr
    g = torch.Generator().manual_seed(8)
    rows = []
    for B, H, W in ((32, 64, 64), (1, 339, 510)):
        for cin in (64, 128):
            x = torch.rand(B, cin, H, W, generator=g).contiguous(memory_format=torch.channels_last).cuda()
            w, b = (torch.randn(128, cin, 1, 1, generator=g) * 0.05).cuda(), torch.rand(128, generator=g).cuda()
            ib = torch.rand(B, 128, generator=g).cuda() if cin == 64 else None
            with torch.no_grad():
                ms = timed(lambda: sisr.ops.conv_1x1(x, w, b, slope=0.2, image_bias=ib), reps=21)
            rows.append({"batch": B, "height": H, "width": W, "cin": cin, "cout": 128, "forward_ms": ms})
    return rows


def pointwise_ab(other_lib, rounds=2):
    """the product library (128 outputs as two 64-channel halves) and `other_lib` (a build whose host dispatch launches
    bk_pw_kernel<4>, all four N-tiles in one wave) in fresh child processes, alternating"""
    import subprocess
    runs = {"halves": [], "one_wave": []}
    for _ in range(rounds):
        for name, lib in (("halves", None), ("one_wave", other_lib)):
            env = dict(os.environ)
            env.pop("SISR_HIP_LIB", None)
            if lib:
                env["SISR_HIP_LIB"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--pointwise-only"], env=env, capture_output=True,
                               text=True, timeout=300, check=True)
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    return runs


def experiments(root, blocks=16):
    """SFTMD (KEYS as its metadata), the default predictor and the default corrector around them as new experiments under
    `root` -> the three ModelInterfaces, in train mode"""
    import sisr_amd as sisr
    torch.manual_seed(8)
    keys = list(P.KEYS)
    sft = P.save_experiment(sisr, root, "sftmd", {"name": "sftmd", "internal_params": {
        "scale": 4, "lr": 1e-4, "metadata": keys, "num_blocks": blocks, "num_features": 64, "in_nc": 3}}, gpu=True)
    pred = P.save_experiment(sisr, root, "pred", {"name": "predictor", "internal_params": {
        "scale": 4, "lr": 1e-4, "metadata": keys}}, gpu=True)
    return sft, pred


def corrector_experiment(root, iterations=7):
    import sisr_amd as sisr
    torch.manual_seed(9)
    return sisr.ModelInterface(str(root), "corr", gpu="single", sp_gpu=0, mode="train", new_params={
        "name": "corrector", "internal_params": {"scale": 4, "lr": 1e-4, "metadata": list(P.KEYS), "sr_model": ["sftmd", 0],
                                                 "predictor": ["pred", 0], "iterations": iterations}})


def whole_loop(root):
    """IKC's loop on one 339 x 510 LR image at x 4: predictor, 7 x (SFTMD of 16 blocks + corrector), the final SFTMD pass;
    untrained weights (the time does not depend on them)"""
    experiments(root)
    h = corrector_experiment(root).model
    x = torch.rand(1, 3, 339, 510, generator=torch.Generator().manual_seed(8)).cuda()
    code = h.initial_codes(x)
    with torch.no_grad():
        h.net.eval()
        sr = h.super_resolve(x, code)
        out = {"lr_height": 339, "lr_width": 510, "iterations": 7,
               "predictor_ms": timed(lambda: h.initial_codes(x)),
               "sftmd_pass_ms": timed(lambda: h.super_resolve(x, code)),
               "corrector_pass_ms": timed(lambda: h.run_model(sr, extra_channels=code)),
               "loop_without_final_sr_ms": timed(lambda: h.correct(x, code, want_sr=False), reps=5),
               "loop_with_final_sr_ms": timed(lambda: h.correct(x, code), reps=5)}
    out["sftmd_share_of_loop"] = 7 * out["sftmd_pass_ms"] / out["loop_without_final_sr_ms"]
    return out


def learning(root, steps, every=50):
    """The recorded learning run (a measurement, not a test): on 32 x 32 LR tiles of the five Set5 HR images under
    tests/golden/set5 with blur + noise + JPEG drawn online, `steps` steps each of a reduced SFTMD (4 blocks, true codes) and
    of the default predictor, then `steps` batches (7 optimiser steps each) of the default corrector around the two, frozen.
    code_MAE of iterations 0 .. 7 on 20 fixed degraded Set5 images every `every` batches, beside the mean code of the tiles."""
    import random

    import numpy as np
    import sisr_amd as sisr
    hr = os.path.join(ROOT, "tests", "golden", "set5", "hr")
    np.random.seed(8)
    torch.manual_seed(8)
    random.seed(8)
    dev = torch.device("cuda:0")
    ds = lambda **kw: sisr.data.SuperResImages(hr_dir=hr, online_degradations=True, split="all", scale=4,  # noqa: E731
                                                online_degradation_params=dict(P.DEGRADATIONS), **kw)
    loader = sisr.data.DeviceTileLoader([ds(random_crop=32, random_augments=True)], 5, dev, degrade_tiles=True)
    val_set = ds()
    val = [val_set[i % 5] for i in range(20)]  # 20 fixed draws: each Set5 image under four degradations
    keys = [tuple([k]) for k in val_set.metadata_keys]
    sft, pred = experiments(root, blocks=4)
    seen = []

    def batches(n):
        done = 0
        while done < n:
            for batch in loader:
                if done >= n:
                    return
                yield batch
                done += 1

    for batch in batches(steps):
        seen.append(pred.model.target_codes(batch["lr"], batch["metadata"], batch["metadata_keys"]).cpu())
        sft.model.run_train(batch["lr"], batch["hr"], metadata=batch["metadata"], metadata_keys=batch["metadata_keys"],
                            keep_on_device=True)
        pred.model.train_step(batch["lr"], None, metadata=batch["metadata"], metadata_keys=batch["metadata_keys"])
    sft.save(override=True)
    pred.save(override=True)
    h = corrector_experiment(root).model
    vt = torch.stack([h.target_codes(v["lr"][None], torch.from_numpy(np.asarray(v["metadata"]))[None], keys)[0].cpu() for v in val])
    mean_code = torch.cat(seen).mean(dim=0)
    curve = []

    def validate(step):
        per_iteration = [[] for _ in range(8)]
        for v in val:
            history = h.correct(v["lr"][None], want_sr=False)[2]
            for i, c in enumerate(history):
                per_iteration[i].append(c.cpu())
        mae = [float((torch.cat(c).double() - vt.double()).abs().mean()) for c in per_iteration]
        curve.append({"corrector_batches": step, "code_MAE_by_iteration": mae})

    validate(0)
    for step, batch in enumerate(batches(steps), 1):
        h.run_train(batch["lr"], None, metadata=batch["metadata"], metadata_keys=batch["metadata_keys"], keep_on_device=True)
        if step % every == 0:
            validate(step)
    return {"steps_of_sftmd_and_predictor": steps, "corrector_batches": steps, "iterations": 7, "tiles_per_step": 5, "lr_tile": 32,
            "learning_rate": 1e-4, "sftmd_blocks": 4, "degradations": P.DEGRADATIONS, "validation_images": len(val),
            "code_MAE_mean_code": float((mean_code.double()[None] - vt.double()).abs().mean()),
            "code_MAE_predictor_alone": curve[0]["code_MAE_by_iteration"][0], "curve": curve}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corrector_bench.json"))
    ap.add_argument("--learn", type=int, default=200, help="steps of the recorded learning run (0: skip it)")
    ap.add_argument("--pointwise-ab", metavar="LIB", help="also time the 128-output pointwise layers under this other build "
                                                          "of the library (the one-wave form), alternating with the product's")
    ap.add_argument("--pointwise-only", action="store_true", help="print the pointwise times of the loaded library and stop")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("corrector_bench needs a GPU: nothing here can be measured without one")
    if args.pointwise_only:
        print(json.dumps(pointwise_times()))
        return
    net, stock = nets()
    doc = {"metric": "corrector_bench", "device": torch.cuda.get_device_name(0), "num_codes": M,
           "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK_TFLOPS, "shapes": []}
    for B, H, W, train in SHAPES:
        doc["shapes"].append(bench_shape(net, stock, B, H, W, train, args))
    doc["parity_2x3x37x70"] = parity()
    import tempfile
    with tempfile.TemporaryDirectory() as root:
        doc["whole_loop_339x510"] = whole_loop(root)
    if args.learn:
        with tempfile.TemporaryDirectory() as root:
            doc["learning"] = learning(root, args.learn)
    if args.pointwise_ab:
        doc["pointwise_128_outputs_halves_against_one_wave"] = pointwise_ab(args.pointwise_ab)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
