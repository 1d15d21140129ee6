"""The output stage of evaluation on one GPU: metrics.eval_output (csrc/eval_output.hip) beside the host path it replaces and
beside the same arithmetic from stock torch ops, and what the device_outputs switch does to eval_sisr end to end.

python tools/eval_output_bench.py [--window 1.0] [--rounds 3] [--out profiles/eval_output_bench.json]

1. One output image of 2040 x 1356 x 3 and one of 512 x 512 x 3, already on the device with its HR image, for three cases --
   PSNR only, bytes only, both.  Every form ends with the same things on the host (the PSNR value, the uint8 HWC image):
     hip        metrics.eval_output on the device tensors: one sisr_eval_output call, n float64 values and / or the bytes copied back
     host       the present path: the fp32 output copied to the host, metrics.batch_rgb_to_ycbcr of it and of the HR image, metrics.psnr,
                (clip(rgb) * 255).round().astype(uint8) -- D2H copy included, host clock
     stock      stock torch ops on the same GPU: clamp, weighted sum, squared difference .double().mean(), mul / round / to(uint8) /
                permute, then the same copies back
   Host clock around work that ends with everything on the host; the forms alternate window by window (each at least `window`
   seconds), medians reported.  The sisr_eval_output call alone (buffers made beforehand, nothing copied back) is timed
   between two device events as well, with the bytes it needs (computed from the shape) over that time.
2. eval_sisr on the Set5 fixture with a full-depth RCAN x4 (seeded weights), PSNR + SSIM, save_im on: seconds per image with
   device_outputs off and on, alternating, after one warm-up run of each; the whole call, and the call less the time inside
   ModelInterface.__init__ (network construction and checkpoint load, which the switch does not touch).
Prints one JSON line and, with --out, writes it.  Fails without a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np  # noqa: E402
import torch  # noqa: E402

SIZES = ((1356, 2040), (512, 512))  # (h, w)
CASES = (("psnr", True, False), ("bytes", False, True), ("both", True, True))


def host_window(fn, seconds):
    """run fn() (which leaves nothing in flight) for at least `seconds` of wall time -> ms per call"""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return 1e3 * dt / n


def device_window(fn, seconds):
    """run fn() repeatedly for at least `seconds` of device time between two device events -> ms per call"""
    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= seconds * 1e3:
            return ms / n
        n = max(n + 1, int(n * min(10.0, 1.2 * seconds * 1e3 / max(ms, 1e-3))))


def alternate(fns, window, seconds, rounds):
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for t, fn in zip(ts, fns):
            t.append(window(fn, seconds))
    return ts


def bench_size(h, w, args):
    from sisr_amd import hip
    from sisr_amd import metrics as M
    g = torch.Generator().manual_seed(8)
    hr = torch.rand((1, 3, h, w), generator=g)
    out = (hr + 0.05 * torch.randn((1, 3, h, w), generator=g)).cuda()
    hr_dev, hr_host = hr.cuda(), hr
    weights = torch.tensor([0.299, 0.587, 0.114], device="cuda").view(1, 3, 1, 1)
    L = hip.lib()
    nbytes = L.sisr_eval_output_workspace_bytes(1, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    mse = torch.empty(1, dtype=torch.float64, device="cuda")
    rgb8 = torch.empty((1, h, w, 3), dtype=torch.uint8, device="cuda")
    res = {"shape": [1, 3, h, w], "cases": {}}
    med = statistics.median
    for name, want_psnr, want_rgb8 in CASES:
        def hip_call():
            values, b = M.eval_output(out, hr_dev, want_psnr=want_psnr, want_rgb8=want_rgb8)
            return values, (b.cpu().numpy() if b is not None else None)

        def host_call():
            rgb = out.cpu().numpy()
            values = b = None
            if want_psnr:
                ya, yb = M.batch_rgb_to_ycbcr(rgb), M.batch_rgb_to_ycbcr(hr_host.numpy())
                values = [M.psnr(ya[0, 0], yb[0, 0], 1)]
            if want_rgb8:
                b = (M.standard_image_formatting(rgb)[0].transpose(1, 2, 0) * 255).round().astype(np.uint8)
            return values, b

        def stock_call():
            values = b = None
            c = out.clamp(0, 1)
            if want_psnr:
                ya, yb = (c * weights).sum(1), (hr_dev.clamp(0, 1) * weights).sum(1)
                m = (ya - yb).double().square().mean(dim=(1, 2)).cpu().tolist()
                values = [100 if v == 0 else 20 * np.log10(1 / np.sqrt(v)) for v in m]
            if want_rgb8:
                b = c.mul(255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
            return values, b

        def kernel_call():
            hip.check(L.sisr_eval_output(out.data_ptr(), 3, None, hr_dev.data_ptr() if want_psnr else None, 0, 3, 1, h, w, 0,
                                         mse.data_ptr() if want_psnr else None, rgb8.data_ptr() if want_rgb8 else None,
                                         ws.data_ptr(), nbytes, hip.stream()), "sisr_eval_output")

        calls = {"hip": hip_call, "host": host_call, "stock": stock_call}
        for fn in list(calls.values()) + [kernel_call]:  # every form warmed up: code objects, allocator, pinned staging
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        a, b, c = hip_call(), host_call(), stock_call()
        case = {}
        if want_psnr:
            case["psnr_hip_host_stock"] = [float(a[0][0]), float(b[0][0]), float(c[0][0])]
        if want_rgb8:
            case["bytes_hip_equal_host"] = bool((a[1][0] == b[1]).all())
            case["bytes_stock_differing_from_host"] = int((c[1][0] != b[1]).sum())
        ts = dict(zip(calls, alternate(list(calls.values()), host_window, args.window, args.rounds)))
        for k, v in ts.items():
            case[k + "_ms"] = med(v)
            case[k + "_windows_ms"] = v
        kt = [device_window(kernel_call, args.window) for _ in range(args.rounds)]
        need = h * w * ((24 if want_psnr else 12) + (3 if want_rgb8 else 0))  # fp32 planes read, bytes written
        case.update(kernel_ms=med(kt), kernel_windows_ms=kt, kernel_bytes=need,
                    kernel_tb_per_s=need / (med(kt) * 1e-3) / 1e12,
                    host_over_hip=case["host_ms"] / case["hip_ms"], stock_over_hip=case["stock_ms"] / case["hip_ms"])
        res["cases"][name] = case
    return res


def bench_eval_sisr(args):
    """seconds per image of eval_sisr on the Set5 fixture, full-depth RCAN x4, device_outputs off and on"""
    from sisr_amd import cli
    from sisr_amd.handlers import ModelInterface
    set5 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "set5")
    with tempfile.TemporaryDirectory() as tmp:
        params = {"name": "rcan", "internal_params": {"scale": 4, "lr": 1e-4}}
        torch.manual_seed(8)
        m = ModelInterface(tmp, "rcan_full", gpu="single", sp_gpu=0, mode="train", new_params=params)
        cli._dump_toml({"model": params}, os.path.join(m.base_folder, "config.toml"))
        m.save()
        del m
        torch.cuda.empty_cache()

        load = [0.0]  # seconds inside ModelInterface.__init__ (network construction + checkpoint load), timed apart
        real_init = cli.ModelInterface.__init__

        def timed_init(self, *a, **k):
            t = time.perf_counter()
            real_init(self, *a, **k)
            torch.cuda.synchronize()
            load[0] += time.perf_counter() - t
        cli.ModelInterface.__init__ = timed_init

        def run(on, name):
            load[0] = 0.0
            t0 = time.perf_counter()
            df, _ = cli.eval_sisr(model_and_epoch=[["rcan_full", "0"]], model_loc=tmp, gpu=True, hr_dir=os.path.join(set5, "hr"),
                                  lr_dir=os.path.join(set5, "lr_random_blur"), full_directory=True, scale=4, out_loc=tmp,
                                  results_name=name, metrics=["PSNR", "SSIM"], save_im=True, device_outputs=on)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            return dt / len(df), df, (dt - load[0]) / len(df)

        try:
            df0, df1 = run(False, "warm_off")[1], run(True, "warm_on")[1]
            off, on, off_run, on_run = [], [], [], []
            for r in range(args.rounds):
                a, b = run(False, "off%d" % r), run(True, "on%d" % r)
                off.append(a[0])
                on.append(b[0])
                off_run.append(a[2])
                on_run.append(b[2])
        finally:
            cli.ModelInterface.__init__ = real_init
        med = statistics.median
        return {"images": len(df0), "model": "rcan x4, full depth, seeded weights", "metrics": ["PSNR", "SSIM"], "save_im": True,
                "whole_call": "model load, data loading, forward, metrics, PNG encoding",
                "off_s_per_image": med(off), "on_s_per_image": med(on), "off_runs": off, "on_runs": on,
                "off_over_on": med(off) / med(on),
                "without_model_load": "the same calls less the time inside ModelInterface.__init__",
                "off_s_per_image_without_load": med(off_run), "on_s_per_image_without_load": med(on_run),
                "off_runs_without_load": off_run, "on_runs_without_load": on_run,
                "off_over_on_without_load": med(off_run) / med(on_run),
                "max_abs_psnr_difference_db": float(np.abs(np.asarray(df0["PSNR"]) - np.asarray(df1["PSNR"])).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-eval-sisr", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_output_bench needs a GPU: nothing here can be measured without one")
    doc = {"metric": "eval_output", "device": torch.cuda.get_device_name(0), "host_cpus": os.cpu_count(), "sizes": []}
    for h, w in SIZES:
        doc["sizes"].append(bench_size(h, w, args))
    if not args.skip_eval_sisr:
        doc["eval_sisr_set5"] = bench_eval_sisr(args)
    line = json.dumps(doc)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
