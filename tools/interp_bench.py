"""Time the evaluator's bicubic pre-up-sampling: the device kernel (sisr_pil_upsample, RGB + YCbCr in one launch) against the
host path it replaces (the reference's own calls: ToPILImage -> PIL resize BICUBIC -> ToTensor, then the numpy BT.601
conversion), on one DIV2K validation image at x4: 510 x 339 -> 2040 x 1356.

Device: HIP events around each call after a warm-up, >= 100 repeats; median and spread (min, p10, p90, max).  The kernel
writes scale^2 times what it reads, so the rate given is the output bytes over the median time, against the 8 TB/s HBM roof
(MI355X_MICROARCH.md; 6.29 TB/s is what a float4 copy reaches).  Cases: both outputs, each alone, and a batch of eight images
whose output no cache holds.  Host: wall clock around cli._low_res_prep + metrics.batch_rgb_to_ycbcr on the same machine, a few
repeats.  Every device output is compared with the host's.

    python tools/interp_bench.py [--reps 200] [--out profiles/interp_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ROOF_TBS, HBM_COPY_TBS = 8.0, 6.29  # MI355X_MICROARCH.md: spec peak / measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_bench.json"))
    a = ap.parse_args()
    import torch
    import sisr_amd
    D, M, hip = sisr_amd.degrade, sisr_amd.metrics, sisr_amd.hip
    if not torch.cuda.is_available():
        raise SystemExit("interp_bench needs a HIP device")
    L = hip.lib()
    scale, h, w = 4, 339, 510
    H, W = h * scale, w * scale
    results = []
    # one image, as eval_sisr's default batch size gives it; and eight, whose 531 MB of output no cache holds
    for name, n, want_rgb, want_ycc in (("rgb+ycbcr", 1, True, True), ("rgb", 1, True, False), ("ycbcr", 1, False, True),
                                        ("8 x rgb+ycbcr", 8, True, True)):
        lr = torch.rand((n, 3, h, w), generator=torch.Generator().manual_seed(0))
        dev = lr.cuda()
        bh, ch, ks = D._device_table(w, W, dev.device)
        bv, cv, _ = D._device_table(h, H, dev.device)
        rgb = torch.empty((n, 3, H, W), device="cuda") if want_rgb else None
        ycc = torch.empty((n, 3, H, W), device="cuda") if want_ycc else None
        stream = hip.stream()

        def call():
            hip.check(L.sisr_pil_upsample(dev.data_ptr(), hip.ptr(rgb), hip.ptr(ycc), bh.data_ptr(), ch.data_ptr(), bv.data_ptr(),
                                          cv.data_ptr(), ks, n, 3, h, w, H, W, stream), "sisr_pil_upsample")
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
        for e0, e1 in ev:
            e0.record()
            call()
            e1.record()
        torch.cuda.synchronize()
        us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev])
        # the host path: the reference's Pillow calls (+ its numpy colour conversion where YCbCr is asked for)
        host_s = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            host_rgb = sisr_amd.cli._low_res_prep(lr, scale)
            host_ycc = M.batch_rgb_to_ycbcr(host_rgb.numpy()) if want_ycc else None
            host_s.append(time.perf_counter() - t0)
        same = True
        if want_rgb:
            same = same and bool(np.array_equal(rgb.cpu().numpy(), host_rgb.numpy()))
        if want_ycc:
            same = same and bool(np.array_equal(ycc.cpu().numpy(), host_ycc))
        med = float(np.median(us))
        out_bytes = (int(want_rgb) + int(want_ycc)) * n * 3 * H * W * 4
        r = dict(case=name, images=n, h=h, w=w, scale=scale, reps=a.reps, warmup=a.warmup,
                 device_us=dict(median=med, min=float(us.min()), p10=float(np.percentile(us, 10)),
                                p90=float(np.percentile(us, 90)), max=float(us.max())),
                 output_bytes=out_bytes, input_bytes=n * 3 * h * w * 4, write_tbs=out_bytes / (med * 1e-6) / 1e12,
                 share_of_hbm_roof=out_bytes / (med * 1e-6) / 1e12 / HBM_ROOF_TBS,
                 host_s=dict(median=float(np.median(host_s)), min=float(min(host_s)), reps=a.host_reps),
                 host_over_device=float(np.median(host_s)) / (med * 1e-6), bit_identical_to_host=same)
        results.append(r)
        print(f"{name:>14}: device median {med:7.1f} us (p10 {r['device_us']['p10']:.1f}, p90 {r['device_us']['p90']:.1f})  "
              f"{r['write_tbs']:.2f} TB/s written = {100 * r['share_of_hbm_roof']:.0f} % of {HBM_ROOF_TBS} TB/s  "
              f"host {r['host_s']['median'] * 1e3:7.1f} ms  host/device {r['host_over_device']:.0f}x  identical {same}", flush=True)
    doc = dict(tool="tools/interp_bench.py", device=torch.cuda.get_device_name(0), hbm_roof_tbs=HBM_ROOF_TBS,
               hbm_copy_tbs=HBM_COPY_TBS, results=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
