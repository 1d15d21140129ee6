"""Time the device SSIM (sisr_ssim: tile launch + per-image reduction) against the host float64 form (metrics.ssim).

Device: HIP events around each call after a warm-up, >= 100 repeats per size; median and spread (min, p10, p90, max).
Host: wall clock around metrics.ssim on the same Y planes (a few repeats: it takes about a second per DIV2K image).
Rates: bytes = the two input batches read once (the floor: n * channels * h * w * 4 B each); fp64 FLOP = what the
algorithm needs per valid window, 5 maps x 2 separable passes x 11 taps x 2 + 3 products + 17 for S = 240 (halo rows and
columns that a tile filters again are not counted).  The guide gives no fp64 peak, so no share of peak is claimed.

    python tools/ssim_bench.py [--reps 200] [--out profiles/ssim_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.29  # MI355X_MICROARCH.md: measured HBM read bandwidth
FLOP_PER_WINDOW = 5 * 2 * 11 * 2 + 3 + 17


def _case(g, name, n, c, h, w):
    if c == 3:  # SR output with overshoot against an HR image
        hr = g.random((n, 3, h, w), dtype=np.float32)
        sr = np.clip(hr + np.float32(0.1) * g.standard_normal(hr.shape).astype(np.float32), -0.1, 1.1)
    else:
        hr = g.random((n, 1, h, w), dtype=np.float32)
        sr = np.clip(hr + np.float32(0.1) * g.standard_normal(hr.shape).astype(np.float32), 0, 1)
    return dict(name=name, n=n, c=c, h=h, w=w, sr=sr.astype(np.float32), hr=hr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_bench.json"))
    a = ap.parse_args()
    import torch
    import sisr_amd
    M, hip = sisr_amd.metrics, sisr_amd.hip
    if not torch.cuda.is_available():
        raise SystemExit("ssim_bench needs a HIP device")
    L = hip.lib()
    g = np.random.default_rng(0)
    cases = [_case(g, "div2k_2040x1356_rgb", 1, 3, 1356, 2040), _case(g, "512x512_rgb", 1, 3, 512, 512),
             _case(g, "16x128x128_y", 16, 1, 128, 128)]
    results = []
    for cs in cases:
        n, c, h, w = cs["n"], cs["c"], cs["h"], cs["w"]
        da, db = torch.from_numpy(cs["sr"]).cuda(), torch.from_numpy(cs["hr"]).cuda()
        nbytes = L.sisr_ssim_workspace_bytes(n, h, w)
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        stream = hip.stream()

        def call():
            hip.check(L.sisr_ssim(da.data_ptr(), db.data_ptr(), n, c, h, w, 1.0, out.data_ptr(), ws.data_ptr(), nbytes,
                                  stream), "sisr_ssim")
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
        dev_vals = out.cpu().numpy()
        # host float64 form on the same Y planes
        ys = M.batch_rgb_to_ycbcr(cs["sr"])[:, 0] if c == 3 else cs["sr"][:, 0]
        yh = M.batch_rgb_to_ycbcr(cs["hr"])[:, 0] if c == 3 else cs["hr"][:, 0]
        host_s = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            host_vals = [M.ssim(ys[i], yh[i]) for i in range(n)]
            host_s.append(time.perf_counter() - t0)
        med = float(np.median(us))
        bytes_floor = 2 * n * c * h * w * 4
        flop = FLOP_PER_WINDOW * n * (h - 10) * (w - 10)
        r = dict(case=cs["name"], n=n, channels=c, h=h, w=w, reps=a.reps, warmup=a.warmup,
                 device_us=dict(median=med, min=float(us.min()), p10=float(np.percentile(us, 10)),
                                p90=float(np.percentile(us, 90)), max=float(us.max())),
                 bytes_floor=bytes_floor, floor_us_at_hbm=bytes_floor / (HBM_TBS * 1e12) * 1e6,
                 achieved_gbs=bytes_floor / (med * 1e-6) / 1e9, fp64_flop=flop, achieved_fp64_gflops=flop / (med * 1e-6) / 1e9,
                 host_float64_s=dict(median=float(np.median(host_s)), min=float(min(host_s)), reps=a.host_reps),
                 host_over_device=float(np.median(host_s)) / (med * 1e-6),
                 max_abs_device_minus_host=float(np.max(np.abs(dev_vals - np.array(host_vals)))))
        results.append(r)
        print(f"{cs['name']:>22}: device median {med:8.1f} us (p10 {r['device_us']['p10']:.1f}, p90 {r['device_us']['p90']:.1f})"
              f"  floor {r['floor_us_at_hbm']:.1f} us  {r['achieved_gbs']:7.1f} GB/s  {r['achieved_fp64_gflops']:8.1f} fp64 GFLOP/s"
              f"  host {r['host_float64_s']['median'] * 1e3:8.1f} ms  |dev-host| {r['max_abs_device_minus_host']:.1e}",
              flush=True)
    doc = dict(tool="tools/ssim_bench.py", device=torch.cuda.get_device_name(0), hbm_tbs_reference=HBM_TBS,
               flop_per_window=FLOP_PER_WINDOW, results=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
