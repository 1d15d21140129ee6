"""Time the JPEG degradation stage: the device kernel (sisr_jpeg_roundtrip, one launch) against the Pillow calls it stands for
(`save(buf, "JPEG", subsampling=0, quality=q)`, `open`, and the `load` that actually decodes), on an LR image of a DIV2K
validation picture at x4, 510 x 339 x 3, and on a 128 x 128 x 3 one; and the cost of the stage inside the degrader: one
OnlineDegrader call on a 2040 x 1356 HR image with and without `jpeg`.

Device: HIP events around each call after a warm-up, >= 100 repeats; median and spread (min, p10, p90, max).  The launch is a
few thousand 8 x 8 blocks, far too little to fill the machine: the time is a launch latency, and no rate is derived from it.
Host: wall clock around the Pillow calls on the same machine, median of a few dozen repeats.  Degrader: a host clock around
the call, ended by a device synchronise, the two forms alternating under the same seed (the draws are part of the call).
Every device output is compared with Pillow's.

    python tools/jpeg_bench.py [--reps 200] [--out profiles/jpeg_bench.json]
"""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)),
                max=float(v.max()))


def pil_roundtrip(hwc, quality):
    import PIL.Image
    buf = io.BytesIO()
    PIL.Image.fromarray(hwc).save(buf, "JPEG", subsampling=0, quality=quality)
    buf.seek(0)
    im = PIL.Image.open(buf)
    im.load()
    return im


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=30)
    ap.add_argument("--degrader-reps", type=int, default=20)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    a = ap.parse_args()
    import PIL
    import torch
    import sisr_amd
    D, hip = sisr_amd.degrade, sisr_amd.hip
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs a HIP device")
    L = hip.lib()
    q = a.quality
    results = []
    for h, w in ((339, 510), (128, 128)):
        # a smooth picture with noise on it rather than white noise: the coefficient statistics of an image, which is what
        # Pillow's entropy coder (the part the kernel leaves out) is sensitive to
        rng = np.random.RandomState(h)
        yy, xx = np.mgrid[:h, :w]
        base = np.stack([127 + 90 * np.sin(xx / 17.0 + c) * np.cos(yy / 23.0 - c) for c in range(3)], -1)
        hwc = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        dev = torch.from_numpy(np.ascontiguousarray(hwc.transpose(2, 0, 1))).cuda()
        want = np.asarray(pil_roundtrip(hwc, q)).transpose(2, 0, 1)
        for to_float in (1, 0):
            out = torch.empty((3, h, w), device="cuda", dtype=torch.float32 if to_float else torch.uint8)
            stream = hip.stream()

            def call():
                hip.check(L.sisr_jpeg_roundtrip(dev.data_ptr(), out.data_ptr(), 3, h, w, q, to_float, stream), "sisr_jpeg_roundtrip")
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                call()
                e1.record()
            torch.cuda.synchronize()
            us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
            got = out.cpu().numpy()
            same = bool(np.array_equal(got, want.astype(np.float32) / np.float32(255) if to_float else want))
            host_s = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                pil_roundtrip(hwc, q)
                host_s.append(time.perf_counter() - t0)
            r = dict(case=f"{w}x{h}x3 {'fp32' if to_float else 'uint8'} out", h=h, w=w, quality=q, to_float=to_float,
                     blocks=((h + 7) // 8) * ((w + 7) // 8), reps=a.reps, warmup=a.warmup, device_us=spread(us),
                     pillow_us=dict(spread(np.array(host_s) * 1e6), reps=a.host_reps), bit_identical_to_pillow=same)
            r["pillow_over_device"] = r["pillow_us"]["median"] / r["device_us"]["median"]
            results.append(r)
            print(f"{r['case']:>24}: device median {r['device_us']['median']:7.1f} us (p10 {r['device_us']['p10']:.1f}, p90 "
                  f"{r['device_us']['p90']:.1f})  Pillow save+open+load {r['pillow_us']['median']:8.1f} us  "
                  f"Pillow/device {r['pillow_over_device']:.0f}x  identical {same}", flush=True)

    # the stage inside the degrader, at a DIV2K validation image's size
    H, W = 1356, 2040
    hr = torch.rand((3, H, W), generator=torch.Generator().manual_seed(0)).cuda()
    pca = torch.from_numpy(np.random.RandomState(0).randn(441, 10).astype(np.float32))
    forms = {"plain": D.OnlineDegrader(scale=4, pca=pca), "jpeg": D.OnlineDegrader(scale=4, pca=pca, jpeg=True)}
    times = {k: [] for k in forms}
    for i in range(a.degrader_reps + 3):
        for name, deg in forms.items():
            np.random.seed(i)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            deg(hr)
            torch.cuda.synchronize()
            if i >= 3:  # the first rounds load code objects and build the resampler's tables
                times[name].append((time.perf_counter() - t0) * 1e6)
    degrader = dict(hr_h=H, hr_w=W, scale=4, reps=a.degrader_reps, plain_us=spread(times["plain"]), jpeg_us=spread(times["jpeg"]))
    degrader["jpeg_minus_plain_us"] = degrader["jpeg_us"]["median"] - degrader["plain_us"]["median"]
    print(f"OnlineDegrader on {W}x{H}: plain median {degrader['plain_us']['median']:.0f} us, with jpeg "
          f"{degrader['jpeg_us']['median']:.0f} us (+{degrader['jpeg_minus_plain_us']:.0f} us)", flush=True)
    doc = dict(tool="tools/jpeg_bench.py", device=torch.cuda.get_device_name(0), pillow=PIL.__version__, results=results,
               degrader=degrader)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
