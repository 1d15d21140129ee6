"""Time one training batch's production for the interpolated-input and Y-channel models under `online_degradations`
(`input = 'interp'`, `degradation_scale = 4`, `scale = 1`), in three forms on the same machine:

  tiles   `device_tiles` + `degrade_tiles`: one degrade launch for the LR windows, one sisr_upsample_tiles launch, one HR gather
          (+ one colour conversion of the HR tiles under 'ycbcr') per batch;
  whole   `device_tiles` alone: per sample the whole image is blurred, down-sampled and up-sampled again on the device
          (sisr_pil_upsample), then two gathers per batch;
  host    the stock host form with the LR bytes GIVEN (no blur, no down-sampling): per sample Pillow's `resize(BICUBIC)`,
          ToTensor, data.rgb_to_ycbcr under 'ycbcr', flips and the matched crop on the host, then the collation.

Set-up: N synthetic 2040 x 1356 HR images (a DIV2K picture's size; written once as BMP files into a temporary folder and read
back by the real SuperResImages / DeviceTileLoader), crop = 128, B in {8, 32}, colorspace 'rgb' and 'ycbcr' (Y alone).  Per
repeat the three forms run under the same seeds, alternating; a batch is timed by a host clock ended by a device synchronise
(and by HIP events for the two device forms).  Warm-up repeats come first; median and spread are reported; the tile and the
whole-image batches are compared bit for bit.
Then the new kernel alone: `--kernel-launches` back-to-back sisr_upsample_tiles launches on fixed windows and records between
two HIP events -> time per launch, bytes written per second, and that as a share of the 8 TB/s HBM roof (the kernel reads
B * C * cw^2 bytes and writes B * C_out * c^2 * 4: the writes are what it moves).

    python tools/interp_tiles_bench.py [--reps 10] [--out profiles/interp_tiles_bench.json]
"""
import argparse
import ctypes
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    v = np.asarray(v, dtype=np.float64)
    return dict(median=float(np.median(v)), min=float(v.min()), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)),
                max=float(v.max()), n=int(v.size))


def write_images(folder, n, H, W):
    """The synthetic pictures of tools/degrade_tiles_bench.py: smooth + noise."""
    import PIL.Image
    yy, xx = np.mgrid[:H, :W]
    for i in range(n):
        rng = np.random.RandomState(i)
        base = np.stack([127 + 90 * np.sin(xx / (17.0 + i) + c) * np.cos(yy / 23.0 - c) for c in range(3)], -1)
        img = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        PIL.Image.fromarray(img).save(os.path.join(folder, "im%03d.bmp" % i))


HBM_ROOF = 8e12  # bytes / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3, help="repeats of the host form (seconds per batch at B = 32)")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--height", type=int, default=1356)
    ap.add_argument("--width", type=int, default=2040)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--crop", type=int, default=128)
    ap.add_argument("--factor", type=int, default=4)
    ap.add_argument("--kernel-launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_tiles_bench.json"))
    a = ap.parse_args()
    import PIL.Image
    import torch
    import sisr_amd
    D, data, hip = sisr_amd.degrade, sisr_amd.data, sisr_amd.hip
    if not torch.cuda.is_available():
        raise SystemExit("interp_tiles_bench needs a HIP device")
    dev = torch.device("cuda:0")
    pca = torch.from_numpy(np.random.RandomState(0).randn(441, 10).astype(np.float32))
    s, c = a.factor, a.crop

    loaders, lr_pil, hr_host = {}, [], []
    with tempfile.TemporaryDirectory() as folder:
        write_images(folder, a.images, a.height, a.width)
        for cs in ("rgb", "ycbcr"):
            for mode in ("whole", "tiles"):
                ds = data.SuperResImages(hr_dir=folder, online_degradations=True, split="all", scale=1, input="interp",
                                         colorspace=cs, random_crop=c, random_augments=True,
                                         online_degradation_params=dict(pca=pca, degradation_scale=s))
                loaders[cs, mode] = data.DeviceTileLoader([ds], a.batches[0], dev, degrade_tiles=mode == "tiles")
        # the host form's givens: the LR bytes of every image (made once, by the device path) and the centre-cropped HR images
        deg = D.OnlineDegrader(scale=s, pca=pca)
        for name in sorted(os.listdir(folder)):
            hr = data.to_tensor(data.read_image(os.path.join(folder, name)))
            lr, _, _, (top, left, rh, rw) = deg(hr.to(dev))
            lr_pil.append(PIL.Image.fromarray(lr.mul(255).byte().permute(1, 2, 0).contiguous().cpu().numpy()))
            hr_host.append(hr[:, top:top + rh, left:left + rw])

    def seed(v):
        torch.manual_seed(v)
        np.random.seed(v)
        random.seed(v)

    def device_batch(cs, mode, v):
        seed(v)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        batch = next(iter(loaders[cs, mode]))
        e1.record()
        torch.cuda.synchronize()
        return batch, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    def host_batch(cs, B, v):
        seed(v)
        t0 = time.perf_counter()
        lrs, hrs = [], []
        for i in range(B):
            im = lr_pil[i % len(lr_pil)]
            lr = data.to_tensor(im.resize((im.width * s, im.height * s), resample=PIL.Image.BICUBIC))
            hr = hr_host[i % len(hr_host)]
            if cs == "ycbcr":
                lr, hr = data.rgb_to_ycbcr(lr, y_only=True), data.rgb_to_ycbcr(hr, y_only=True)
            lr, hr = data.random_flip_rotate(lr, hr)
            lr, hr = data.random_matched_crop(lr, hr, crop_size=c, scale=1)
            lrs.append(lr), hrs.append(hr)
        out = torch.stack(lrs), torch.stack(hrs)
        return out, (time.perf_counter() - t0) * 1e3

    def kernel_alone(B, form):
        """Back-to-back launches of sisr_upsample_tiles on fixed windows, the records uploaded once."""
        h, w = a.height // s, a.width // s
        cw = D.interp_window_edge(c, s)
        C_out = {"rgb": 3, "y": 1}[form]
        rng = np.random.RandomState(B)
        win = torch.from_numpy(rng.randint(0, 256, (B, 3, cw, cw)).astype(np.uint8)).to(dev)
        bh, ch, ks = D._device_table(w, w * s, dev)
        bv, cv, _ = D._device_table(h, h * s, dev)
        recs = (hip.UpsampleTile * B)()
        for b in range(B):
            ty, tx = int(rng.randint(0, h * s - c + 1)), int(rng.randint(0, w * s - c + 1))
            r = recs[b]
            r.bounds_h, r.coef_h, r.bounds_v, r.coef_v = bh.data_ptr(), ch.data_ptr(), bv.data_ptr(), cv.data_ptr()
            r.h, r.w, r.H, r.W, r.ty, r.tx, r.flips = h, w, h * s, w * s, ty, tx, b % 8
            r.wy, r.wx = D.interp_window(h, s, c, ty)[0], D.interp_window(w, s, c, tx)[0]
        rdev = torch.from_numpy(np.frombuffer(bytes(recs), np.uint8).copy()).to(dev)
        out = torch.empty((B, C_out, c, c), device=dev)
        L, st = hip.lib(), hip.stream()

        def launch():
            hip.check(L.sisr_upsample_tiles(ctypes.addressof(recs), rdev.data_ptr(), win.data_ptr(), out.data_ptr(), ks, B, 3, c, cw,
                                            D.UPSAMPLE_FORMS[form], st), "sisr_upsample_tiles")
        for _ in range(20):
            launch()
        per = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.kernel_launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            per.append(e0.elapsed_time(e1) / a.kernel_launches * 1e3)  # microseconds per launch
        written = B * C_out * c * c * 4
        us = float(np.median(per))
        return dict(B=B, form=form, window_edge=cw, launches=1, us_per_launch=spread(per), bytes_written=written,
                    bytes_read=B * 3 * cw * cw, written_bytes_per_second=written / (us * 1e-6),
                    share_of_8TBps_roof=written / (us * 1e-6) / HBM_ROOF)

    results, kernels = [], []
    for B in a.batches:
        for cs in ("rgb", "ycbcr"):
            for mode in ("whole", "tiles"):
                loaders[cs, mode].batch_size = B
            wall = {"host": [], "whole": [], "tiles": []}
            evt = {"whole": [], "tiles": []}
            same = None
            for i in range(a.reps + a.warmup):
                got = {}
                for mode in ("whole", "tiles"):
                    got[mode], wl, ev = device_batch(cs, mode, 100 + i)
                    if i >= a.warmup:
                        wall[mode].append(wl)
                        evt[mode].append(ev)
                if i <= a.host_reps:  # one warm-up, then host_reps timed
                    _, wl = host_batch(cs, B, 100 + i)
                    if i >= 1:
                        wall["host"].append(wl)
                if i == 0:
                    same = bool(torch.equal(got["whole"]["lr"], got["tiles"]["lr"]) and
                                torch.equal(got["whole"]["hr"], got["tiles"]["hr"]) and
                                torch.equal(got["whole"]["metadata"], got["tiles"]["metadata"]))
                    shape = list(got["tiles"]["lr"].shape)
            r = dict(B=B, crop=c, colorspace=cs, lr_shape=shape, tiles_identical_to_whole=same,
                     tiles=dict(wall_ms=spread(wall["tiles"]), events_ms=spread(evt["tiles"])),
                     whole_image=dict(wall_ms=spread(wall["whole"]), events_ms=spread(evt["whole"])),
                     host=dict(wall_ms=spread(wall["host"])))
            r["whole_over_tiles"] = r["whole_image"]["wall_ms"]["median"] / r["tiles"]["wall_ms"]["median"]
            r["host_over_tiles"] = r["host"]["wall_ms"]["median"] / r["tiles"]["wall_ms"]["median"]
            results.append(r)
            print(f"B={B:2d} c={c} {cs:5s}: tiles {r['tiles']['wall_ms']['median']:8.3f} ms (p10 {r['tiles']['wall_ms']['p10']:.3f}, p90 "
                  f"{r['tiles']['wall_ms']['p90']:.3f})  whole-image {r['whole_image']['wall_ms']['median']:9.2f} ms  host "
                  f"{r['host']['wall_ms']['median']:9.1f} ms  x{r['whole_over_tiles']:.1f} / x{r['host_over_tiles']:.0f}  identical= {same}",
                  flush=True)
        for form in ("rgb", "y"):
            k = kernel_alone(B, form)
            kernels.append(k)
            print(f"sisr_upsample_tiles B={B:2d} c={c} {form:3s}: {k['us_per_launch']['median']:.2f} us per launch, "
                  f"{k['written_bytes_per_second'] / 1e9:.1f} GB/s written = {100 * k['share_of_8TBps_roof']:.2f} % of the 8 TB/s roof",
                  flush=True)

    doc = dict(tool="tools/interp_tiles_bench.py", device=torch.cuda.get_device_name(0), hr_size=[a.height, a.width], factor=s,
               crop=c, images=a.images, reps=a.reps, warmup=a.warmup, host_reps=a.host_reps, kernel_launches=a.kernel_launches, batches=results,
               upsample_tiles_kernel=kernels)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
