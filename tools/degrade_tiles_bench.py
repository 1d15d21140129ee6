"""Time one training batch's production under `online_degradations` + `device_tiles`: the whole-image mode (per sample: blur of
the full HR image, [host-drawn noise field + upload], two resample launches, [JPEG], a copy of the cropped HR image; then two
gathers) against `degrade_tiles = true` (one degrade launch, [one JPEG launch], one HR gather per batch), on the same draws.

Set-up: N synthetic 2040 x 1356 HR images (a DIV2K picture's size; smooth + noise, written once as BMP files into a temporary
folder and read back by the real SuperResImages / DeviceTileLoader), x 4.  Configurations: B in {8, 32}, tile edge in {48, 64},
noise and JPEG each off / on.  One pair of loaders is built; batch size, tile edge and degrader are swapped in per configuration
(the images stay resident).  Per repeat both modes run under the same seeds, alternating; a batch is timed by HIP events around
`next(iter(loader))` and by a host clock ended by a device synchronise (the host clock is the one that counts: the whole-image
mode's cost is largely host work between its launches).  Warm-up repeats come first; median and spread are reported.  Without
JPEG the two modes' LR and HR batches are compared bit for bit (with noise only HR: the fields differ by design).
Then: a QEDSR training step fed by each loader (batch production + step, host clock with a final synchronise).

    python tools/degrade_tiles_bench.py [--reps 10] [--out profiles/degrade_tiles_bench.json]
"""
import argparse
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
    import PIL.Image
    yy, xx = np.mgrid[:H, :W]
    for i in range(n):
        rng = np.random.RandomState(i)
        base = np.stack([127 + 90 * np.sin(xx / (17.0 + i) + c) * np.cos(yy / 23.0 - c) for c in range(3)], -1)
        img = np.clip(base + rng.normal(0, 12, base.shape), 0, 255).astype(np.uint8)
        PIL.Image.fromarray(img).save(os.path.join(folder, "im%03d.bmp" % i))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-noise-reps", type=int, default=2, help="repeats of the whole-image mode with noise (seconds per batch)")
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--height", type=int, default=1356)
    ap.add_argument("--width", type=int, default=2040)
    ap.add_argument("--batches", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--tiles", type=int, nargs="+", default=[48, 64])
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--only-tiles", action="store_true", help="skip the whole-image mode (for a kernel trace of the new mode)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "degrade_tiles_bench.json"))
    a = ap.parse_args()
    import torch
    import sisr_amd
    D, data = sisr_amd.degrade, sisr_amd.data
    if not torch.cuda.is_available():
        raise SystemExit("degrade_tiles_bench needs a HIP device")
    dev = torch.device("cuda:0")
    pca = torch.from_numpy(np.random.RandomState(0).randn(441, 10).astype(np.float32))

    with tempfile.TemporaryDirectory() as folder:
        write_images(folder, a.images, a.height, a.width)
        loaders = {}
        for mode in ("whole", "tiles"):
            ds = data.SuperResImages(hr_dir=folder, online_degradations=True, split="all", scale=4, random_crop=a.tiles[0],
                                     random_augments=True, online_degradation_params=dict(pca=pca))
            loaders[mode] = data.DeviceTileLoader([ds], a.batches[0], dev, degrade_tiles=mode == "tiles")

    def configure(B, c, noise, jpeg):
        deg = D.OnlineDegrader(scale=4, pca=pca, noise=noise, jpeg=jpeg)
        for ld in loaders.values():
            ld.batch_size, ld.sampler.crop, ld.degraders = B, c, [deg] * len(ld.degraders)

    def one_batch(mode, seed):
        torch.manual_seed(seed)
        np.random.seed(seed)
        random.seed(seed)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        batch = next(iter(loaders[mode]))
        e1.record()
        torch.cuda.synchronize()
        return batch, (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)

    results = []
    for B in a.batches:
        for c in a.tiles:
            for noise in (False, True):
                for jpeg in (False, True):
                    configure(B, c, noise, jpeg)
                    reps = {"whole": a.host_noise_reps if noise else a.reps, "tiles": a.reps}
                    warm = {"whole": 1 if noise else a.warmup, "tiles": a.warmup}
                    if a.only_tiles:
                        reps["whole"] = warm["whole"] = 0
                    wall, evt = {"whole": [], "tiles": []}, {"whole": [], "tiles": []}
                    same_lr = same_hr = same_meta = None
                    for i in range(max(reps[m] + warm[m] for m in reps)):
                        got = {}
                        for mode in ("whole", "tiles"):
                            if i >= reps[mode] + warm[mode]:
                                continue
                            got[mode], w, e = one_batch(mode, 100 + i)
                            if i >= warm[mode]:
                                wall[mode].append(w)
                                evt[mode].append(e)
                        if i == 0 and not a.only_tiles:
                            same_hr = bool(torch.equal(got["whole"]["hr"], got["tiles"]["hr"]))
                            same_meta = bool(torch.equal(got["whole"]["metadata"], got["tiles"]["metadata"]))
                            same_lr = bool(torch.equal(got["whole"]["lr"], got["tiles"]["lr"])) if not (noise or jpeg) else None
                    r = None if a.only_tiles else dict(B=B, tile=c, noise=noise, jpeg=jpeg, hr_identical=same_hr, metadata_identical=same_meta,
                             lr_identical=same_lr,
                             whole_image=dict(wall_ms=spread(wall["whole"]), events_ms=spread(evt["whole"])),
                             tiles=dict(wall_ms=spread(wall["tiles"]), events_ms=spread(evt["tiles"])))
                    if a.only_tiles:
                        print(f"B={B:2d} c={c} noise={int(noise)} jpeg={int(jpeg)}: tiles wall {spread(wall['tiles'])['median']:.3f} ms", flush=True)
                        continue
                    r["wall_ratio"] = r["whole_image"]["wall_ms"]["median"] / r["tiles"]["wall_ms"]["median"]
                    results.append(r)
                    print(f"B={B:2d} c={c} noise={int(noise)} jpeg={int(jpeg)}: whole-image wall {r['whole_image']['wall_ms']['median']:9.2f} ms "
                          f"(events {r['whole_image']['events_ms']['median']:9.2f})  tiles wall {r['tiles']['wall_ms']['median']:7.3f} ms "
                          f"(p10 {r['tiles']['wall_ms']['p10']:.3f}, p90 {r['tiles']['wall_ms']['p90']:.3f}; events "
                          f"{r['tiles']['events_ms']['median']:7.3f})  x{r['wall_ratio']:.1f}  hr= {same_hr} lr= {same_lr}", flush=True)

    if a.only_tiles:
        return
    steps = []
    if not a.no_step:
        torch.manual_seed(8)
        h = sisr_amd.available_models["qedsr"](device=0, model_save_dir=tempfile.gettempdir(), eval_mode=False, scale=4,
                                               metadata=["blur_kernel"])
        for B in a.batches:
            configure(B, 64, False, False)
            times = {"whole": [], "tiles": [], "step_only": []}
            for i in range(a.reps + a.warmup):
                for mode in ("whole", "tiles"):
                    torch.manual_seed(200 + i)
                    np.random.seed(200 + i)
                    random.seed(200 + i)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    b = next(iter(loaders[mode]))
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    h.train_step(b["lr"], b["hr"], metadata=b["metadata"], metadata_keys=b["metadata_keys"])
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if i >= a.warmup:
                        times[mode].append((t2 - t0) * 1e3)
                        times["step_only"].append((t2 - t1) * 1e3)
            s = dict(B=B, tile=64, model="qedsr", batch_plus_step_ms={m: spread(times[m]) for m in ("whole", "tiles")},
                     step_only_ms=spread(times["step_only"]))
            steps.append(s)
            print(f"QEDSR B={B} c=64: batch + step, whole-image {s['batch_plus_step_ms']['whole']['median']:.2f} ms, tiles "
                  f"{s['batch_plus_step_ms']['tiles']['median']:.2f} ms; the step alone {s['step_only_ms']['median']:.2f} ms", flush=True)

    doc = dict(tool="tools/degrade_tiles_bench.py", device=torch.cuda.get_device_name(0), hr_size=[a.height, a.width], scale=4,
               images=a.images, reps=a.reps, warmup=a.warmup, host_noise_reps=a.host_noise_reps, batches=results, steps=steps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
