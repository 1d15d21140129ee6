"""Make a fixed JPEG-degraded evaluation set from a folder of LR images: every image goes through the JPEG round trip
(`save(buf, "JPEG", subsampling=0, quality=q)` + `open`, as the reference's data_converter.py jpeg_compress stage does it) at
each of the given qualities and is written losslessly, with the quality on record in a `degradation_metadata.csv`.

Layout, as the reference's converter writes it and SuperResImages / eval_sisr read it: `<name>_q<i>.png` for quality number i
of several (`<name>.png` for a single quality), and a CSV with the columns `image` (the file name, the index) and
`jpeg_quality` (an integer, which the reader min-max normalises over the file).

The pixels come from the device kernel (degrade.jpeg_roundtrip) when a HIP device is present and from its numpy statement
(degrade.jpeg_roundtrip_host) otherwise; the two are bit-identical to each other and to Pillow, so the files do not depend on
which one ran.

    python tools/make_jpeg_set.py LR_DIR OUT_DIR --quality 10 60 [--host]
"""
import argparse
import csv
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_jpeg_set(lr_dir, out_dir, qualities, host=None):
    """-> the list of (file name, quality) written to out_dir.  host: True / False forces the numpy form / the device kernel;
    None takes the device when there is one."""
    import PIL.Image
    import torch
    import sisr_amd
    D = sisr_amd.degrade
    qualities = [D._check_quality(q) for q in qualities]
    if not qualities:
        raise ValueError("give at least one quality")
    if host is None:
        host = not torch.cuda.is_available()
    names = sisr_amd.data.image_names(lr_dir)
    if not names:
        raise RuntimeError(f"no images in {lr_dir}")
    os.makedirs(out_dir, exist_ok=True)
    rows = []
    for path in names:
        im = PIL.Image.open(path)
        grey = im.mode == "L"
        arr = np.asarray(im if grey else im.convert("RGB"))
        planar = np.ascontiguousarray(arr[None] if grey else arr.transpose(2, 0, 1))
        dev = None if host else torch.from_numpy(planar).cuda()
        stem = os.path.splitext(os.path.basename(path))[0]
        for i, q in enumerate(qualities):
            out = D.jpeg_roundtrip_host(planar, q) if host else D.jpeg_roundtrip(dev, q, to_float=False).cpu().numpy()
            name = stem + ("_q%d" % i if len(qualities) > 1 else "") + ".png"
            PIL.Image.fromarray(out[0] if grey else np.ascontiguousarray(out.transpose(1, 2, 0))).save(os.path.join(out_dir, name))
            rows.append((name, q))
    with open(os.path.join(out_dir, "degradation_metadata.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["image", "jpeg_quality"])
        w.writerows(rows)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("lr_dir")
    ap.add_argument("out_dir")
    ap.add_argument("--quality", type=int, nargs="+", required=True, help="one or more JPEG qualities, 1..100")
    ap.add_argument("--host", action="store_true", help="use the numpy form even when a HIP device is present")
    a = ap.parse_args()
    rows = make_jpeg_set(a.lr_dir, a.out_dir, a.quality, host=True if a.host else None)
    print(f"wrote {len(rows)} images and degradation_metadata.csv to {a.out_dir}")


if __name__ == "__main__":
    main()
