"""Shared by test_jpeg_cpu.py and test_jpeg_gpu.py: Pillow's JPEG round trip (the reference's call) and the test images."""
import io
import os

import numpy as np

from conftest import GOLDEN

SIZES = [(1, 1), (7, 9), (8, 8), (9, 7), (16, 24), (37, 41)]  # below a block, across block edges either way, whole blocks, odd
QUALITIES = [1, 10, 49, 50, 51, 75, 95, 100]                  # both branches of the table scaling and their meeting point
PATTERN_QUALITIES = [1, 2, 3]                                 # coarsest tables: the inverse DCT's largest excursions
BABY = os.path.join(GOLDEN, "set5", "lr_random_blur", "baby.png")


def pil_roundtrip(u8, quality):
    """(C, H, W) uint8, C = 3 (RGB) or 1 (mode L) -> the image PIL opens after save(buf, "JPEG", subsampling=0, quality)
    (ref: sr_tools/data_converter.py:186-192)."""
    import PIL.Image
    im = PIL.Image.fromarray(u8[0], "L") if u8.shape[0] == 1 else PIL.Image.fromarray(np.ascontiguousarray(u8.transpose(1, 2, 0)), "RGB")
    buf = io.BytesIO()
    im.save(buf, "JPEG", subsampling=0, quality=quality)
    buf.seek(0)
    out = np.asarray(PIL.Image.open(buf))
    return np.ascontiguousarray(out[None] if out.ndim == 2 else out.transpose(2, 0, 1))


def random_image(C, hw, seed=0):
    rng = np.random.RandomState(1000 * hw[0] + 10 * hw[1] + C + seed)
    return rng.randint(0, 256, size=(C,) + tuple(hw)).astype(np.uint8)


def baby():
    import PIL.Image
    return np.ascontiguousarray(np.asarray(PIL.Image.open(BABY).convert("RGB")).transpose(2, 0, 1))


def patterns(C, hw=(19, 22)):
    """name -> (C, H, W) uint8: saturated checkerboards and stripes (all the energy in the highest frequencies) and the two
    constant extremes; the colour planes of the C = 3 forms are out of phase, so the chroma planes are patterned too."""
    H, W = hw
    yy, xx = np.mgrid[:H, :W]
    board = ((yy + xx) % 2 * 255).astype(np.uint8)
    stripe = (xx % 2 * 255).astype(np.uint8) + np.zeros_like(board)
    rows = (yy % 2 * 255).astype(np.uint8) + np.zeros_like(board)

    def planes(p):
        return np.stack([p, 255 - p, p][:C]) if C == 3 else p[None]
    return {"checkerboard": planes(board), "stripes": planes(stripe), "row_stripes": planes(rows),
            "all_0": np.zeros((C, H, W), np.uint8), "all_255": np.full((C, H, W), 255, np.uint8)}


def cases(C, sizes=SIZES):
    """[(label, image, quality)]: random images of every size at every quality (the Set5 LR baby.png with C = 3), and the
    patterns at the lowest qualities."""
    out = [(f"random{hw}", random_image(C, hw), q) for hw in sizes for q in QUALITIES]
    if C == 3:
        out += [("baby", baby(), q) for q in QUALITIES]
    out += [(name, img, q) for name, img in patterns(C).items() for q in PATTERN_QUALITIES]
    return out
