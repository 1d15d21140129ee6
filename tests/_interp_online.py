"""Shared pieces of the tests of online degradation for interpolated-input and Y-channel models (test_interp_online_cpu.py,
test_interp_online_gpu.py; helper module, not collected).

Expected values never come from the code under test: the up-sampled image is Pillow's `resize(BICUBIC)` of the LR bytes that
the EXISTING entry points make, the colour forms are data.rgb_to_ycbcr on the host, and a tile is read out of them with the
index map of tests/_degrade_tiles.py::gather_on_host."""
import numpy as np
import torch

import sisr_amd
from _degrade_tiles import FLIPS, draw_for_origin, gather_on_host

D = sisr_amd.degrade
data = sisr_amd.data


def pillow_upsample(lr_u8, scale):
    """(C, h, w) uint8 -> Pillow's resize((w * s, h * s), BICUBIC), (C, s h, s w) uint8."""
    from PIL import Image
    a = np.asarray(lr_u8)
    im = Image.fromarray(a[0] if a.shape[0] == 1 else np.ascontiguousarray(a.transpose(1, 2, 0)))
    up = np.asarray(im.resize((im.width * scale, im.height * scale), resample=Image.BICUBIC))
    return up[None] if up.ndim == 2 else np.ascontiguousarray(up.transpose(2, 0, 1))


def to_tensor_u8(u8):
    """ToTensor of a planar uint8 image."""
    return torch.from_numpy(np.asarray(u8)).to(torch.float32).div(255)


def host_form(rgb, form):
    """The data set's colour conversion on the host: 'rgb' | 'ycbcr' | 'y' of a (3, H, W) fp32 host image."""
    return rgb if form == "rgb" else data.rgb_to_ycbcr(rgb, y_only=form == "y", im_type="jpg")


def window_upsample_host(win, h, w, scale, wy, wx, ty, tx, c):
    """numpy restatement of both passes of libImaging/Resample.c's 8-bit resampler for the c x c tile at (ty, tx) of the
    (h, w) -> (s h, s w) up-sampling, from the LR window `win` (C, cwy, cwx) uint8 whose origin in the LR image is (wy, wx):
    whole-image tables, tap addresses relative to the window -> (C, c, c) uint8."""
    bv, cv, _ = D.pil_bicubic_table(h, h * scale)
    bh, ch, _ = D.pil_bicubic_table(w, w * scale)
    win = np.asarray(win).astype(np.int64)
    C, rows, _ = win.shape
    tmp = np.zeros((C, rows, c), np.int64)
    for x in range(c):
        lo, n = bh[tx + x]
        ss = np.full((C, rows), 1 << 21, np.int64)
        for k in range(n):
            ss += win[:, :, lo - wx + k] * int(ch[tx + x, k])
        tmp[:, :, x] = np.clip(ss >> 22, 0, 255)
    out = np.zeros((C, c, c), np.int64)
    for y in range(c):
        lo, n = bv[ty + y]
        ss = np.full((C, c), 1 << 21, np.int64)
        for k in range(n):
            ss += tmp[:, lo - wy + k, :] * int(cv[ty + y, k])
        out[:, y, :] = np.clip(ss >> 22, 0, 255)
    return out.astype(np.uint8)


def origins_1d(size, c, scale):
    """Tile origins along one axis of a `size`-pixel up-sampled image: every origin congruent to 0, 1 or s - 1 modulo s that
    lies within one tap span (5 LR pixels = 5 s outputs) of either border, and one interior origin of each residue."""
    last = size - c
    res = {0, 1 % scale, scale - 1}
    near = [o for o in range(last + 1) if o % scale in res and (o < 5 * scale or o > last - 5 * scale)]
    mid = last // 2
    inner = [o for o in range(mid, min(mid + scale, last + 1)) if o % scale in res]
    return sorted(set(near + inner + [0, last]))


def origin_pairs(H, W, c, scale):
    """(ty, tx) pairs that visit every origin of origins_1d along each axis at least once, the four corners included."""
    ys, xs = origins_1d(H, c, scale), origins_1d(W, c, scale)
    n = max(len(ys), len(xs))
    pairs = [(ys[i % len(ys)], xs[(3 * i + 1) % len(xs)]) for i in range(n)]
    pairs += [(ys[(5 * i + 2) % len(ys)], xs[i % len(xs)]) for i in range(n)]
    pairs += [(0, 0), (0, W - c), (H - c, 0), (H - c, W - c)]
    assert {p[0] for p in pairs} >= set(ys) and {p[1] for p in pairs} >= set(xs)
    return pairs


def with_flips(pairs):
    """Every pair with one of the eight flip / transpose combinations in turn; the first pair and the four corners (the last
    four) with all eight."""
    out = [(p, FLIPS[i % 8]) for i, p in enumerate(pairs)]
    for p in [pairs[0]] + pairs[-4:]:
        out += [(p, fl) for fl in FLIPS]
    return out


def expected_tile(image, ty, tx, c, flips):
    """The c x c tile with source origin (ty, tx) of a (C, H, W) host image through the flips, with the index map of
    sisr_crop_augment (gather_on_host) -- the draw (top, left) that reads that square is solved for independently of
    data.tile_source_box."""
    _, H, W = image.shape
    top, left = draw_for_origin(H, W, c, ty, tx, *flips)
    return gather_on_host(image, (H, W, top, left) + tuple(flips), c)
