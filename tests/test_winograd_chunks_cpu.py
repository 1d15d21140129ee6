"""Chunked Winograd weights of the fused-shuffle upsampler convs (pack_conv3x3_many_kernel, SISR_PACK_WINOGRAD with r > 1):
a numpy float32 restatement of U = G g G^T in the kernel's summation order, of the (q, c) block offsets and of the two channel
maps, checked on integer data against the direct conv through PixelShuffle and against its input gradient."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

BLOCK = 16 * 64 * 64  # floats of one transformed 64 x 64 block, layout [xi 16][G 4][q4 4][co 64][e 4], ci = 16 G + 4 q4 + e
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def gmul(x, a, b, c):
    """Row x of G = {{1, 0, 0}, {1/2, 1/2, 1/2}, {1/2, -1/2, 1/2}, {0, 0, 1}} times (a, b, c), float32, the kernel's order."""
    if x == 0:
        return a
    if x == 3:
        return c
    h = np.float32(0.5)
    return h * ((a + b) + c) if x == 1 else h * ((a - b) + c)


def transform(g):
    """g: (..., 3, 3) float32 -> U: (4, 4, ...) float32, columns first: rk[kh] = G[xc] . g[kh, :], U[xr][xc] = G[xr] . rk."""
    g = g.astype(np.float32)
    u = np.empty((4, 4) + g.shape[:-2], np.float32)
    for xc in range(4):
        rk = [gmul(xc, g[..., kh, 0], g[..., kh, 1], g[..., kh, 2]) for kh in range(3)]
        for xr in range(4):
            u[xr, xc] = gmul(xr, rk[0], rk[1], rk[2])
    return u


def forward_channel(q, n, r):
    """Original output channel held by slot n of output chunk q of the forward packing."""
    return n * r * r + q


def dgrad_channel(c, k, r):
    """Original output channel held by slot k of input chunk c of the input-gradient packing."""
    return k * r * r + c


def block_offset(q, c, cin_chunks):
    return (q * cin_chunks + c) * BLOCK


def pair_weight(w, r, q, c, dgrad):
    """The 64 x 64 x 3 x 3 weight g[co][ci] that block (q, c) transforms.  w: (64 r^2, 64, 3, 3)."""
    rr = r * r
    co, ci = np.arange(64)[:, None], np.arange(64)[None, :]
    if not dgrad:  # output chunk q of rr, input chunk c of 1
        return w[forward_channel(q, co, r), c * 64 + ci]
    # output chunk q of 1 (original input channels), input chunk c of rr (original output channels); taps flipped
    return w[dgrad_channel(c, ci, r), q * 64 + co][..., ::-1, ::-1]


def chunked_u(w, r, dgrad):
    """The floats behind the direct packing of a (64 r^2, 64, 3, 3) weight, forward or input-gradient order."""
    w = np.asarray(w, np.float32)
    rr = r * r
    oc, ic = (1, rr) if dgrad else (rr, 1)  # output / input chunks of the launch that reads the packing
    out = np.empty(rr * BLOCK, np.float32)
    for q in range(oc):
        for c in range(ic):
            u = transform(pair_weight(w, r, q, c, dgrad))  # [xr][xc][co][ci]
            blk = u.reshape(16, 64, 4, 4, 4).transpose(0, 2, 3, 1, 4)  # [xi][co][G][q4][e] -> [xi][G][q4][co][e]
            o = block_offset(q, c, ic)
            out[o:o + BLOCK] = blk.reshape(-1)
    return out


def block_as_matrix(flat, q, c, cin_chunks):
    """U[xi][ci][co] (float64) of block (q, c)."""
    o = block_offset(q, c, cin_chunks)
    blk = flat[o:o + BLOCK].reshape(16, 4, 4, 64, 4)  # [xi][G][q4][co][e]
    return blk.transpose(0, 1, 2, 4, 3).reshape(16, 64, 64).astype(np.float64)


def winograd_block(x, u):
    """x: (B, 64, H, W) float64 with even H, W; u: [xi][ci][co] -> the zero-padded 3 x 3 conv (B, 64, H, W) as F(2x2,3x3)."""
    B, C, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    y = np.zeros((B, 64, H, W))
    for th in range(H // 2):
        for tw in range(W // 2):
            d = xp[:, :, 2 * th:2 * th + 4, 2 * tw:2 * tw + 4]
            v = np.einsum("ai,bcij,dj->bcad", BT, d, BT).reshape(B, C, 16)
            m = np.einsum("bcx,xco->box", v, u).reshape(B, 64, 4, 4)
            y[:, :, 2 * th:2 * th + 2, 2 * tw:2 * tw + 2] = np.einsum("ai,boij,dj->boad", AT, m, AT)
    return y


def integer_case(r, seed):
    g = np.random.default_rng(seed)
    w = (4 * g.integers(-2, 3, size=(64 * r * r, 64, 3, 3))).astype(np.float32)  # multiples of 4: the 1/4 of G g G^T stays exact
    return g, w


@pytest.mark.parametrize("r", [2, 3])
def test_channel_maps_are_permutations(r):
    rr = r * r
    fwd = sorted(forward_channel(q, n, r) for q in range(rr) for n in range(64))
    dg = sorted(dgrad_channel(c, k, r) for c in range(rr) for k in range(64))
    assert fwd == list(range(64 * rr)) and dg == list(range(64 * rr))
    offs = sorted(block_offset(q, 0, 1) for q in range(rr))
    assert offs == [k * BLOCK for k in range(rr)] == sorted(block_offset(0, c, rr) for c in range(rr))


@pytest.mark.parametrize("r", [2, 3])
def test_transform_sum_equals_the_direct_forward(r):
    """Per output chunk q: A^T (sum_ci V U_q) A, stored at the shuffled position, is conv2d + pixel_shuffle exactly."""
    g, w = integer_case(r, 1)
    rr = r * r
    x = g.integers(-3, 4, size=(2, 64, 4, 6)).astype(np.float64)
    flat = chunked_u(w, r, dgrad=False)
    want = F.pixel_shuffle(F.conv2d(torch.from_numpy(x), torch.from_numpy(w).double(), padding=1), r).numpy()
    got = np.full_like(want, np.nan)
    for q in range(rr):
        got[:, :, q // r::r, q % r::r] = winograd_block(x, block_as_matrix(flat, q, 0, 1))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("r", [2, 3])
def test_transform_sum_equals_the_direct_input_gradient(r):
    """The folds of the r^2 input chunks, read through the shuffle view, add up to the transposed conv of the un-shuffled dy."""
    g, w = integer_case(r, 2)
    rr = r * r
    dy = g.integers(-3, 4, size=(2, 64, 4 * r, 6 * r)).astype(np.float64)
    flat = chunked_u(w, r, dgrad=True)
    want = F.conv_transpose2d(F.pixel_unshuffle(torch.from_numpy(dy), r), torch.from_numpy(w).double(), padding=1).numpy()
    got = np.zeros_like(want)
    for c in range(rr):
        got += winograd_block(dy[:, :, c // r::r, c % r::r], block_as_matrix(flat, 0, c, rr))
    assert np.array_equal(got, want)


def test_one_chunk_pair_is_the_64_to_64_layout():
    """r = 1: one block, thread k = (G * 4 + q4) * 256 + co * 4 + e of plane xi holds U[xi][ci = 16 G + 4 q4 + e][co]."""
    g = np.random.default_rng(3)
    w = g.standard_normal((64, 64, 3, 3)).astype(np.float32)
    flat = chunked_u(w, 1, dgrad=False)
    u = transform(w)  # [xr][xc][co][ci]
    for xi, G, q4, co, e in [(0, 0, 0, 0, 0), (5, 1, 2, 33, 3), (15, 3, 3, 63, 1), (9, 2, 0, 17, 2)]:
        assert flat[xi * 4096 + (G * 4 + q4) * 256 + co * 4 + e] == u[xi >> 2, xi & 3, co, 16 * G + 4 * q4 + e]
    ud = transform(np.ascontiguousarray(w.transpose(1, 0, 2, 3)[..., ::-1, ::-1]))
    assert np.array_equal(chunked_u(w, 1, dgrad=True).reshape(16, 4, 4, 64, 4)[7, 2, 1, 40, 3], ud[1, 3, 40, 39])
