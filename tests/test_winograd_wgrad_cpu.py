"""The transform algebra of the Winograd F(2x2,3x3) weight gradient (csrc/wgrad3x3_mfma.hip, wgrad3x3_c64_w4_kernel) in
float64 on the CPU: per 2 x 2 output block, V = B^T d B of the zero-padded 4 x 4 input patch at stride 2 and M = A dY A^T
(with A's last row negated, as the kernel stages it); dg = G^T [sum_blocks M . V] G (with the matching sign on G's last
row) must equal the direct weight gradient, on odd and even map sizes."""
import numpy as np
import pytest
import torch

import _exact as X

# the kernel's matrices: rows of B^T (xr 0: d0 - d2, 1: d1 + d2, 2: d2 - d1, 3: d1 - d3)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
# A dY A^T with A's last row read as (0, +1): rows xr 0: y0, 1: y0 + y1, 2: y0 - y1, 3: y1
AS = np.array([[1, 0], [1, 1], [1, -1], [0, 1]], dtype=np.float64)
# the fold f0 = u0 + (u1 + u2) / 2, f1 = (u1 - u2) / 2, f2 = (u1 + u2) / 2 - u3: G with its last row negated
GS = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, -1]], dtype=np.float64)


def winograd_wgrad(x, dy):
    """x (B, C, H, W), dy (B, O, H, W) float64 numpy -> dw (O, C, 3, 3)"""
    B, C, H, W = x.shape
    O = dy.shape[1]
    Hb, Wb = (H + 1) // 2, (W + 1) // 2
    # dY outside the map is zero (half-covered blocks); x padded by one on top / left and up to the block grid + 1 below
    dyp = np.zeros((B, O, 2 * Hb, 2 * Wb))
    dyp[:, :, :H, :W] = dy
    xp = np.zeros((B, C, 2 * Hb + 2, 2 * Wb + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    dU = np.zeros((4, 4, O, C))
    for bh in range(Hb):
        for bw in range(Wb):
            d = xp[:, :, 2 * bh:2 * bh + 4, 2 * bw:2 * bw + 4]        # (B, C, 4, 4)
            y = dyp[:, :, 2 * bh:2 * bh + 2, 2 * bw:2 * bw + 2]       # (B, O, 2, 2)
            V = np.einsum("rk,bckl,sl->bcrs", BT, d, BT)
            M = np.einsum("ri,boij,sj->bors", AS, y, AS)
            dU += np.einsum("bors,bcrs->rsoc", M, V)
    return np.einsum("ra,rsoc,sb->ocab", GS, dU, GS)


@pytest.mark.parametrize("B,C,O,H,W", [(1, 3, 2, 4, 4), (2, 4, 3, 7, 9), (1, 2, 5, 5, 1), (3, 3, 3, 1, 6), (1, 5, 4, 10, 13)])
def test_transform_algebra_matches_the_direct_weight_gradient(B, C, O, H, W):
    g = np.random.default_rng(1000 + H * 31 + W)
    x, dy = g.standard_normal((B, C, H, W)), g.standard_normal((B, O, H, W))
    want = X.wgrad_ref(torch.from_numpy(x), torch.from_numpy(dy)).numpy()
    np.testing.assert_allclose(winograd_wgrad(x, dy), want, rtol=1e-12, atol=1e-12)


def test_transform_coefficients_are_exact_in_fp32():
    """0, +-1 and 1/2 only: every transform step is one exact scaling or one fp32 addition"""
    for m in (BT, AS, GS):
        assert set(np.unique(np.abs(m))) <= {0.0, 0.5, 1.0}
