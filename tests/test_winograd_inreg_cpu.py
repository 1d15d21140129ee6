"""The lane -> LDS address map of the A-fragment reads of conv3x3_c64_w4_kernel, restated: lane (n = l & 15, q = l >> 4) of
wave (mb, coh) reads, for step (xr, G) and j = 0..3, the 16-byte piece (4G + q) ^ (col & 15) of halo pixel
(row 2mb + r, col = 2n + j).  A ds_read_b128 is served in four groups of 16 lanes, one LDS cycle each when the 16 lanes
touch 16 distinct 16-byte bank groups (64 banks x 4 B = 16 groups): asserted for every (mb, G, j, row)."""
import itertools

HALO_W, PIX_FLOATS = 34, 64
# ds_read_b128 lane groups of the CDNA4 LDS
GROUPS = [
    list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64)),
]


def read_byte_address(lane, mb, G, j, row):
    """as the kernel forms it: aoff[j] ^ (G << 4) floats, plus the row"""
    n, q = lane & 15, lane >> 4
    col = 2 * n + j
    aoff = 2 * mb * HALO_W * PIX_FLOATS + col * PIX_FLOATS + ((q ^ (col & 15)) << 2)
    return 4 * ((aoff ^ (G << 4)) + row * HALO_W * PIX_FLOATS)


def commit_byte_address(r, col, c4):
    """where commit() puts the 16-byte channel piece c4 of halo pixel (r, col)"""
    return 4 * (r * HALO_W * PIX_FLOATS + col * PIX_FLOATS + ((c4 ^ (col & 15)) << 2))


def test_lane_groups_cover_the_wave():
    assert sorted(itertools.chain(*GROUPS)) == list(range(64))


def test_a_fragment_reads_are_conflict_free():
    for mb, G, j, row in itertools.product(range(2), range(4), range(4), range(4)):
        for grp in GROUPS:
            bank_groups = {(read_byte_address(l, mb, G, j, row) // 16) % 16 for l in grp}
            assert len(bank_groups) == 16, (mb, G, j, row, grp)


def test_a_fragment_reads_hit_the_committed_pieces():
    """the read of lane (n, q) is piece 4G + q of pixel (2mb + row, 2n + j), inside the 6 x 34 halo image"""
    for mb, G, j, row, lane in itertools.product(range(2), range(4), range(4), range(4), range(64)):
        n, q = lane & 15, lane >> 4
        a = read_byte_address(lane, mb, G, j, row)
        assert a == commit_byte_address(2 * mb + row, 2 * n + j, 4 * G + q)
        assert 0 <= a and a + 16 <= 6 * HALO_W * PIX_FLOATS * 4
