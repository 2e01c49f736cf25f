"""CPU twin of `flaxdiff_amd/ops/hip/lds_swizzle.h`.

The hand GEMM and the halo conv keep unpadded `[row][64]` bf16 LDS images
(128-byte rows) filled lane-linearly by `global_load_lds`, with the 16-byte
chunk XOR-swizzled on the DMA's source address and on the `ds_read_b128`
offset. This file rebuilds the header's model and address formulas in Python
and checks two things:

* cycles: under the `ds_read_b128` lane-group model (four 16-lane groups
  {0-3,12-15,20-27}, {4-11,16-19,28-31} and the same two plus 32; a group takes
  as many cycles as the largest number of distinct addresses on one 16-byte
  slot of the 256-byte bank row) the old key `row & 7` costs 8 cycles per
  fragment read (16 for the W=8 halo) and the new key `(krow >> 1) & 7`
  costs the minimum of 4 — so the model sees the defect the key removes;
* round trip: the image the DMA formula writes, read back with the reader
  formula at (row, k-chunk), yields logical chunk k for every row.
"""
import itertools

import pytest

ROW_BYTES = 128
GROUP0 = [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27]
GROUP1 = [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]
GROUPS = [GROUP0, GROUP1, [l + 32 for l in GROUP0], [l + 32 for l in GROUP1]]


def b128_cycles(addrs):
    """LDS-array cycles of one wave `ds_read_b128` from 64 byte addresses."""
    assert len(addrs) == 64
    total = 0
    for grp in GROUPS:
        per_slot = {}
        for l in grp:
            per_slot.setdefault((addrs[l] >> 4) & 15, set()).add(addrs[l])
        total += max(len(s) for s in per_slot.values())
    return total


def key_new(krow):
    return (krow >> 1) & 7


def key_old(krow):
    return krow & 7


def key_pitch(W):
    """Pitch of the halo KEY row; the physical pitch stays W + 2."""
    return {8: 24, 16: 32}.get(W, W + 2)


def halo_key_row(W, slot, pos):
    return slot * key_pitch(W) + pos


def halo_phys_row(W, slot, pos):
    return slot * (W + 2) + pos


def frag_addrs(base_row, rows, krows, kk, key):
    """Byte addresses of one fragment read: lane (half, l31) reads row
    rows[l31], logical chunk 2*kk + half."""
    out = []
    for lane in range(64):
        half, l31 = lane >> 5, lane & 31
        ch = (2 * kk + half) ^ key(krows[l31])
        out.append((base_row + rows[l31]) * ROW_BYTES + ch * 16)
    return out


def halo_geom(BMT, W):
    nslot = BMT // W + 2
    nrow_h = nslot * (W + 2)
    return nslot, nrow_h, nrow_h + 3       # NSLOT, ZR, WB0


TILES = [(256, 64), (128, 128)]            # (BMT, BNT)


# ---- cycles ---------------------------------------------------------------

def weight_reads(BMT, BNT, W):
    """(absolute base row, relative rows) of every halo weight fragment."""
    _, _, wb0 = halo_geom(BMT, W)
    for buf, wn, fn in itertools.product(range(3), range(BNT // 64), range(2)):
        rel = [wn * 64 + fn * 32 + l for l in range(32)]
        yield wb0 + buf * BNT, rel


@pytest.mark.parametrize("W", [8, 16, 32, 64])
@pytest.mark.parametrize("BMT,BNT", TILES)
def test_halo_weight_read_cycles(BMT, BNT, W):
    for base, rel in weight_reads(BMT, BNT, W):
        for kk in range(4):
            assert b128_cycles(frag_addrs(base, rel, rel, kk, key_old)) == 8
            assert b128_cycles(frag_addrs(base, rel, rel, kk, key_new)) == 4


def halo_b_rows(BMT, W, wm, fm, dr, ds):
    """Physical and key rows of an interior B fragment (no zero-row lane)."""
    phys, krow = [], []
    for l31 in range(32):
        m = wm * 64 + fm * 32 + l31
        slot = m // W + dr + 1
        pos = m % W + 1 + ds
        phys.append(halo_phys_row(W, slot, pos))
        krow.append(halo_key_row(W, slot, pos))
    return phys, krow


@pytest.mark.parametrize("W", [8, 16, 32, 64])
@pytest.mark.parametrize("BMT,BNT", TILES)
def test_halo_b_read_cycles(BMT, BNT, W):
    old_expected = 16 if W == 8 else 8
    for wm, fm, dr, ds in itertools.product(
            range(BMT // 64), range(2), (-1, 0, 1), (-1, 0, 1)):
        phys, krow = halo_b_rows(BMT, W, wm, fm, dr, ds)
        for kk in range(4):
            assert b128_cycles(frag_addrs(0, phys, phys, kk, key_old)) \
                == old_expected
            assert b128_cycles(frag_addrs(0, phys, krow, kk, key_new)) == 4


def test_halo_b_narrow_needs_key_pitch():
    """The physical row as key row is not enough on the narrow widths."""
    worst = {}
    for W in (8, 16):
        worst[W] = max(
            b128_cycles(frag_addrs(0, phys, phys, kk, key_new))
            for wm, fm, dr, ds, kk in itertools.product(
                range(4), range(2), (-1, 0, 1), (-1, 0, 1), range(4))
            for phys, _ in [halo_b_rows(256, W, wm, fm, dr, ds)])
    assert worst == {8: 12, 16: 8}


@pytest.mark.parametrize("W", [8, 16])
def test_halo_b_zero_row_redirect_bound(W):
    """Image rows of a fragment redirected to the zero row (sample borders
    inside a fragment on the narrow widths) may conflict, never above 8."""
    _, zr, _ = halo_geom(256, W)
    rpf = 32 // W                       # image rows per fragment
    worst = 0
    for mask in range(1, 1 << rpf):
        for fm, dr, ds, kk in itertools.product(
                range(2), (-1, 0, 1), (-1, 0, 1), range(4)):
            phys, krow = halo_b_rows(256, W, 0, fm, dr, ds)
            for l31 in range(32):
                if mask >> (l31 // W) & 1:
                    # the kernel keeps the lane's key delta (14 * slot)
                    kd = krow[l31] - phys[l31]
                    phys[l31] = zr + 1 + ds
                    krow[l31] = phys[l31] + kd
            c = b128_cycles(frag_addrs(0, phys, krow, kk, key_new))
            assert 4 <= c <= 8
            worst = max(worst, c)
    assert worst <= 8


@pytest.mark.parametrize("BMT,BNT", TILES)
def test_gemm_read_cycles(BMT, BNT):
    xtile_rows, wtile_rows = BMT, BNT
    for buf in range(2):
        for wn, fn in itertools.product(range(BNT // 64), range(2)):
            rel = [wn * 64 + fn * 32 + l for l in range(32)]
            base = 2 * xtile_rows + buf * wtile_rows
            for kk in range(4):
                assert b128_cycles(frag_addrs(base, rel, rel, kk, key_old)) == 8
                assert b128_cycles(frag_addrs(base, rel, rel, kk, key_new)) == 4
        for wm, fm in itertools.product(range(BMT // 64), range(2)):
            rel = [wm * 64 + fm * 32 + l for l in range(32)]
            base = buf * xtile_rows
            for kk in range(4):
                assert b128_cycles(frag_addrs(base, rel, rel, kk, key_old)) == 8
                assert b128_cycles(frag_addrs(base, rel, rel, kk, key_new)) == 4


# ---- round trip -----------------------------------------------------------

def dma_piece(image, row0, krow0):
    """One `global_load_lds` piece: lane l lands at (row0 + l/8, chunk l&7)
    and fetched source chunk (l & 7) ^ key(krow0 + l/8) of that row."""
    for lane in range(64):
        r8, c = lane >> 3, lane & 7
        image[(row0 + r8, c)] = (row0 + r8, c ^ key_new(krow0 + r8))


def read_chunk(image, row, krow, k):
    return image[(row, k ^ key_new(krow))]


@pytest.mark.parametrize("W", [8, 16, 32, 64])
@pytest.mark.parametrize("BMT", [128, 256])
def test_round_trip_halo(BMT, W):
    nslot, _, _ = halo_geom(BMT, W)
    image = {}
    for q in range(nslot * W // 8):
        slot, c = divmod(q, W // 8)
        pos0 = 1 + c * 8
        dma_piece(image, halo_phys_row(W, slot, pos0),
                  halo_key_row(W, slot, pos0))
    assert len(image) == nslot * W * 8
    for slot, pix, k in itertools.product(range(nslot), range(W), range(8)):
        row = halo_phys_row(W, slot, pix + 1)
        got = read_chunk(image, row, halo_key_row(W, slot, pix + 1), k)
        assert got == (row, k)
    # the reader's form: key row = physical row + (key pitch - pitch) * slot
    for slot, pix in itertools.product(range(nslot), range(W)):
        row = halo_phys_row(W, slot, pix + 1)
        assert halo_key_row(W, slot, pix + 1) \
            == row + (key_pitch(W) - (W + 2)) * slot


@pytest.mark.parametrize("rows", [64, 128, 256])
def test_round_trip_row_tiles(rows):
    """Weight ring buffers and both GEMM tiles: key row = row in the tile."""
    image = {}
    for p in range(rows // 8):
        dma_piece(image, p * 8, p * 8)
    for row, k in itertools.product(range(rows), range(8)):
        assert read_chunk(image, row, row, k) == (row, k)
