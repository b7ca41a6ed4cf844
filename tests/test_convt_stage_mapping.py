"""CPU check of convT1's staged output tile (csrc/conv_rows.hip, convt_rows_pw_kernel).

A step's two output rows (2 x 32 pixels x 64 channels of 16 bits) are 8 KB, contiguous in the
NHWC output. Wave nb, lane (m = lane & 15, kg = lane >> 4) holds, per phase (py, px), the four
channels 16 nb + 4 kg .. + 3 of pixel (py, 2 m + px) in 8 bytes and writes them into an LDS
tile; after the barrier wave w, lane l reads 16 bytes twice (j = 0, 1) and stores them at output
byte 2048 w + 1024 j + 16 l of the tile's 8 KB. The index maps are restated here (ct_tile_write,
ct_tile_read, the half swap) and checked: both cover the tile exactly once, the read-back
reproduces NHWC, both are free of LDS bank conflicts under tools/lds_banks.py's model, and the
unrolled loop's ring slots are the rolled loop's.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from lds_banks import conflicts  # noqa: E402

TILE = 2 * 32 * 64 * 2


def tile_write(nb, m, kg):
    """ct_tile_write: the lane's piece of phase (0, 0); phase (py, px) adds 4096 py + 128 px."""
    return 256 * m + 8 * ((4 * nb + kg) ^ m)


def tile_read(w, lane, j):
    """ct_tile_read: where the 16 bytes of tile byte L = 2048 w + 1024 j + 16 lane sit."""
    L = 2048 * w + 1024 * j + 16 * lane
    p = (L >> 7) & 31
    return (L & ~0x70) | (((lane & 7) ^ (p >> 2)) << 4)


def nhwc_byte(py, p, ch):
    return (py * 32 + p) * 128 + 2 * ch


def written_tile():
    """tile[byte] = the NHWC byte (of the 8 KB) that the write map put there, -1: none."""
    tile = np.full(TILE, -1, dtype=np.int64)
    for nb in range(4):
        for lane in range(64):
            m, kg = lane & 15, lane >> 4
            for ph in range(4):
                py, px = ph >> 1, ph & 1
                a = tile_write(nb, m, kg) + 4096 * py + 128 * px
                assert a % 8 == 0 and 0 <= a <= TILE - 8
                assert (tile[a:a + 8] == -1).all(), "piece written twice"
                tile[a:a + 8] = nhwc_byte(py, 2 * m + px, 16 * nb + 4 * kg) + np.arange(8)
    return tile


def test_write_map_covers_tile_once():
    tile = written_tile()
    assert (tile >= 0).all()
    assert np.array_equal(np.sort(tile), np.arange(TILE))


def test_read_back_covers_tile_once_and_is_nhwc():
    tile = written_tile()
    seen = np.zeros(TILE, dtype=np.int64)
    out = np.full(TILE, -1, dtype=np.int64)
    for w in range(4):
        for lane in range(64):
            swap = (lane >> 4) & 1
            for j in range(2):
                a = tile_read(w, lane, j)
                assert a % 16 == 0 and 0 <= a <= TILE - 16
                seen[a:a + 16] += 1
                v = tile[a:a + 16]
                if swap:
                    v = np.concatenate([v[8:], v[:8]])
                g = 2048 * w + 1024 * j + 16 * lane  # the store's byte offset in the 8 KB
                out[g:g + 16] = v
    assert (seen == 1).all()
    # global byte g of the tile's 8 KB holds NHWC byte g: rows 2s and 2s + 1, all 32 pixels
    assert np.array_equal(out, np.arange(TILE))


def test_tile_accesses_bank_conflict_free():
    for nb in range(4):
        for ph in range(4):
            addrs = [tile_write(nb, l & 15, l >> 4) + 4096 * (ph >> 1) + 128 * (ph & 1)
                     for l in range(64)]
            assert conflicts("ds_write_b64", addrs)[0] == 0
        for j in range(2):
            addrs = [tile_read(nb, l, j) for l in range(64)]
            assert conflicts("ds_read_b128", addrs)[0] == 0
    # the plain layout the swizzle replaces: a 128-byte pixel pitch puts the 16 positions of a
    # ds_write_b64 lane group on the same banks
    plain = [256 * (l & 15) + 8 * (l >> 4) for l in range(64)]
    assert conflicts("ds_write_b64", plain)[0] == 4 * 15


def test_unrolled_slots():
    """Step g = 8 k + I reads ring slots (I + 1 + dy) & 7, refills slot (I + 6) & 7 (position
    g + 3 + LEAD, LEAD = 3), writes tile buffer I & 1 and stores buffer (I + 1) & 1; the held
    tile after a loop of S steps is buffer (S - 1) & 1."""
    LEAD = 3
    for g in range(64):
        I = g & 7
        for dy in (-1, 0, 1):
            assert (I + 1 + dy) & 7 == (g + 1 + dy) & 7
        assert (I + 3 + LEAD) & 7 == (g + 3 + LEAD) & 7
        assert I & 1 == g & 1 and (I + 1) & 1 == (g - 1) & 1
        # the slot refilled in step g is none of those read in steps g .. g + 1 (a wave may
        # run one barrier ahead of the refill's landing check)
        assert (g + 3 + LEAD) & 7 not in {(h + 1 + dy) & 7 for h in (g, g + 1) for dy in (-1, 0, 1)}
