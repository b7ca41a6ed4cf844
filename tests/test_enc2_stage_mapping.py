"""CPU check of the fused encoder's schedule 1 (csrc/conv_rows.hip, enc2_rows_kernel<T, 4, 1>).

A step's pooled row (32 pixels x 32 channels of 16 bits) is 2 KB, contiguous in the NHWC
output. Wave (wx, nb), lane (m = lane & 15, kg = lane >> 4) holds the four channels
16 nb + 4 kg .. + 3 of pixel (16 wx + m) / 2 in 8 bytes (lanes m, m ^ 1 the same ones) and
writes them into an LDS tile; after the barrier store wave k (waves 6 and 7), lane l reads 16
bytes and stores them at byte 1024 k + 16 l of the row. The index maps are restated here
(e2_tile_write, e2_tile_read) and checked: both cover the tile exactly once, the read-back
reproduces NHWC, and both are free of LDS bank conflicts under tools/lds_banks.py's model.

The step bookkeeping is restated too: the flag word (three bits per position of the step
stream, shifted once per step) against the predicates schedule 0 evaluates from its (image,
row) counters, and the scalar pointer walks (pooled-row base, DMA source row) against the
multiply forms, for every step of 1 .. 5 images per workgroup at H = 4 .. 32.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from lds_banks import conflicts  # noqa: E402

TILE = 32 * 32 * 2


def tile_write(p, c8):
    """e2_tile_write: 8-byte chunk c8 = 4 nb + kg of pixel p."""
    return 64 * p + 8 * (c8 ^ (2 * ((p >> 1) & 3)))


def tile_read(k, lane):
    """e2_tile_read: where the 16 bytes of row byte 1024 k + 16 lane sit."""
    p = 16 * k + (lane >> 2)
    return 64 * p + 16 * ((lane & 3) ^ ((p >> 1) & 3))


def lane_write(wv, lane):
    wx, nb, m, kg = wv % 4, wv // 4, lane & 15, lane >> 4
    return tile_write((16 * wx + m) >> 1, 4 * nb + kg), (16 * wx + m) >> 1, 16 * nb + 4 * kg


def written_tile():
    """tile[byte] = the NHWC byte (of the row's 2 KB) that the write map put there, -1: none."""
    tile = np.full(TILE, -1, dtype=np.int64)
    for wv in range(8):
        for lane in range(64):
            a, p, ch = lane_write(wv, lane)
            assert a % 8 == 0 and 0 <= a <= TILE - 8
            want = (p * 32 + ch) * 2 + np.arange(8)
            # lanes m and m ^ 1 write the same piece to the same place; nobody else does
            assert (tile[a:a + 8] == -1).all() or ((lane & 1) and (tile[a:a + 8] == want).all())
            tile[a:a + 8] = want
    return tile


def test_write_map_covers_tile_once():
    tile = written_tile()
    assert (tile >= 0).all()
    assert np.array_equal(np.sort(tile), np.arange(TILE))


def test_read_back_covers_tile_once_and_is_nhwc():
    tile = written_tile()
    seen = np.zeros(TILE, dtype=np.int64)
    out = np.full(TILE, -1, dtype=np.int64)
    for k in range(2):
        for lane in range(64):
            a = tile_read(k, lane)
            assert a % 16 == 0 and 0 <= a <= TILE - 16
            seen[a:a + 16] += 1
            g = 1024 * k + 16 * lane  # the store's byte offset in the row
            out[g:g + 16] = tile[a:a + 16]
    assert (seen == 1).all()
    assert np.array_equal(out, np.arange(TILE))


def test_tile_accesses_bank_conflict_free():
    for wv in range(8):
        assert conflicts("ds_write_b64", [lane_write(wv, l)[0] for l in range(64)])[0] == 0
    for k in range(2):
        assert conflicts("ds_read_b128", [tile_read(k, l) for l in range(64)])[0] == 0
    # the plain layout the swizzle replaces: a 64-byte pixel pitch puts four of a lane group's
    # eight pixels on the same banks
    plain = [64 * ((l & 15) >> 1) + 8 * (l >> 4) for l in range(64)]
    assert conflicts("ds_write_b64", plain)[0] == 4 * 3


# ---------------------------------------------------------------- step bookkeeping
REAL, BUB, TOP = 1, 2, 4
F_PROD, F_CBUB, F_CTOP = REAL, BUB << 6, TOP << 6
F_OUT, F_OTOP, F_HELD = REAL << 12, TOP << 12, REAL << 15
ROWO, ROWX = 2048, 256


def fdiv(x, d):
    return x // d  # floor


@pytest.mark.parametrize("H1", range(4, 36, 4))
@pytest.mark.parametrize("nimg", range(1, 6))
def test_flag_word_and_pointer_walks(H1, nimg):
    H, G, b = H1 // 2, 7, 3  # conv2 input height; grid size and this workgroup's index
    SPI, PPI, PHh = H // 2 + 1, H1 + 4, H // 2
    S = nimg * SPI + 1
    OUT, X = 1 << 40, 1 << 41  # base addresses

    def bits(t):  # position t = il SPI + q of the step stream
        il, q = fdiv(t, SPI), t % SPI
        if t < 0:
            return 0
        return (REAL if il < nimg and q != PHh else 0) | (BUB if q == PHh else 0) | \
            (TOP if q == 0 else 0)

    # the kernel's set-up: positions 0 .. 2 pushed, ob at pair -2 of the virtual image before
    ilT = qT = 0
    fl = 0

    def push():
        nonlocal fl
        inn = qT < PHh
        fl = ((fl << 3) | ((ilT < nimg and inn) * REAL) | ((not inn) * BUB) | ((qT < 1) * TOP)) \
            & 0xFFFFFFFF

    def walk():
        nonlocal ilT, qT
        qT += 1
        if qT == SPI:
            qT, ilT = 0, ilT + 1

    push(); walk(); push(); walk(); push()
    ob = OUT + ((b - G) * PHh + SPI - 2) * ROWO
    obp = ob - ROWO
    ojump = (G - 1) * PHh * ROWO
    xjump = (G - 1) * H1 * ROWX
    dma = []
    for wv in range(4):
        ilD, rD = divmod(32 + wv, PPI)
        dma.append([ilD, rD, X + ((b + ilD * G) * H1 + rD - 2) * ROWX, wv if wv < 2 else H1 + wv])
    held = False
    for s in range(S + 1):  # (step S: only the tile store after the loop)
        # the word holds positions s + 2 .. s - 3
        for k in range(6):
            assert (fl >> (3 * k)) & 7 == bits(s + 2 - k), (s, k)
        # schedule 0's predicates, from its counters
        ilA, qA = fdiv(s - 2, SPI), (s - 2) % SPI
        ilB, qB = fdiv(s + 2, SPI), (s + 2) % SPI
        qC = s % SPI
        stored = 0 <= ilA < nimg and qA < PHh
        assert bool(fl & F_OUT) == stored
        assert bool(fl & F_HELD) == held
        if fl & F_HELD:  # the tile of pair s - 3 goes to obp
            il3, q3 = fdiv(s - 3, SPI), (s - 3) % SPI
            assert obp == OUT + ((b + il3 * G) * PHh + q3) * ROWO
        if s == S:
            break
        assert bool(fl & F_CTOP) == (qC == 0)
        assert bool(fl & F_CBUB) == (qC == SPI - 1)
        for jr in range(2):
            assert bool(fl & F_PROD) == (ilB < nimg and 2 * qB + jr < H)
        if stored:  # (the unstaged store's address)
            assert ob == OUT + ((b + ilA * G) * PHh + qA) * ROWO
        for wv in range(4):
            ilD, rD, xs, zr = dma[wv]
            pos = 4 * s + 32 + wv
            assert (ilD, rD) == divmod(pos, PPI)
            y = rD - 2
            real = ilD < nimg and 0 <= y < H1
            assert real == (ilD < nimg and rD != zr)
            if real:
                assert xs == X + ((b + ilD * G) * H1 + y) * ROWX
        # next(): step s + 1's
        held = stored
        walk()
        push()
        obp = ob
        ob += ojump if fl & F_OTOP else ROWO
        for d in dma:
            d[1] += 4
            if d[1] >= PPI:
                d[1] -= PPI
                d[0] += 1
                d[2] += xjump
            else:
                d[2] += 4 * ROWX
    # every output row of every image was stored exactly once is implied by the asserts above:
    # `stored` is schedule 0's own condition and obp the row's multiply-form address
