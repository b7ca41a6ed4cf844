"""CPU check of the packed conv1 row sweep (csrc/conv_rows.hip: c1_afrag, c1_k4row, c1_k4word,
c1_bfrag; conv1_rows_pool_kernel and the conv1 part of enc2_rows_kernel).

Conv2D(16, 5, relu, same) + MaxPooling2D(2) on one-channel 128-wide images
(VAE/manual_scan_3layers.py:187-188). Lane m of wave w owns pooled pixel p = 16 w + m. Its two
output columns 2p, 2p + 1 read the six-column window from column 2p - 2; the column parity cb
is put into the weights, so 5 kernel rows x 6 window columns fill 30 of the 32 K slots of one
v_mfma_f32_16x16x32 and one B fragment serves both parities:

    lane group g, slot j < 6          kernel row g, window column j
    lane group g < 3, slot j = 6, 7   kernel row 4, window column 2g + j - 6
    lane group 3, slot j = 6, 7       weight zero, the lane reads a word that is always zero

Here the staged rows are built as the kernel's 32-bit words (two 16-bit elements as loaded,
fp16 or bf16 bit patterns), every lane gathers its four words by the kernel's formulas, the
MFMA is evaluated by its lane layout (A[i][k] in lane i + 16 (k / 8), B[k][n] in lane
n + 16 (k / 8), D[i][n] in lane n + 16 (i / 4), register i % 4) and the pooled result is
compared with a direct convolution. The LDS reads are then checked against the bank model of
tools/lds_banks.py at every ring position of both kernels.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from lds_banks import conflicts  # noqa: E402

C1W = 128    # image width
C1ROW = 80   # words per staged row (elements x = -8 .. W + 5 in words 0 .. 70)
C1ZW = 72    # a word of the row's tail pad: never written
K = 5


# ---- 16-bit formats as bit patterns (the kernel moves words, not values)
def to_bits(v, fmt):
    v = np.asarray(v, dtype=np.float64)
    if fmt == "f16":
        h = v.astype(np.float16)
        assert np.array_equal(h.astype(np.float64), v), "test values must be exact in fp16"
        return h.view(np.uint16)
    f = v.astype(np.float32)
    b = (f.view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(from_bits(b, fmt), v), "test values must be exact in bf16"
    return b


def from_bits(b, fmt):
    b = np.asarray(b, dtype=np.uint16)
    if fmt == "f16":
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ---- the kernel's formulas
def k4row(w, g):
    return 4 if g < 3 else 3 + (w & 1)


def k4word(p, g):
    return p + 3 + g if g < 3 else C1ZW


def afrag(wgt, m, g, cb):
    """A fragment (8 values) of column parity cb for lane (channel m, lane group g)."""
    out = np.zeros(8)
    for j in range(8):
        ky = g if j < 6 else 4
        c = (j if j < 6 else 2 * g + j - 6) - cb
        if (j < 6 or g < 3) and 0 <= c <= 4:
            out[j] = wgt[m, ky, c]
    return out


def stage_rows(img, fmt):
    """The workgroup's row stream of one image as staged words: position r + 2 holds row r
    (two zero rows above and below), element x at half (x + 8) of the row's 80 words."""
    H = img.shape[0]
    halves = np.zeros((H + 4, 2 * C1ROW), dtype=np.uint16)
    halves[2:H + 2, 8:8 + C1W] = to_bits(img, fmt)
    return (halves[:, 0::2].astype(np.uint32) | (halves[:, 1::2].astype(np.uint32) << 16))


def bfrag_words(rows, pos, w, lane):
    """The four words lane reads for the output row whose input rows are at pos .. pos + 4."""
    m, g = lane & 15, lane >> 4
    p = 16 * w + m
    run = rows[pos + g, p + 3:p + 6]
    return np.array([run[0], run[1], run[2], rows[pos + k4row(w, g), k4word(p, g)]], dtype=np.uint32)


def unpack(words, fmt):
    h = np.empty(8, dtype=np.uint16)
    h[0::2] = words & 0xFFFF  # slot 2i: low half, slot 2i + 1: high half
    h[1::2] = words >> 16
    return from_bits(h, fmt)


def mfma(a, b, acc):
    """v_mfma_f32_16x16x32 by lane layout: a, b [64][8] fragments, acc [64][4]."""
    A = np.zeros((16, 32))
    B = np.zeros((32, 16))
    for lane in range(64):
        A[lane & 15, 8 * (lane >> 4):8 * (lane >> 4) + 8] = a[lane]
        B[8 * (lane >> 4):8 * (lane >> 4) + 8, lane & 15] = b[lane]
    D = A @ B
    out = acc.copy()
    for lane in range(64):
        for j in range(4):
            out[lane, j] += D[4 * (lane >> 4) + j, lane & 15]
    return out


def packed_conv1_pool(img, wgt, bias, fmt):
    """The row sweep on one image [H][128] -> pooled [H/2][64][16]."""
    H = img.shape[0]
    rows = stage_rows(img, fmt)
    out = np.full((H // 2, C1W // 2, 16), np.nan)
    A = [np.array([afrag(wgt, lane & 15, lane >> 4, cb) for lane in range(64)]) for cb in range(2)]
    bias_l = np.array([[bias[4 * (lane >> 4) + i] for i in range(4)] for lane in range(64)])
    for pr in range(H // 2):          # step: pooled row pr, input row 2 pr - 2 at position 2 pr
        for w in range(4):
            acc = []
            for dy in range(2):
                B = np.array([unpack(bfrag_words(rows, 2 * pr + dy, w, lane), fmt)
                              for lane in range(64)])
                for cb in range(2):
                    acc.append(mfma(A[cb], B, bias_l))
            v = np.maximum(np.max(np.array(acc), axis=0), 0.0)
            for lane in range(64):
                out[pr, 16 * w + (lane & 15), 4 * (lane >> 4):4 * (lane >> 4) + 4] = v[lane]
    return out


def direct_conv1_pool(img, wgt, bias):
    H = img.shape[0]
    pad = np.zeros((H + 4, C1W + 4))
    pad[2:-2, 2:-2] = img
    conv = np.zeros((H, C1W, 16))
    for ky in range(K):
        for kx in range(K):
            conv += pad[ky:ky + H, kx:kx + C1W, None] * wgt[None, None, :, ky, kx]
    conv = np.maximum(conv + bias, 0.0)
    return conv.reshape(H // 2, 2, C1W // 2, 2, 16).max(axis=(1, 3))


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_packed_conv1_matches_direct(fmt):
    """6 x 128 image: pooled rows 0 and 2 touch the zero rows above and below, pixels p = 0 and
    p = 63 the left and right halo. Values are small multiples of 1/8: exact in both formats,
    every product and sum exact in float64."""
    rng = np.random.default_rng(5)
    img = rng.integers(-15, 16, (6, C1W)) / 8.0
    wgt = rng.integers(-15, 16, (16, K, K)) / 8.0
    bias = rng.integers(-7, 8, 16) / 4.0
    wq = from_bits(to_bits(wgt, fmt), fmt)
    got = packed_conv1_pool(img, wq, bias, fmt)
    ref = direct_conv1_pool(img, wgt, bias)
    assert not np.isnan(got).any()
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-12)
    for pr in (0, 2):
        for p in (0, 63):
            assert np.abs(ref[pr, p]).max() > 0  # the edge cells are not trivially zero


def test_every_tap_has_one_slot():
    """Each of the 25 taps sits in exactly one K slot of A[cb], at the slot whose B element is
    input (row ky, window column kx + cb); every other slot is zero."""
    wgt = np.arange(1, 26, dtype=np.float64).reshape(1, K, K).repeat(16, axis=0)
    for cb in range(2):
        seen = {}
        for g in range(4):
            a = afrag(wgt, 3, g, cb)
            for j in range(8):
                if a[j] == 0:
                    continue
                ky, col = (g, j) if j < 6 else (4, 2 * g + j - 6)
                assert a[j] == wgt[3, ky, col - cb]
                assert (ky, col - cb) not in seen
                seen[(ky, col - cb)] = (g, j)
        assert len(seen) == 25


def test_fragment_words_stay_inside_the_row():
    for w in range(4):
        for lane in range(64):
            m, g = lane & 15, lane >> 4
            p = 16 * w + m
            assert 3 <= p + 3 and p + 5 <= 70
            assert k4word(p, g) <= 70 or (g == 3 and 71 <= k4word(p, g) < C1ROW)
            assert 3 <= k4row(w, g) <= 4
    # the DMA writes words 4 .. 67 only (x = 0 .. W - 1): the zero word is never written
    assert C1ZW > 67 and C1ZW < C1ROW


@pytest.mark.parametrize("ring_rows", [16, 32])  # conv1_rows_pool_kernel, enc2_rows_kernel
def test_row_stride_is_conflict_free(ring_rows):
    """All four ds_read_b32 of a B fragment at every ring position, every pixel block: no extra
    LDS cycle under tools/lds_banks.py (ring bases are multiples of 128 bytes)."""
    for pos in range(32):
        for w in range(4):
            for k in range(4):
                addrs = []
                for lane in range(64):
                    m, g = lane & 15, lane >> 4
                    p = 16 * w + m
                    if k < 3:
                        row, word = (pos + g) % ring_rows, p + 3 + k
                    else:
                        row, word = (pos + k4row(w, g)) % ring_rows, k4word(p, g)
                    addrs.append(4 * (row * C1ROW + word))
                extra, cycles = conflicts("ds_read_b32", addrs)
                assert extra == 0, (pos, w, k, extra)
                assert cycles == 2
