"""A plain numpy restatement of the bilateral label filter that specenh.filters.bilateral runs
(include/specenh_bilateral.h), shared by the CPU and GPU tests.

``cv2.bilateralFilter(u8, d, sigmaColor, sigmaSpace)`` on one 8-bit channel with
BORDER_DEFAULT (OpenCV is absent, so its algorithm is restated):

    sigma <= 0 becomes 1;  radius = d <= 0 ? cvRound(1.5 sigmaSpace) : d // 2, at least 1
    taps (i, j), row-major, over the disc i^2 + j^2 <= radius^2, the centre included
    sw[k] = float32(exp(-0.5 (i^2 + j^2) / sigmaSpace^2))
    cw[t] = float32(exp(-0.5 t^2 / sigmaColor^2)),  t = |v - v0| = 0 .. 255
    q     = sum_k v_k sw[k] cw[|v_k - v0|] / sum_k sw[k] cw[|v_k - v0|]   (BORDER_REFLECT_101)
    out   = cvRound(q)                                  (half to even, like numpy.rint)

cv2 accumulates q in float32 in an order that depends on its SIMD build, so its bytes are not
reproducible; the truth here is ``quotient64``: the float32 tables, products and sums in
float64. Every float32 evaluation (one product per weight, one chain per sum, one division)
stays within ``delta(n) = 255 (2 n + 3) 2^-24`` of it, n the tap count, so the criterion for
an 8-bit result is ``|out - q64| <= 0.5 + delta(n)`` at every pixel.
"""
import numpy as np

from oracle import filters as of

MAX_RADIUS = 15


def radius_of(d, sigma_space):
    if sigma_space <= 0:
        sigma_space = 1.0
    r = int(np.rint(1.5 * sigma_space)) if d <= 0 else d // 2
    return max(r, 1)


def offsets(radius):
    """The taps (i, j) in accumulation order, int arrays."""
    ij = [(i, j) for i in range(-radius, radius + 1) for j in range(-radius, radius + 1)
          if i * i + j * j <= radius * radius]
    a = np.asarray(ij, dtype=np.int64)
    return a[:, 0], a[:, 1]


def taps(d, sigma_space):
    """(radius, tap count)."""
    r = radius_of(d, sigma_space)
    return r, int(offsets(r)[0].size)


def tables(d, sigma_color, sigma_space):
    """(i, j, sw float32 [n], cw float32 [256]): exp in float64, rounded once."""
    if sigma_color <= 0:
        sigma_color = 1.0
    if sigma_space <= 0:
        sigma_space = 1.0
    i, j = offsets(radius_of(d, sigma_space))
    sw = np.exp(-0.5 * (i * i + j * j).astype(np.float64) / (sigma_space * sigma_space))
    t = np.arange(256, dtype=np.float64)
    cw = np.exp(-0.5 * t * t / (sigma_color * sigma_color))
    return i, j, sw.astype(np.float32), cw.astype(np.float32)


def _gather(u8, i, j):
    """v[k, r, c] = u8 at (r + i_k, c + j_k) under BORDER_REFLECT_101, int64."""
    rows, cols = u8.shape
    ri = of._reflect101(np.arange(rows)[None, :] + i[:, None], rows)    # [n, rows]
    ci = of._reflect101(np.arange(cols)[None, :] + j[:, None], cols)    # [n, cols]
    return u8.astype(np.int64)[ri[:, :, None], ci[:, None, :]]


def quotient64(u8, d=15, sigma_color=75.0, sigma_space=75.0):
    """q64 [rows, cols] float64: the float32 tables, products and sums in float64."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 2
    i, j, sw, cw = tables(d, sigma_color, sigma_space)
    v = _gather(u8, i, j)
    w = sw.astype(np.float64)[:, None, None] * cw.astype(np.float64)[np.abs(v - u8.astype(np.int64))]
    return (v * w).sum(axis=0) / w.sum(axis=0)


def quotient32(u8, d=15, sigma_color=75.0, sigma_space=75.0):
    """The float32 evaluation the kernel makes: w = sw * cw rounded, both sums one float32
    chain in tap order (the product v * w rounded on its own here, fused in the kernel)."""
    u8 = np.asarray(u8)
    i, j, sw, cw = tables(d, sigma_color, sigma_space)
    v = _gather(u8, i, j)
    sv = np.zeros(u8.shape, np.float32)
    sw_sum = np.zeros(u8.shape, np.float32)
    c = u8.astype(np.int64)
    for k in range(i.size):
        w = sw[k] * cw[np.abs(v[k] - c)]
        assert w.dtype == np.float32
        sw_sum = sw_sum + w
        sv = sv + v[k].astype(np.float32) * w
    return sv / sw_sum


def delta(n):
    """Worst-case distance of the float32 quotient from q64 for n taps."""
    return 255.0 * (2 * n + 3) * 2.0 ** -24


def bilateral_u8(u8, d=15, sigma_color=75.0, sigma_space=75.0):
    return np.rint(quotient64(u8, d, sigma_color, sigma_space)).astype(np.uint8)


def bilateral(src, d=15, sigma_color=75.0, sigma_space=75.0):
    """dataset.ipynb's bilateral(src) with numpy's rescale of a uint8 array."""
    return of.rescale_u8(bilateral_u8(of.to_u8(np.asarray(src)), d, sigma_color, sigma_space))


def check(out_u8, u8, d, sigma_color, sigma_space):
    """(worst |out - q64| - 0.5, bound delta(n)) of an 8-bit result; the criterion is
    worst <= bound."""
    q = quotient64(u8, d, sigma_color, sigma_space)
    n = taps(d, sigma_space)[1]
    return float(np.abs(np.asarray(out_u8).astype(np.float64) - q).max() - 0.5), delta(n)


def noise_image(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


def smooth_image(rows, cols, seed):
    """A double cumulative sum of noise, rescaled to 0 .. 255: neighbours a few levels apart,
    which is where the colour weight varies."""
    g = np.random.default_rng(seed).standard_normal((rows, cols))
    s = np.cumsum(np.cumsum(g, axis=0), axis=1)
    if s.max() == s.min():
        return np.zeros((rows, cols), np.uint8)
    return np.rint((s - s.min()) / (s.max() - s.min()) * 255).astype(np.uint8)
