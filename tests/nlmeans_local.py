"""A plain numpy restatement of the non-local means denoiser that specenh.filters.nl_means runs
(include/specenh_nlmeans.h), shared by the CPU and GPU tests. scikit-image is absent, so the
formula is restated, with its ``fast_mode=True`` weighting and without its cutoff at a > 5:

    u~      = the image extended by np.pad(mode="reflect"),  f = P // 2
    d2(x,t) = (1/P^2) sum_{o in [-f,f]^2} (u~(x+o) - u~(x+t+o))^2
    a(x,t)  = max(d2(x,t) - 2 sigma^2, 0) / h^2,   w = exp(-a),   t in [-D, D]^2 row-major
    q(x)    = sum_t w(x,t) u~(x+t) / sum_t w(x,t)

``quotient64`` evaluates it in float64 on the float32 image. The kernel evaluates it in float32;
per pixel its result must lie within ``bound``:

    eta_t = w_t (c_d eps (a_t + k) + c_e eps) + 2^-126,   k = 2 sigma^2 / h^2,  eps = 2^-24
    B(x)  = sum_t eta_t |v_t - q| / (W - sum_t eta_t) + (2 n + 3) eps max_t |v_t|

with c_d = P^2 + 8 roundings on the way to a (the difference, the square, P^2 - 1 additions of
non-negative terms, the scale and its constant, 2 sigma^2 and its subtraction, the log2(e)
scaling), c_e = 4 for the device exp2, 2^-126 for weights that leave float32's normal range,
and the second term for the two float32 chains over the n shifts and the division. The
constants depend on P alone.
"""
import numpy as np

EPS = 2.0 ** -24
C_E = 4


def c_d(P):
    return P * P + 8


def terms(u32, P=7, D=11, h=0.1, sigma=0.0):
    """(a, v): float64 [n, ..., rows, cols], the scaled patch distance and the shifted pixel of
    every shift, for a float32 image [rows, cols] or a stack of images [..., rows, cols]."""
    u32 = np.asarray(u32)
    assert u32.dtype == np.float32 and u32.ndim >= 2
    assert P % 2 == 1 and P >= 1 and D >= 0 and h > 0 and sigma >= 0
    f = P // 2
    H = D + f
    rows, cols = u32.shape[-2:]
    lead = u32.shape[:-2]
    up = np.pad(u32.astype(np.float64), [(0, 0)] * len(lead) + [(H, H), (H, H)], mode="reflect")
    hr, hc = rows + 2 * f, cols + 2 * f          # the pixels under every patch of the image
    own = up[..., D:D + hr, D:D + hc]
    n = (2 * D + 1) ** 2
    a = np.empty((n,) + u32.shape)
    v = np.empty((n,) + u32.shape)
    k = 0
    for ti in range(-D, D + 1):
        for tj in range(-D, D + 1):
            sh = up[..., D + ti:D + ti + hr, D + tj:D + tj + hc]
            e = (own - sh) ** 2
            d2 = np.zeros(u32.shape)
            for oi in range(P):
                for oj in range(P):
                    d2 += e[..., oi:oi + rows, oj:oj + cols]
            d2 /= P * P
            a[k] = np.maximum(d2 - 2.0 * sigma * sigma, 0.0) / (h * h)
            v[k] = sh[..., f:f + rows, f:f + cols]
            k += 1
    return a, v


def quotient64_and_bound(u32, P=7, D=11, h=0.1, sigma=0.0):
    """(q, B): the float64 quotient and the per-pixel bound on a float32 evaluation."""
    a, v = terms(u32, P, D, h, sigma)
    n = a.shape[0]
    w = np.exp(-a)
    W = w.sum(axis=0)
    q = (w * v).sum(axis=0) / W
    eta = w * (c_d(P) * EPS * (a + 2.0 * sigma * sigma / (h * h)) + C_E * EPS) + 2.0 ** -126
    B = ((eta * np.abs(v - q)).sum(axis=0) / (W - eta.sum(axis=0))
         + (2 * n + 3) * EPS * np.abs(v).max(axis=0))
    return q, B


def quotient64(u32, P=7, D=11, h=0.1, sigma=0.0):
    return quotient64_and_bound(u32, P, D, h, sigma)[0]


def bound(u32, P=7, D=11, h=0.1, sigma=0.0):
    return quotient64_and_bound(u32, P, D, h, sigma)[1]


def _reflect(p, n):
    """Index of the reflection without edge repeat, applied as often as needed."""
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * n - 2 - p
    return p


def brute(u, P=7, D=11, h=0.1, sigma=0.0):
    """The formula literally, four loops, for images of a few pixels."""
    u = np.asarray(u, dtype=np.float64)
    rows, cols = u.shape
    f = P // 2
    out = np.empty((rows, cols))
    for r in range(rows):
        for c in range(cols):
            W = S = 0.0
            for ti in range(-D, D + 1):
                for tj in range(-D, D + 1):
                    d2 = 0.0
                    for oi in range(-f, f + 1):
                        for oj in range(-f, f + 1):
                            x = u[_reflect(r + oi, rows), _reflect(c + oj, cols)]
                            y = u[_reflect(r + ti + oi, rows), _reflect(c + tj + oj, cols)]
                            d2 += (x - y) ** 2
                    w = np.exp(-max(d2 / (P * P) - 2.0 * sigma * sigma, 0.0) / (h * h))
                    W += w
                    S += w * u[_reflect(r + ti, rows), _reflect(c + tj, cols)]
            out[r, c] = S / W
    return out


# ---------------------------------------------------------------- images, float32 in [0, 1]
def noise_image(rows, cols, seed):
    return np.random.default_rng(seed).random((rows, cols), dtype=np.float32)


def smooth_image(rows, cols, seed):
    """A double cumulative sum of noise, rescaled: neighbouring patches a little apart, which
    is where the weights vary."""
    g = np.random.default_rng(seed).standard_normal((rows, cols))
    s = np.cumsum(np.cumsum(g, axis=0), axis=1)
    if s.max() == s.min():
        return np.full((rows, cols), 0.5, np.float32)
    return ((s - s.min()) / (s.max() - s.min())).astype(np.float32)


def clean_ridge(rows, cols):
    """A slanted ridge in [0, 1], like a mode on a spectrogram."""
    r = np.arange(rows)[:, None]
    c = np.arange(cols)[None, :]
    return np.exp(-0.5 * ((r - rows * (0.3 + 0.4 * c / max(cols, 1))) / 2.0) ** 2)


def ridge_image(rows, cols, seed):
    """The ridge on a background of uniform noise."""
    rng = np.random.default_rng(seed)
    return ((clean_ridge(rows, cols) + 0.3 * rng.random((rows, cols))) / 1.3).astype(np.float32)
