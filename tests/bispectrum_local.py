"""A plain numpy / scipy restatement of the bispectrum and squared bicoherence that
specenh.bispectrum computes (include/specenh_bispectrum.h), shared by the CPU and GPU tests.

X_t[k] is column t of scipy.signal.spectrogram(s, ..., mode='complex') on each group's slice
(the slices of tests/test_spectral_gpu.py); for k + l <= N/2

    B[k, l]  = mean_t X_t[k] Y_t[l] conj(Z_t[k + l])
    D[k, l]  = mean_t |X_t[k] Y_t[l]|^2,   E[m] = mean_t |Z_t[m]|^2
    b2[k, l] = |B[k, l]|^2 / (D[k, l] E[k + l])

and 0 in both outside. The sums run frame by frame, so only [B, K, K] temporaries exist, and
in a chosen dtype: the float32 run is complex64 / float32 throughout (asserted), which gives
the reference's own rounding error that the GPU bound is taken from.
"""
import numpy as np
import scipy.signal


def group_slices(length, nperseg, noverlap, navg):
    """The sample slice of every averaging group (navg <= 0: one group of all frames)."""
    hop = nperseg - noverlap
    T = (length - nperseg) // hop + 1
    glen = navg if navg >= 1 else T
    return [slice(g * glen * hop, g * glen * hop + (glen - 1) * hop + nperseg)
            for g in range(T // glen)]


def accumulate(X, Y, Z, rows, cols):
    """B, b2 [batch, len(rows), len(cols)] from spectra [batch, F, T] of one group, in the
    spectra's precision."""
    cdt = X.dtype
    rdt = np.float32 if cdt == np.complex64 else np.float64
    assert cdt in (np.complex64, np.complex128) and Y.dtype == cdt and Z.dtype == cdt
    nb, F, T = X.shape
    m = rows[:, None] + cols[None, :]
    inside = m <= F - 1
    mc = np.minimum(m, F - 1)
    Bs = np.zeros((nb,) + m.shape, cdt)
    D = np.zeros((nb,) + m.shape, rdt)
    E = np.zeros((nb,) + m.shape, rdt)
    for t in range(T):
        # the product written out in real arithmetic: both cross terms are rounded before
        # they are added, so X_k X_l and X_l X_k agree bit for bit (a library complex multiply
        # may fuse one of them)
        a, c = X[:, rows, t][:, :, None], Y[:, cols, t][:, None, :]
        P = np.empty((nb,) + m.shape, cdt)
        P.real = a.real * c.real - a.imag * c.imag
        P.imag = a.real * c.imag + a.imag * c.real
        Zm = Z[:, :, t][:, mc]
        Bs += P * np.conj(Zm)
        D += P.real * P.real + P.imag * P.imag
        E += Zm.real * Zm.real + Zm.imag * Zm.imag
        assert P.dtype == cdt and Zm.dtype == cdt
    assert Bs.dtype == cdt and D.dtype == rdt and E.dtype == rdt
    with np.errstate(invalid="ignore", divide="ignore"):
        b2 = (Bs.real * Bs.real + Bs.imag * Bs.imag) / (D * E)
    Bs = Bs / rdt(T)
    assert Bs.dtype == cdt and b2.dtype == rdt
    return np.where(inside, Bs, cdt.type(0)), np.where(inside, b2, rdt(0))


def bispectrum(x, y=None, z=None, fs=1.0, window="hann", nperseg=256, noverlap=None,
               detrend="constant", scaling="density", navg=0, nbins=None, dtype=np.float64,
               sel=None):
    """(bispec, b2), each [batch, G, K, K]; with sel (bin indices) the rows and columns sel of
    the full plane, [batch, G, len(sel), len(sel)]. y, z None: x."""
    noverlap = nperseg // 2 if noverlap is None else noverlap
    F = nperseg // 2 + 1
    K = F if nbins is None else nbins
    idx = np.arange(K) if sel is None else np.asarray(sel)
    x = np.atleast_2d(x)
    sig = [x, x if y is None else np.atleast_2d(y), x if z is None else np.atleast_2d(z)]
    kw = dict(fs=fs, window=window, nperseg=nperseg, noverlap=noverlap, detrend=detrend,
              scaling=scaling, mode="complex")
    bis, b2 = [], []
    for sl in group_slices(x.shape[1], nperseg, noverlap, navg):
        spec = {}
        for s in sig:  # a signal given twice is transformed once
            if id(s) not in spec:
                spec[id(s)] = scipy.signal.spectrogram(s[:, sl].astype(dtype), **kw)[2]
        Bg, bg = accumulate(*(spec[id(s)] for s in sig), idx, idx)
        bis.append(Bg)
        b2.append(bg)
    want = np.complex64 if dtype == np.float32 else np.complex128
    out = np.stack(bis, axis=1), np.stack(b2, axis=1)
    assert out[0].dtype == want  # scipy really ran in `dtype`
    return out


def triple_loop(X, Y, Z, K):
    """The definition, literally: B, b2 [K, K] from spectra [F, T] in complex128."""
    F, T = X.shape
    B = np.zeros((K, K), np.complex128)
    b2 = np.zeros((K, K))
    for k in range(K):
        for l in range(K):
            if k + l > F - 1:
                continue
            s, d, e = 0j, 0.0, 0.0
            for t in range(T):
                p = X[k, t] * Y[l, t]
                s += p * np.conj(Z[k + l, t])
                d += abs(p) ** 2
                e += abs(Z[k + l, t]) ** 2
            B[k, l] = s / T
            b2[k, l] = abs(s) ** 2 / (d * e) if d * e != 0 else np.nan
    return B, b2


# the coupling recipe: 48 independent 128-sample segments of cos(12) + cos(20) + 0.5 cos(32)
# (in bins) + 0.1 N(0, 1), the phases uniform per segment; coupled: phi3 = phi1 + phi2
COUPLING = dict(window="hann", nperseg=128, noverlap=0, detrend=False, scaling="density")
COUPLING_SEED = 1979


def coupling_signal(coupled, seed=COUPLING_SEED):
    rng = np.random.default_rng(seed)
    n = np.arange(128)
    segs = []
    for _ in range(48):
        p1, p2, p3 = rng.uniform(0, 2 * np.pi, 3)
        if coupled:
            p3 = p1 + p2
        segs.append(np.cos(2 * np.pi * 12 * n / 128 + p1) + np.cos(2 * np.pi * 20 * n / 128 + p2)
                    + 0.5 * np.cos(2 * np.pi * 32 * n / 128 + p3) + 0.1 * rng.standard_normal(128))
    return np.concatenate(segs).astype(np.float32)
