"""A plain numpy / scipy restatement of the two-point wavenumber-frequency spectrum S(k, f)
that specenh.wavenumber computes (include/specenh_wavenumber.h), shared by the CPU and GPU
tests.

X_t[f], Y_t[f] are column t of scipy.signal.spectrogram(s, ..., mode='complex') on each
group's slice (the slices of tests/bispectrum_local.py); for an even K in [4, 256]

    c      = conj(X_t[f]) Y_t[f]
    theta  = atan2(Im c, Re c);  c == 0 -> theta = 0
    j      = (rint(theta K / (2 pi)) + K/2) mod K
    w      = o[f] (|X_t[f]|^2 + |Y_t[f]|^2) / 2        o = 2 for 0 < f < N/2, else 1
    S[b, g, f, j] = (1/T_g) sum over the group's frames with j_t[f] == j of w_t[f]

in a chosen dtype: the float32 run is complex64 / float32 throughout (asserted), which gives the
reference's own rounding, bin flips included, that the comparison rules below are taken from.

Rounding can move a sample across a bin edge, so histograms are compared row by row
(`compare`): a row (b, g, f) is flipped when sum_j |S - S_ref| / sum_j S_ref > FLIP; at most
max(1, 1 %) of a configuration's rows may be flipped; the unflipped rows agree to TOL normwise
per shot; in a flipped row the total still agrees to TOL and the moved weight went to a
cyclically adjacent bin.
"""
import functools
import math

import numpy as np
import scipy.signal

from bispectrum_local import group_slices

FS = 5e5
FLIP = 1e-5  # a row is flipped above this relative L1 distance
TOL = 1e-5   # the project's bound for every averaged spectrum (TOL_BISPEC, README parity line)

# (nperseg, noverlap, length, nk, B, navg, window, detrend): x and y distinct
PARITY = [
    (64, 32, 2048, 16, 4, 0, "hann", "constant"),
    (128, 96, 4096, 64, 3, 0, "hamm", "constant"),     # T = 125: crosses the chunk
    (128, 96, 4096, 256, 3, 0, "hamm", "constant"),    # nk = 256: the LDS maximum
    (128, 96, 4096, 64, 3, 7, "hamm", "constant"),     # G = 17, six frames left over
    (128, 96, 4096, 256, 3, 7, "hamm", "constant"),
    (256, 128, 8192, 128, 2, 0, "hann", "linear"),
    (1024, 768, 16384, 32, 2, 0, "hamm", "constant"),  # F = 513: partial last tile of bins
    (4096, 2048, 12288, 8, 1, 0, "hann", "constant"),  # T = 5: largest transform
    (128, 0, 128, 4, 1, 0, "hann", "constant"),        # T = 1
    (128, 0, 4224, 4, 1, 33, "hann", "constant"),      # one frame past a chunk
]


def cfg_id(c):
    return "-".join(str(v) for v in c)


def onesided(F):
    """o[f]: 2 for 0 < f < N/2, else 1 (F = N/2 + 1)."""
    o = np.full(F, 2.0)
    o[0] = o[F - 1] = 1.0
    return o


def histogram(X, Y, K, o):
    """S [batch, F, K] from the spectra [batch, F, T] of one group, in the spectra's precision;
    o [F] the per-bin factor."""
    cdt = X.dtype
    rdt = np.float32 if cdt == np.complex64 else np.float64
    assert cdt in (np.complex64, np.complex128) and Y.dtype == cdt
    nb, F, T = X.shape
    # conj(X) Y written out in real arithmetic, so every intermediate has the run's precision
    re = X.real * Y.real + X.imag * Y.imag
    im = X.real * Y.imag - X.imag * Y.real
    theta = np.where((re == 0) & (im == 0), rdt(0), np.arctan2(im, re))
    q = np.rint(theta * rdt(K / (2 * np.pi)))
    w = (X.real * X.real + X.imag * X.imag + Y.real * Y.real + Y.imag * Y.imag) * rdt(0.5)
    w = w * o.astype(rdt)[None, :, None]
    assert re.dtype == rdt and theta.dtype == rdt and q.dtype == rdt and w.dtype == rdt
    j = (q.astype(np.int64) + K // 2) % K
    S = np.zeros((nb, F, K), rdt)
    bi, fi = np.meshgrid(np.arange(nb), np.arange(F), indexing="ij")
    for t in range(T):  # ascending frame order; (b, f, j_t) is unique within a frame
        S[bi, fi, j[:, :, t]] += w[:, :, t]
    S = S / rdt(T)
    assert S.dtype == rdt
    return S


def wavenumber_spectrum(x, y, fs=1.0, window="hann", nperseg=256, noverlap=None,
                        detrend="constant", scaling="density", navg=0, nk=64, dtype=np.float64):
    """S [batch, G, F, nk] in `dtype`."""
    noverlap = nperseg // 2 if noverlap is None else noverlap
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    kw = dict(fs=fs, window=window, nperseg=nperseg, noverlap=noverlap, detrend=detrend,
              scaling=scaling, mode="complex")
    out = []
    for sl in group_slices(x.shape[1], nperseg, noverlap, navg):
        X = scipy.signal.spectrogram(x[:, sl].astype(dtype), **kw)[2]
        Y = X if y is x else scipy.signal.spectrogram(y[:, sl].astype(dtype), **kw)[2]
        assert X.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
        out.append(histogram(X, Y, nk, onesided(X.shape[1])))
    return np.stack(out, axis=1)


def triple_loop(X, Y, K, o):
    """The definition, literally: S [F, K] from spectra [F, T], looping over f, t and j."""
    F, T = X.shape
    S = np.zeros((F, K))
    for f in range(F):
        for t in range(T):
            c = np.conj(X[f, t]) * Y[f, t]
            theta = math.atan2(c.imag, c.real) if c != 0 else 0.0
            jt = (round(theta * K / (2 * math.pi)) + K // 2) % K  # round: half to even, as rint
            w = o[f] * (abs(X[f, t]) ** 2 + abs(Y[f, t]) ** 2) / 2
            for j in range(K):
                if j == jt:
                    S[f, j] += w / T
    return S


def k_grid(K, dx=1.0):
    return np.fft.fftshift(np.fft.fftfreq(K)) * 2 * np.pi / dx


def phase_bin(theta, K):
    """The bin of a phase (any real, wrapped here)."""
    theta = np.angle(np.exp(1j * np.asarray(theta, dtype=np.float64)))
    return (np.rint(theta * K / (2 * np.pi)).astype(np.int64) + K // 2) % K


def compare(S, ref):
    """The row-by-row comparison of a histogram S with the float64 reference, both
    [B, G, F, K]. Returns a dict of the measured figures; `check` asserts on them."""
    S, ref = np.asarray(S, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert S.shape == ref.shape and np.isfinite(S).all()
    D = S - ref
    tot = ref.sum(-1)
    l1 = np.abs(D).sum(-1)
    flipped = l1 > FLIP * tot
    rows = flipped.size
    err = np.where(flipped[..., None], 0.0, np.abs(D))
    unflipped = float((err.max(axis=(1, 2, 3)) / ref.max(axis=(1, 2, 3))).max())
    total, emd = 0.0, 0.0  # over the flipped rows: total mismatch; transport cost / moved weight
    for d, r in zip(D[flipped], ref[flipped]):
        total = max(total, abs(d.sum()) / r.sum())
        C = np.cumsum(d)
        emd = max(emd, np.abs(C - np.median(C)).sum() / (np.abs(d).sum() / 2))
    return dict(rows=rows, flipped=int(flipped.sum()), cap=max(1.0, 0.01 * rows),
                unflipped=unflipped, total=total, emd=emd)


def check_cap(m):
    assert m["flipped"] <= m["cap"], m
    assert m["unflipped"] <= TOL, m


def check(m):
    check_cap(m)
    assert m["total"] <= TOL, m
    assert m["emd"] <= 1 + 1e-3, m  # the moved weight went to a cyclically adjacent bin


@functools.lru_cache(maxsize=None)
def signals(B, L, seed=11):
    """The partly coherent x, y of tests/test_spectral_gpu.py (fp64 recipe, cast to fp32)."""
    from specenh.synthetic import plasma_chirps

    x = plasma_chirps(B, L, seed0=seed, dtype=np.float64)
    y = 0.7 * np.roll(x, 3, axis=1) + 0.5 * plasma_chirps(B, L, seed0=seed + 100,
                                                          dtype=np.float64)
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def ref_kw(cfg):
    n, nov, _, nk, _, navg, w, detrend = cfg
    return dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, navg=navg, nk=nk)


@functools.lru_cache(maxsize=None)
def reference(cfg, dtype=np.float64):
    """The oracle on signals(B, L) of a PARITY configuration, read-only."""
    x, y = signals(cfg[4], cfg[2])
    S = wavenumber_spectrum(x, y, dtype=dtype, **ref_kw(cfg))
    S.setflags(write=False)
    return S


# the delayed pair: y[n] = x[n - DELAY] + weak noise, x white. With nperseg = 128 the phase of
# bin f is -2 pi f DELAY / 128 = -f * 5.625 degrees, a bin centre of K = 64 (width 5.625
# degrees), so the ridge is not decided on an edge.
DELAY = dict(fs=FS, window="hann", nperseg=128, noverlap=64, detrend="constant", nk=64)
DELAY_D = 2


@functools.lru_cache(maxsize=None)
def delayed_pair(L=128 + 64 * 63, seed=1982):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(L + DELAY_D)
    x = s[DELAY_D:]
    y = s[:L] + 0.01 * rng.standard_normal(L)
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def delay_phase():
    """theta[f] = -2 pi f d / fs per bin of the delayed pair, unwrapped."""
    n = DELAY["nperseg"]
    f = np.arange(n // 2 + 1) * FS / n
    return -2 * np.pi * f * DELAY_D / FS
