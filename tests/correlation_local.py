"""A plain numpy / scipy restatement of the block-averaged cross-correlation that
specenh.correlation computes (include/specenh_correlation.h), shared by the CPU and GPU tests.

With x_t, y_t the frames of a group (slices of the signal, scipy.signal.detrend, times the
window) and a maximum lag M:

    r_t[m]   = scipy.signal.correlate(y_t, x_t, 'full', method='direct')[N - 1 + m], m = -M .. M
    R[b,g,m] = mean over the group's frames of r_t[m]
    Ex[b,g]  = mean over the group's frames of sum_n x_t[n]^2       (Ey likewise)
    rho      = R / sqrt(Ex Ey), 0 where Ex Ey == 0

`correlation` is that in float64. `correlation_fft32` is a float32 run of the FFT formulation
the kernel uses (scipy.fft.rfft of the frames zero-padded to 2N, complex64 sums in frame order,
one irfft per group; the dtypes asserted), which gives the rounding such a formulation has.

The error of an FFT correlation scales with the signals' energies, not with R itself (which is
near zero for weakly correlated channels), so `compare` measures on the coefficient scale, for
every (b, g) row: max_m |R - R_ref| / sqrt(Ex_ref Ey_ref) <= TOL.
"""
import functools

import numpy as np
import scipy.fft
import scipy.signal

from bispectrum_local import group_slices

FS = 5e5
TOL = 1e-5   # the project's bound for every averaged spectrum (TOL in tests/wavenumber_local.py)

# (nperseg, noverlap, length, maxlag, B, navg, window, detrend): x and y distinct
PARITY = [
    (64, 32, 2048, 63, 4, 0, "boxcar", "constant"),
    (128, 96, 4096, 127, 3, 0, "hamm", "constant"),     # T = 125: crosses a chunk
    (128, 96, 4096, 16, 3, 7, "hamm", "constant"),      # G = 17, frames left over, short lags
    (256, 128, 8192, 40, 2, 0, "hann", "linear"),
    (1024, 768, 16384, 1023, 2, 0, "hamm", "constant"),
    (2048, 1024, 12288, 2047, 1, 0, "boxcar", "constant"),  # T = 5: largest transform
    (128, 0, 128, 127, 1, 0, "hann", False),            # T = 1
    (128, 0, 4224, 0, 1, 33, "boxcar", "constant"),     # only lag 0; one frame past a chunk
]


def cfg_id(c):
    return "-".join(str(v) for v in c)


def frames_of(s, nperseg, noverlap, detrend, window, dtype):
    """The detrended, windowed frames [batch, T, N] of a group's slice s [batch, len]."""
    hop = nperseg - noverlap
    T = (s.shape[1] - nperseg) // hop + 1
    fr = np.stack([s[:, t * hop:t * hop + nperseg] for t in range(T)], axis=1).astype(dtype)
    if detrend:
        fr = scipy.signal.detrend(fr, axis=-1, type=detrend)
    fr = fr * scipy.signal.get_window(window, nperseg).astype(dtype)
    assert fr.dtype == dtype
    return fr


def correlation(x, y, window="boxcar", nperseg=256, noverlap=None, detrend="constant", navg=0,
                maxlag=None):
    """dict(R [batch, G, 2 M + 1], Ex [batch, G], Ey): the direct sum in float64."""
    noverlap = nperseg // 2 if noverlap is None else noverlap
    M = nperseg - 1 if maxlag is None else maxlag
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    R, Ex, Ey = [], [], []
    for sl in group_slices(x.shape[1], nperseg, noverlap, navg):
        fx = frames_of(x[:, sl], nperseg, noverlap, detrend, window, np.float64)
        fy = fx if y is x else frames_of(y[:, sl], nperseg, noverlap, detrend, window, np.float64)
        r = np.zeros((x.shape[0], 2 * M + 1))
        for b in range(fx.shape[0]):
            for t in range(fx.shape[1]):
                full = scipy.signal.correlate(fy[b, t], fx[b, t], "full", method="direct")
                r[b] += full[nperseg - 1 - M:nperseg + M]
        R.append(r / fx.shape[1])
        Ex.append((fx * fx).sum(-1).mean(-1))
        Ey.append((fy * fy).sum(-1).mean(-1))
    return dict(R=np.stack(R, 1), Ex=np.stack(Ex, 1), Ey=np.stack(Ey, 1))


def correlation_fft32(x, y, window="boxcar", nperseg=256, noverlap=None, detrend="constant",
                      navg=0, maxlag=None):
    """R [batch, G, 2 M + 1] float32 by the FFT formulation, float32 / complex64 throughout."""
    noverlap = nperseg // 2 if noverlap is None else noverlap
    M = nperseg - 1 if maxlag is None else maxlag
    x, y = np.atleast_2d(x), np.atleast_2d(y)
    N = nperseg
    R = []
    for sl in group_slices(x.shape[1], nperseg, noverlap, navg):
        fx = frames_of(x[:, sl], nperseg, noverlap, detrend, window, np.float32)
        fy = frames_of(y[:, sl], nperseg, noverlap, detrend, window, np.float32)
        X, Y = scipy.fft.rfft(fx, n=2 * N, axis=-1), scipy.fft.rfft(fy, n=2 * N, axis=-1)
        assert X.dtype == np.complex64 and Y.dtype == np.complex64 and X.shape[-1] == N + 1
        C = np.zeros((x.shape[0], N + 1), np.complex64)
        for t in range(X.shape[1]):  # frame order
            C += np.conj(X[:, t]) * Y[:, t]
        r = scipy.fft.irfft(C, n=2 * N, axis=-1)
        assert C.dtype == np.complex64 and r.dtype == np.float32
        r = np.concatenate([r[:, 2 * N - M:], r[:, :M + 1]], axis=-1) / np.float32(X.shape[1])
        assert r.dtype == np.float32
        R.append(r)
    return np.stack(R, 1)


def coefficient(ref):
    """rho [batch, G, 2 M + 1] of a `correlation` result: 0 where Ex Ey == 0."""
    den = np.sqrt(ref["Ex"] * ref["Ey"])[..., None]
    return np.where(den > 0, ref["R"] / np.where(den > 0, den, 1.0), 0.0)


def compare(R, R_ref, scale):
    """max over the rows (b, g) of max_m |R - R_ref| / scale[b, g]: the error on the
    coefficient scale (scale = sqrt(Ex_ref Ey_ref) for a raw R, 1 for a coefficient)."""
    R, R_ref = np.asarray(R, dtype=np.float64), np.asarray(R_ref, dtype=np.float64)
    assert R.shape == R_ref.shape and np.isfinite(R).all()
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), R.shape[:2])
    return float((np.abs(R - R_ref).max(-1) / scale).max())


@functools.lru_cache(maxsize=None)
def signals(B, L, seed=23):
    """x, and y = x delayed by three samples plus as much independent signal (fp64 recipe,
    cast to fp32)."""
    from specenh.synthetic import plasma_chirps

    x = plasma_chirps(B, L, seed0=seed, dtype=np.float64)
    y = 0.7 * np.roll(x, 3, axis=1) + 0.5 * plasma_chirps(B, L, seed0=seed + 100,
                                                          dtype=np.float64)
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def ref_kw(cfg):
    n, nov, _, M, _, navg, w, detrend = cfg
    return dict(window=w, nperseg=n, noverlap=nov, detrend=detrend, navg=navg, maxlag=M)


@functools.lru_cache(maxsize=None)
def reference(cfg, auto=False):
    """The float64 restatement on signals(B, L) of a PARITY configuration (auto: y is x),
    read-only."""
    x, y = signals(cfg[4], cfg[2])
    ref = correlation(x, x if auto else y, **ref_kw(cfg))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def shape_of(cfg, B=None):
    n, nov, L, M, b, navg = cfg[:6]
    T = (L - n) // (n - nov) + 1
    return (b if B is None else B, 1 if navg <= 0 else T // navg, 2 * M + 1)


# the delayed pair: y[n] = x[n - d] + 1 % noise, x white; boxcar 256 / 128 in blocks of 8 frames
DELAY = dict(window="boxcar", nperseg=256, noverlap=128, detrend="constant", navg=8)
DELAY_MAXLAG = 32
DELAYS = (0, 3, -5)


@functools.lru_cache(maxsize=None)
def delayed_pair(d, L=256 + 128 * 31, seed=1977):
    """T = 32 frames: four groups of eight."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(L + 16)
    x = s[8:8 + L]
    y = s[8 - d:8 - d + L] + 0.01 * rng.standard_normal(L)
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y
