"""Shared by tests/test_stft_complex_local_cpu.py and tests/test_stft_complex_gpu.py: shots whose
level falls by four decades, their scipy fp64 reference, the two localised error metrics and a
plain numpy emulation of the paired-frame algorithm of csrc/stft_complex.hip.

The paired transforms carry frames (2q, 2q + 1) in one complex FFT, so a frame's rounding
error scales with the louder frame of its pair and a sample's with the loudest frame that
covers it or is the partner of one that does. The metrics divide by exactly that, and the
emulation (complex64 pairs through scipy.fft, fp32 overlap-add) shows that the algorithm itself
stays below 3e-7 under them on these inputs: a GPU value near 1e-5 is the kernel's doing.
"""
import functools

import numpy as np
import scipy.fft
import scipy.ndimage
import scipy.signal

FS = 5e5
# (L, nperseg, noverlap, window): one per supported size
LOCAL = [
    (9000, 64, 48, "hamm"),
    (9000, 128, 96, "hann"),
    (9000, 256, 128, "hann"),
    (12000, 512, 200, "hamm"),
    (12000, 1024, 768, "hamm"),
    (20000, 2048, 1536, "hann"),
    (30000, 4096, 2048, "hann"),
]
LOCAL_IDS = [f"{L}-{n}-{nov}-{w}" for L, n, nov, w in LOCAL]
BATCH = 2
KW = dict(detrend=False, boundary="zeros", padded=True, scaling="spectrum")


@functools.lru_cache(maxsize=None)
def shots(case, reverse):
    """x[b, n] = g_b[n] 10^(-4 n / L), g_b standard normal from default_rng(nperseg + b), fp32;
    reverse=True is the same shots read backwards (the loud end last)."""
    L, n, nov, w = case
    env = 10.0 ** (-4.0 * np.arange(L) / L)
    x = np.stack([np.random.default_rng(n + b).standard_normal(L) * env for b in range(BATCH)])
    x = np.ascontiguousarray(x[:, ::-1] if reverse else x, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(case, reverse):
    """scipy fp64 on the widened samples: Z, its complex64 rounding, and scipy's fp64 inverse
    of that rounded Z."""
    L, n, nov, w = case
    _, _, Z = scipy.signal.stft(shots(case, reverse).astype(np.float64), fs=FS, window=w,
                                nperseg=n, noverlap=nov, **KW)
    Z32 = np.ascontiguousarray(Z, dtype=np.complex64)
    Z32.setflags(write=False)
    _, xi = scipy.signal.istft(Z32.astype(np.complex128), fs=FS, window=w, nperseg=n,
                               noverlap=nov, boundary=True, scaling="spectrum")
    return Z, Z32, xi


def frame_error(got, ref):
    """[B][T]: max_k |got - ref| of frame t over max_k |ref| of frames t and t ^ 1 (the
    kernel's own pairing; a last frame without a partner stands alone)."""
    got, ref = np.asarray(got, dtype=np.complex128), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(got - ref).max(axis=1)
    lvl = np.abs(ref).max(axis=1)
    T = lvl.shape[1]
    partner = np.arange(T) ^ 1
    partner[partner >= T] = T - 1
    return err / np.maximum(lvl, lvl[:, partner])


def sample_error(got, ref, case):
    """[B][n_out]: |got - ref| of sample n over max |ref| on [n - R, n + R], R = nperseg + hop:
    every frame that covers the sample, and those frames' partners."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.abs(got - ref) / sample_levels(ref, case)


def frame_levels(ref):
    """[B][T]: max_k |ref| of every frame."""
    return np.abs(ref).max(axis=1)


def sample_levels(ref, case):
    """[B][n_out]: max |ref| on [n - R, n + R], R = nperseg + hop (clipped to the signal)."""
    L, n, nov, w = case
    R = n + (n - nov)
    return scipy.ndimage.maximum_filter1d(np.abs(ref), size=2 * R + 1, axis=-1, mode="constant",
                                          cval=0.0)


def spread(levels):
    """Loudest over quietest level within a shot, the smaller of the shots."""
    return float((levels.max(axis=-1) / levels.min(axis=-1)).min())


def emulate_forward(case, reverse):
    """Frames (2q, 2q + 1) as one complex64 transform z = a + i b through scipy.fft.fft, then
    A = (Z_k + conj Z_{N-k}) / 2, B = (Z_k - conj Z_{N-k}) / 2i, scaled by 1 / sum(w)."""
    L, n, nov, w = case
    hop = n - nov
    x = shots(case, reverse)
    T = reference(case, reverse)[0].shape[2]
    win = scipy.signal.get_window(w, n)
    w32 = win.astype(np.float32)
    ext = np.zeros((BATCH, (T + (T & 1) - 1) * hop + n), dtype=np.float32)
    ext[:, n // 2:n // 2 + L] = x
    out = np.zeros((BATCH, n // 2 + 1, T + (T & 1)), dtype=np.complex64)
    rs = np.float32(1.0 / win.sum())
    for t in range(0, T, 2):
        a = ext[:, t * hop:t * hop + n] * w32
        b = ext[:, (t + 1) * hop:(t + 1) * hop + n] * w32
        if t + 1 >= T:
            b = np.zeros_like(a)
        Zp = scipy.fft.fft((a + 1j * b).astype(np.complex64), axis=-1)
        assert Zp.dtype == np.complex64
        Zm = np.conj(np.roll(Zp[:, ::-1], 1, axis=-1))  # conj Z_{N-k}
        out[:, :, t] = ((Zp + Zm) * np.float32(0.5) * rs)[:, :n // 2 + 1]
        out[:, :, t + 1] = ((Zp - Zm) * np.complex64(-0.5j) * rs)[:, :n // 2 + 1]
    return out[:, :, :T]


def emulate_inverse(case, reverse):
    """X = A_full + i B_full (Hermitian extensions, the imaginary parts of DC and Nyquist
    dropped) through one complex64 scipy.fft.ifft per pair, a + i b; fp32 overlap-add in
    ascending frame order with norm = sum w^2, x = acc sum(w) / norm, trimmed by nperseg / 2."""
    L, n, nov, w = case
    hop = n - nov
    Z32 = reference(case, reverse)[1]
    T = Z32.shape[2]
    win = scipy.signal.get_window(w, n)
    w32 = win.astype(np.float32)
    acc = np.zeros((BATCH, (T - 1) * hop + n), dtype=np.float32)
    nrm = np.zeros(acc.shape[1], dtype=np.float32)

    def full(A):  # [B][F] -> [B][N]
        A = A.copy()
        A.imag[:, 0] = 0
        A.imag[:, -1] = 0
        return np.concatenate([A, np.conj(A[:, -2:0:-1])], axis=1)

    for t in range(0, T, 2):
        A = full(Z32[:, :, t])
        B = full(Z32[:, :, t + 1]) if t + 1 < T else np.zeros_like(A)
        y = scipy.fft.ifft((A + np.complex64(1j) * B).astype(np.complex64), axis=-1)
        assert y.dtype == np.complex64
        for f, v in ((t, y.real), (t + 1, y.imag)):
            if f < T:
                acc[:, f * hop:f * hop + n] += v * w32
                nrm[f * hop:f * hop + n] += w32 * w32
    out = acc * np.float32(win.sum()) / np.where(nrm > 1e-10, nrm, np.float32(1))
    assert out.dtype == np.float32
    return out[:, n // 2:acc.shape[1] - n // 2]
