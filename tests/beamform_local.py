"""The fp64 restatement of the steered-response spectra (numpy and scipy only): the raw weighted
sum of squared projections, the Bartlett, Capon and MUSIC estimators from a matrix or from given
eigenpairs, the cross-spectral matrices of scipy.signal.csd, and the signal generator the
beamforming tests share (plane-wave modes plus white noise on an irregular angle array).

Conventions (include/specenh_beamform.h): S_ij = mean conj(X_i) X_j, a_c = exp(i kappa p_c),
a fluctuation X_c ~ exp(i kappa0 p_c) peaks at kappa = kappa0."""
import functools

import numpy as np
import scipy.signal

FS = 5e5
SUM, BARTLETT, INVERSE, MUSIC = 0, 1, 2, 3


def table_for(A, lead):
    """A[K, C] or A[F, K, C] broadcast against matrices of leading shape `lead` = (..., F, G):
    [..., K, C] ready for einsum with [..., M, C]."""
    A = np.asarray(A).astype(np.complex128)
    if A.ndim == 2:
        return A
    return A[:, None]  # [F, 1, K, C] against [..., F, G, M, C]


def raw_q(V, w, A, conj=False):
    """q[..., n] = sum_m w[..., m] |sum_c V[..., m, c] A[n, c]|^2 in complex128; A per bin as
    table_for takes it."""
    V = np.asarray(V).astype(np.complex128)
    T = table_for(A, V.shape[:-2])
    T = T.conj() if conj else T
    P = np.einsum("...mc,...nc->...mn", V, T)
    p2 = P.real ** 2 + P.imag ** 2
    if w is None:
        return p2.sum(axis=-2)
    return (np.asarray(w, dtype=np.float64)[..., None] * p2).sum(axis=-2)


def norm2(A):
    """|a_n|^2 = sum_c |A[n, c]|^2: [K], or [F, 1, K] for a table per bin."""
    A = np.asarray(A).astype(np.complex128)
    a2 = (A.real ** 2 + A.imag ** 2).sum(axis=-1)
    return a2 if A.ndim == 2 else a2[:, None]


def post(q, A, mode, scale=1.0):
    a2 = norm2(A)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mode == SUM:
            return q * scale
        if mode == BARTLETT:
            return q * scale / a2 ** 2
        if mode == INVERSE:
            return scale / q
        return a2 / q


def raw_q32(V, w, A, conj=False):
    """raw_q with every operation in complex64 / float32: the kernel's arithmetic in numpy's
    order of summation, what the kernel tolerance is set from."""
    V = np.asarray(V).astype(np.complex64)
    T = table_for(A, V.shape[:-2]).astype(np.complex64)
    T = T.conj() if conj else T
    P = np.einsum("...mc,...nc->...mn", V, T)
    assert P.dtype == np.complex64
    p2 = P.real * P.real + P.imag * P.imag
    if w is not None:
        p2 = np.asarray(w, dtype=np.float32)[..., None] * p2
    q = p2.sum(axis=-2, dtype=np.float32)
    assert q.dtype == np.float32
    return q


def normwise(got, ref):
    """max over matrices of max_n |got - ref| / max_n |ref|, over the finite reference values."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float((np.abs(got - ref).max(axis=-1) / np.abs(ref).max(axis=-1)).max())


@functools.lru_cache(maxsize=None)
def kernel_case(M, C, K, count, per_bin):
    """Random inputs of the generic operator: V complex64 [count, 1, M, C] and A complex64
    [K, C] ([count, K, C] per bin: matrix j takes table j) of unit-variance complex normal
    entries, w float32 [count, 1, M] uniform in [0.5, 1.5)."""
    rng = np.random.default_rng(((M * 131 + C) * 131 + K) * 16 + count * 2 + int(per_bin))

    def cn(*s):
        return ((rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2)).astype(
            np.complex64)

    V = cn(count, 1, M, C)
    A = cn(count, K, C) if per_bin else cn(K, C)
    w = rng.uniform(0.5, 1.5, (count, 1, M)).astype(np.float32)
    for a in (V, A, w):
        a.setflags(write=False)
    return V, A, w


# (M, C, K, count, per_bin): every value of each axis at least once, the corners together
KERNEL_CASES = [(1, 1, 1, 1, False), (64, 64, 257, 7, False), (1, 64, 257, 1, False),
                (64, 1, 1, 7, True), (2, 2, 31, 7, False), (15, 3, 32, 1, False),
                (16, 31, 33, 7, True), (17, 32, 65, 1, False), (31, 33, 257, 7, True),
                (32, 63, 1, 1, False), (33, 64, 65, 7, True), (64, 3, 31, 7, False),
                (1, 64, 1, 7, False), (64, 1, 257, 1, False)]


def bartlett(S, A):
    """sum_ij a_i S_ij conj(a_j) / |a|^4 of S[..., C, C]."""
    T = table_for(A, S.shape[:-2])
    num = np.einsum("...ni,...ij,...nj->...n", T, np.asarray(S).astype(np.complex128), T.conj())
    return num.real / norm2(A) ** 2


def from_eigenpairs(lam, v, A, method, nsources=1, loading=1e-2):
    """The estimators from eigenvalues lam[..., C] (descending) and eigenvectors as ROWS
    v[..., C, C] (hermitian_modes' convention), in fp64."""
    lam = np.asarray(lam, dtype=np.float64)
    C = lam.shape[-1]
    if method == "bartlett":  # a^T S conj(a) = sum_m lambda_m |sum_c a_c v_m[c]|^2
        return post(raw_q(v, lam, A), A, BARTLETT)
    if method == "capon":
        delta = loading * lam.sum(axis=-1, keepdims=True) / C
        d = np.maximum(lam, 0.0) + delta
        with np.errstate(divide="ignore"):  # a term with d == 0 has no weight (pseudo-inverse)
            w = np.where(d == 0, 0.0, 1.0 / d)
        return post(raw_q(v, w, A), A, INVERSE)
    w = np.ones_like(lam)
    w[..., :nsources] = 0.0
    return post(raw_q(v, w, A), A, MUSIC)


def eigenpairs(S):
    """numpy.linalg.eigh of S[..., C, C] in complex128, descending, eigenvectors as rows."""
    lam, U = np.linalg.eigh(np.asarray(S).astype(np.complex128))
    return lam[..., ::-1], np.swapaxes(U[..., ::-1], -1, -2)


def estimate(S, A, method, nsources=1, loading=1e-2):
    """The three estimators from a matrix S[..., C, C]."""
    if method == "bartlett":
        return bartlett(S, A)
    lam, v = eigenpairs(S)
    return from_eigenpairs(lam, v, A, method, nsources, loading)


def steering(positions, kappa):
    """exp(i kappa_k p_c) in complex128, [K, C]."""
    return np.exp(1j * np.asarray(kappa, dtype=np.float64)[:, None]
                  * np.asarray(positions, dtype=np.float64)[None, :])


def scipy_csm(x, n, nov, window, detrend, navg, scaling="density", fs=FS):
    """S[B, F, G, C, C] from scipy.signal.csd of every pair on each group's slice, in fp64."""
    x = np.asarray(x).astype(np.float64)
    hop = n - nov
    T = (x.shape[-1] - n) // hop + 1
    glen = navg if navg and navg >= 1 else T
    kw = dict(fs=fs, window=window, nperseg=n, noverlap=nov, detrend=detrend, scaling=scaling)
    S = []
    for g in range(T // glen):
        s = x[..., g * glen * hop: g * glen * hop + (glen - 1) * hop + n]
        _, p = scipy.signal.csd(s[:, :, None, :], s[:, None, :, :], **kw)  # [B, C, C, F]
        S.append(np.moveaxis(p, -1, 1))
    return np.stack(S, axis=2)


# the generator: modes (mode number, amplitude), each with an independent envelope in the bands
# around BINS (bins of nperseg = 64), on top of white noise
MODES = ((3, 1.0), (-2, 0.5))
BINS = (8, 20)
NOISE = 0.1  # amplitude: mode-to-noise ratios 10 and 5 (>= 3)
NPERSEG = 64


@functools.lru_cache(maxsize=None)
def angles(C, seed=5):
    """C sorted uniform random angles in [0, 2 pi)."""
    th = np.sort(np.random.default_rng(seed + C).uniform(0, 2 * np.pi, C))
    th.setflags(write=False)
    return th


@functools.lru_cache(maxsize=None)
def signals(B, C, L, seed=0):
    """x[B, C, L] float32: for each mode (n, amp) and each band an independent band-limited
    complex random signal e(t) around f = bin fs / 64 (13 tones of random phase and amplitude
    over +-1.5 bins: the two modes are incoherent over a block of 8 frames), seen at angle
    theta_c as Re(amp e(t) exp(i n theta_c)) -- X_c ~ exp(i n theta_c) at positive
    frequencies -- plus white noise of amplitude NOISE. fp64 recipe cast to fp32."""
    rng = np.random.default_rng(1000 * C + L + 7919 * seed)
    th = angles(C)
    t = np.arange(L) / FS
    x = NOISE * rng.standard_normal((B, C, L))
    for n, amp in MODES:
        for k0 in BINS:
            for b in range(B):
                env = np.zeros(L, dtype=np.complex128)
                for df in np.linspace(-1.5, 1.5, 13):
                    env += (rng.uniform(0.5, 1.0) * np.exp(2j * np.pi * rng.uniform())
                            * np.exp(2j * np.pi * (k0 + df) * FS / NPERSEG * t))
                env /= np.sqrt(13.0)
                x[b] += amp * np.real(env[None, :] * np.exp(1j * n * th)[:, None])
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def local_maxima(p):
    """Indices of the strict local maxima of a 1-D array (the ends count), highest first."""
    p = np.asarray(p, dtype=np.float64)
    pad = np.concatenate(([-np.inf], p, [-np.inf]))
    idx = np.nonzero((pad[1:-1] > pad[:-2]) & (pad[1:-1] > pad[2:]))[0]
    return idx[np.argsort(-p[idx])]
