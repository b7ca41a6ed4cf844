"""The fp64 restatement of the steered-response spectra (numpy and scipy only): the raw weighted
sum of squared projections, the Bartlett, Capon and MUSIC estimators from a matrix or from given
eigenpairs, the cross-spectral matrices of scipy.signal.csd, and the signal generator the
beamforming tests share (plane-wave modes plus white noise on an irregular angle array); the
case grids of the kernel tests, and the two CPU measurements their tolerances come from
(restatement32_error, chain32).

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


# (M, C, K, count, per_bin): the ends of each axis together (M, C in {1, 64}, K in {1, 257},
# count in {1, 7}) and the values around one tile of 32 rows, 32 channels and 32 steering rows.
# Of the channel axis that is C = 1, 2, 3, 31, 32, 33, 63, 64: four of the kernel's eight
# instantiations (KH = 4, 16, 20, 32). CHANNEL_CASES below visits the rest.
KERNEL_CASES = [(1, 1, 1, 1, False), (64, 64, 257, 7, False), (1, 64, 257, 1, False),
                (64, 1, 1, 7, True), (2, 2, 31, 7, False), (15, 3, 32, 1, False),
                (16, 31, 33, 7, True), (17, 32, 65, 1, False), (31, 33, 257, 7, True),
                (32, 63, 1, 1, False), (33, 64, 65, 7, True), (64, 3, 31, 7, False),
                (1, 64, 1, 7, False), (64, 1, 257, 1, False)]

# One case per channel count: launch_steered (csrc/steered_power.hip) picks the instantiation
# steered_power_kernel<KH> by (C - 1) / 8, KH = 4, 8, .. 32, eight channel counts each, and
# lane half h owns the channels [h KH, (h + 1) KH): C = 1 (mod 8) leaves the high half one
# channel, C = 0 (mod 8) none to pad. M gives one to four row tiles with a partial last one, K
# one wave, a full workgroup and a second one. No M = 1: a single random row makes 1 / q
# ill-conditioned (the fp32 restatement itself is off by 9.6e-6 there for INVERSE), which would
# test the conditioning and not the kernel.
CHANNEL_CASES = [((16, 31, 33, 65, 97)[C % 5], C, (1, 31, 33, 129, 130)[(C // 3) % 5], 3,
                  bool(C & 1)) for C in range(1, 65)]


def instantiation(C):
    """The index of the kernel launch_steered picks: steered_power_kernel<4 (index + 1)>."""
    return (C - 1) // 8


def restatement32_error(cases):
    """The error of the fp32 restatement against the fp64 one over `cases`, w null and given:
    [SUM, BARTLETT, INVERSE, MUSIC] normwise, the epilogue in fp64 on the fp32 sum as in the
    kernel. The kernel tolerances are 4 x this on KERNEL_CASES."""
    worst = [0.0] * 4
    for case in cases:
        V, A, w = kernel_case(*case)
        for ww in (None, w):
            q, q32 = raw_q(V, ww, A), raw_q32(V, ww, A).astype(np.float64)
            for mode in range(4):
                worst[mode] = max(worst[mode], normwise(post(q32, A, mode), post(q, A, mode)))
    return worst


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


# the end-to-end case of Capon and MUSIC: 24 frames of 64 / 48 in three blocks of 8, 5 samples
# left over, two shots, mode numbers -8 .. 8 on the irregular angles, loading 1e-2, two sources
N_MODES = np.arange(-8, 9)
L_E2E = 64 + 16 * 23 + 5
E2E_KW = dict(fs=FS, window="hann", nperseg=64, noverlap=48, detrend="constant", navg=8)
E2E_SOURCES, E2E_LOADING = 2, 1e-2


@functools.lru_cache(maxsize=None)
def e2e_reference(C):
    """(x float32 [2, C, L_E2E], S complex128 [2, 33, 3, C, C] of scipy.signal.csd, A complex64
    [17, C])."""
    x = signals(2, C, L_E2E)
    S = scipy_csm(x, 64, 48, "hann", "constant", 8)
    S.setflags(write=False)
    return x, S, steering(angles(C), N_MODES).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def chain32(C):
    """What an fp32 eigensolver costs Capon and MUSIC on e2e_reference(C): the normwise
    difference between oracle/herm_eig.py (the fp32 restatement of csrc/herm_eig.hip's method)
    feeding the fp64 projection, and the all-fp64 chain (numpy.linalg.eigh), both on the scipy
    matrices. {method: value}: the entries (C, method) of CHAIN32."""
    from oracle import herm_eig

    _, S, A = e2e_reference(C)
    lam, v, _ = herm_eig.herm_eig_batch(S.reshape(-1, C, C))
    lam, v = lam.reshape(S.shape[:-1]), v.reshape(S.shape)
    return {method: normwise(
        from_eigenpairs(lam, v, A, method, E2E_SOURCES, E2E_LOADING),
        estimate(S, A, method, E2E_SOURCES, E2E_LOADING)) for method in ("capon", "music")}


# chain32(C)[method], to three digits, as measured on the CPU; the end-to-end bound of Capon
# and MUSIC against scipy matrices is 8 x this (tests/test_beamform_gpu.py), and
# tests/test_beamform_cpu.py recomputes every entry
CHAIN32 = {(5, "capon"): 4.03e-6, (5, "music"): 1.83e-5, (12, "capon"): 1.79e-5,
           (12, "music"): 1.45e-5, (20, "capon"): 3.04e-5, (20, "music"): 1.27e-5,
           (40, "capon"): 5.62e-5, (40, "music"): 1.26e-5, (44, "capon"): 5.64e-5,
           (44, "music"): 1.43e-5, (52, "capon"): 7.23e-5, (52, "music"): 1.02e-5,
           (64, "capon"): 6.90e-5, (64, "music"): 1.18e-5}
E2E_CHANNELS = sorted({C for C, _ in CHAIN32})


def local_maxima(p):
    """Indices of the strict local maxima of a 1-D array (the ends count), highest first."""
    p = np.asarray(p, dtype=np.float64)
    pad = np.concatenate(([-np.inf], p, [-np.inf]))
    idx = np.nonzero((pad[1:-1] > pad[:-2]) & (pad[1:-1] > pad[2:]))[0]
    return idx[np.argsort(-p[idx])]
