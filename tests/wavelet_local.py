"""A plain numpy / scipy restatement of the complex FIR filter bank that specenh.wavelet runs
(include/specenh_wavelet.h), shared by the CPU and GPU tests.

Filter s has the taps h_s[m], m = -L_s .. L_s; for a real x of `length` samples extended by
zeros:

    W[b, s, n] = sum_m h_s[m] x_b[n - m] = np.convolve(x_b, h_s)[L_s : L_s + length]

`filter_bank_direct` is that in float64 (np.convolve: the direct sum). `filter_bank_fft32` is a
float32 / complex64 run of the overlap-save formulation the kernel uses (tables = the fp64 DFT
of the wrapped taps rounded once to complex64; per block a complex64 scipy.fft.fft, the
product, a complex64 ifft, outputs [Lmax, Lmax + V) kept; the dtypes asserted), which gives the
rounding such a formulation has.

The error of an FFT convolution scales with the largest output of the row, not with the
element, so `compare` measures per (b, s) row on the row-max scale:

    max_j |out - ref| / max_j |ref|  <= TOL        (complex)
    max_j |P - Pref|  / max_j Pref   <= 2 * TOL    (power modes: d|W|^2 = 2 |W| d|W|)

The parity inputs are broadband (white noise, chirp plus noise, noise on a DC offset of 50), so
no row is empty of signal; a pure tone leaves rows far from it with nothing but the transform's
rounding of the tone and is used only in the closed-form sign test.
"""
import functools
import math

import numpy as np
import scipy.fft

TOL = 1e-5   # the project's bound (TOL in tests/correlation_local.py)
COMPLEX, POWER, MEAN = 0, 1, 2
NFFTS = (256, 512, 1024, 2048, 4096)
MAX_HALF = 1024


def block_len(nfft, lmax, hop=1):
    """V: outputs of W a block yields."""
    return (nfft - 2 * lmax) // hop * hop


def default_nfft(lmax):
    n = 1024
    while n < 4 * lmax:
        n *= 2
    return n


def n_out(length, hop, mode):
    return length // hop if mode == MEAN else (length - 1) // hop + 1


def filters_per_workgroup(nfft, lmax, hop, mode, length, S, B, cus):
    """SC, the filters a workgroup of filterbank_kernel or filterbank_cross_kernel loops over.
    The single-signal kernel gives no way to observe it, so this restates the rule of the host
    code, plan() in csrc/filterbank_block.hpp, which both entries call (p.Vh, p.To, nblk, then
    the `while (p.SC > MIN_SC && ...)` loop): 16, halved down to 4 while the launch has fewer
    than two workgroups a CU. `cus` is the device's compute-unit count (runtime.hpp's
    device_cus)."""
    Vh = (nfft - 2 * lmax) // hop
    To = n_out(length, hop, mode)
    nblk = (To + Vh - 1) // Vh
    sc = 16
    while sc > 4 and nblk * ((S + sc - 1) // sc) * min(B, 65535) < 2 * cus:
        sc //= 2
    return sc


# ---------------------------------------------------------------- filters and inputs
def morlet(scales, w0=6.0, support=4.0):
    """The Morlet taps written out independently of specenh.wavelet.morlet_filters."""
    out = []
    for s in scales:
        L = int(math.ceil(support * s))
        m = np.arange(-L, L + 1, dtype=np.float64)
        out.append(np.pi ** -0.25 * s ** -0.5 * np.exp(1j * w0 * m / s) * np.exp(-0.5 * (m / s) ** 2))
    return out


def morlet_bank(lmax, S=12):
    """S Morlet filters, geometric scales from 1 sample up, the longest with L = lmax exactly
    (support 4)."""
    taps = morlet(np.geomspace(1.0, lmax / 4.0, S))
    assert max(h.size // 2 for h in taps) == lmax
    return taps


def random_bank(half_lengths, seed):
    """Complex, non-Hermitian taps of unit energy: a reversed or conjugated table changes the
    result."""
    rng = np.random.default_rng(seed)
    taps = []
    for L in half_lengths:
        h = rng.standard_normal(2 * L + 1) + 1j * rng.standard_normal(2 * L + 1)
        taps.append(h / np.sqrt((np.abs(h) ** 2).sum()))
    return taps


def mixed_lengths(S, lmax):
    """S half lengths from 0 to lmax, both included when S >= 2 (S = 1: lmax)."""
    if S == 1:
        return [lmax]
    return [int(round(i * lmax / (S - 1))) for i in range(S)]


def signal(kind, B, L, seed):
    """Seeded float32 [B, L], read-only. Broadband kinds: 'white', 'chirp' (a linear chirp
    plus as much noise), 'dc50' (noise on an offset of 50)."""
    rng = np.random.default_rng(seed)
    n = np.arange(L, dtype=np.float64)
    x = rng.standard_normal((B, L))
    if kind == "chirp":
        x = 0.5 * x + np.cos(2 * np.pi * (0.02 * n + 0.5 * (0.3 / max(L, 2)) * n * n))[None, :]
    elif kind == "dc50":
        x = x + 50.0
    elif kind != "white":
        raise ValueError(kind)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


# ---------------------------------------------------------------- the two restatements
def decimate(W, hop, mode):
    """[B, S, To] of the mode from the full W[B, S, length] (any float / complex dtype)."""
    L = W.shape[-1]
    if mode == COMPLEX:
        return W[..., ::hop]
    P = W.real * W.real + W.imag * W.imag
    if mode == POWER:
        return P[..., ::hop]
    To = L // hop
    return P[..., :To * hop].reshape(P.shape[:-1] + (To, hop)).mean(-1, dtype=P.dtype)


def filter_bank_direct(x, taps, hop=1, mode=COMPLEX):
    """The definition in float64: np.convolve, 'same' alignment. [B, S, To]."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    B, length = x.shape
    W = np.empty((B, len(taps), length), dtype=np.complex128)
    for s, h in enumerate(taps):
        h = np.asarray(h, dtype=np.complex128)
        L = h.size // 2
        for b in range(B):
            W[b, s] = np.convolve(x[b], h)[L:L + length]
    return decimate(W, hop, mode)


def tables64(taps, nfft):
    """[S, nfft] complex128: np.fft.fft of the wrapped taps (h[m] at index m mod nfft)."""
    H = np.zeros((len(taps), nfft), dtype=np.complex128)
    for s, h in enumerate(taps):
        L = len(h) // 2
        H[s, np.arange(-L, L + 1) % nfft] = h
    return np.fft.fft(H, axis=-1)


def filter_bank_fft32(x, taps, nfft, lmax=None, hop=1, mode=COMPLEX):
    """The overlap-save formulation in float32 / complex64. [B, S, To]."""
    x = np.atleast_2d(np.asarray(x))
    assert x.dtype == np.float32
    B, length = x.shape
    own = max(len(h) // 2 for h in taps)
    lmax = own if lmax is None else lmax
    V = block_len(nfft, lmax, hop)
    assert V >= hop >= 1 and lmax >= own
    H = tables64(taps, nfft).astype(np.complex64)
    W = np.empty((B, len(taps), length), dtype=np.complex64)
    for q in range((length + V - 1) // V):
        lo = q * V - lmax
        blk = np.zeros((B, nfft), dtype=np.complex64)
        a, e = max(lo, 0), min(lo + nfft, length)
        blk[:, a - lo:e - lo] = x[:, a:e]
        X = scipy.fft.fft(blk, axis=-1)
        y = scipy.fft.ifft(X[:, None, :] * H[None], axis=-1)
        assert X.dtype == np.complex64 and y.dtype == np.complex64
        n = min(V, length - q * V)
        W[:, :, q * V:q * V + n] = y[:, :, lmax:lmax + n]
    out = decimate(W, hop, mode)
    assert out.dtype == (np.complex64 if mode == COMPLEX else np.float32)
    return out


def compare(out, ref, mode=COMPLEX):
    """max over the rows (b, s) of max_j |out - ref| / max_j |ref|; divide a power mode's by
    2 to put it on the scale of TOL."""
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert np.isfinite(out).all(), "an element is NaN or Inf (unwritten?)"
    scale = np.abs(ref).max(-1)
    assert (scale > 0).all(), "a row of the reference is empty of signal"
    return float((np.abs(out.astype(ref.dtype) - ref).max(-1) / scale).max())


def bound(mode):
    return TOL if mode == COMPLEX else 2 * TOL


# ---------------------------------------------------------------- parity configurations
# name -> (nfft, lmax, taps, length, B, input kind). Every one is compared in all modes; the
# float64 W of a configuration is computed once (reference) and decimated per hop and mode.
def _max_half(nfft):
    return min(MAX_HALF, (nfft - 1) // 2)   # the largest Lmax that hop = 1 allows


def _configs():
    c = {}
    for nfft in NFFTS:
        lm = _max_half(nfft)
        V = block_len(nfft, lm)
        # every nfft at its largest Lmax: random complex taps of mixed lengths
        c[f"n{nfft}-max"] = (nfft, lm, ("random", tuple(mixed_lengths(3, lm)), 11), 2 * V + 17, 2,
                             "white")
        # ... and one single-tap filter [1]: L = 0, the output is x
        c[f"n{nfft}-tap1"] = (nfft, 0, ("one",), 2 * nfft + 17, 2, "white")
    # lengths around the block seams (2 V + 17 at 4096 is n4096-max above)
    for nfft, lm in ((256, 32), (4096, 1024)):
        V = block_len(nfft, lm)
        for length in (1, V - 1, V, V + 1, 2 * V + 17):
            if (nfft, length) == (4096, 2 * V + 17):
                continue
            c[f"n{nfft}-len{length}"] = (nfft, lm, ("random", tuple(mixed_lengths(3, lm)), 12),
                                         length, 2, "white")
    # filter counts that are no multiple of the chunk, mixed lengths 0 .. Lmax
    for S in (1, 5, 33):
        c[f"S{S}"] = (1024, 256, ("random", tuple(mixed_lengths(S, 256)), 13), 1041, 2, "white")
    # Morlet w0 = 6, support 4, 12 scales
    for nfft, lm, kind in ((256, 32, "chirp"), (1024, 256, "dc50"), (4096, 1024, "chirp")):
        c[f"morlet{nfft}-{kind}"] = (nfft, lm, ("morlet", lm), 2 * block_len(nfft, lm) + 17, 1, kind)
    # the hop paths at every nfft (the buffer that holds a transform's result depends on its
    # pass count, and the two-level hop mean moves the product to the other one): Lmax =
    # nfft / 8, five filters of mixed lengths
    for nfft in NFFTS:
        lm = nfft // 8
        c[f"hop{nfft}"] = (nfft, lm, ("random", tuple(mixed_lengths(5, lm)), 21),
                           2 * block_len(nfft, lm) + 17, 2, "white")
    return c


CONFIGS = _configs()
HOPS_CFG = "S5"                   # the configuration the hop cases run on: nfft 1024, Lmax 256
HOPS = (1, 3, 7, 37, 512)         # 37: three runs of the hop mean, the last partial; 512 = V


def hops_of(name):
    """The hops a configuration is compared at. hop{nfft}, with V1 = nfft - 2 Lmax: 16 is the
    last hop whose mean is one run (P = 1), 17 two runs with a single value in the second, 37
    rounds V down and leaves the last run partial, V1 is one output a block from V1 / 16 runs."""
    if name == HOPS_CFG:
        return HOPS
    if name.startswith("hop"):
        nfft, lmax = CONFIGS[name][:2]
        return (1, 16, 17, 37, block_len(nfft, lmax))
    return (1,)


# the bank test_filters_per_workgroup_do_not_change_a_bit runs: 33 filters, three chunks of 16
CHUNK_CFG = dict(nfft=256, lmax=32, length=401, S=33)
CHUNK_CASES = ((1, COMPLEX), (5, POWER), (37, MEAN))


def chunk_taps():
    return random_bank(mixed_lengths(CHUNK_CFG["S"], CHUNK_CFG["lmax"]), seed=33)


def chunk_signal(B):
    return signal("white", B, CHUNK_CFG["length"], seed=57)


def chunk_batches(hop, mode, cus):
    """(B16, B8, 2): the smallest batch that keeps SC = 16 on a device of `cus` compute units
    with the bank of CHUNK_CFG, the smallest that gives SC = 8, and 2 shots (SC = 4), by
    filters_per_workgroup."""
    def sc(B):
        return filters_per_workgroup(CHUNK_CFG["nfft"], CHUNK_CFG["lmax"], hop, mode,
                                     CHUNK_CFG["length"], CHUNK_CFG["S"], B, cus)

    B16 = next(B for B in range(1, 65536) if sc(B) == 16)
    B8 = next(B for B in range(1, B16) if sc(B) == 8)
    return B16, B8, 2
SEAM_LENGTHS = {256: (1, 191, 192, 193, 401), 4096: (1, 2047, 2048, 2049, 4113)}


@functools.lru_cache(maxsize=None)
def taps_of(name):
    spec = CONFIGS[name][2]
    if spec[0] == "one":
        return (np.array([1.0 + 0.0j]),)
    if spec[0] == "morlet":
        return tuple(morlet_bank(spec[1]))
    return tuple(random_bank(spec[1], spec[2]))


@functools.lru_cache(maxsize=None)
def signal_of(name):
    _, _, _, length, B, kind = CONFIGS[name]
    return signal(kind, B, length, seed=sum(map(ord, name)))


@functools.lru_cache(maxsize=None)
def reference(name):
    """W [B, S, length] complex128 of a configuration by the direct sum, read-only."""
    W = filter_bank_direct(signal_of(name), taps_of(name))
    W.setflags(write=False)
    return W


def cases(name):
    """(hop, mode) pairs a configuration is compared at."""
    length = CONFIGS[name][3]
    return [(h, m) for h in hops_of(name) for m in (COMPLEX, POWER, MEAN)
            if not (m == MEAN and length < h)]
