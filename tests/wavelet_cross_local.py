"""A plain numpy restatement of the cross spectrum of a pair through a filter bank and of wavelet
coherence (include/specenh_wavelet_cross.h, specenh.wavelet.wavelet_coherence), shared by the
CPU and GPU tests. Filters, configurations and the two runs of the bank itself come from
tests/wavelet_local.py.

With Wx, Wy the outputs of the bank for x and y (wavelet_local.filter_bank_direct in float64,
wavelet_local.filter_bank_fft32 in the overlap-save float32 formulation):

    point:  sxy[j] = conj(Wx[j hop]) Wy[j hop], sxx[j] = |Wx[j hop]|^2     To = (length-1)//hop + 1
    mean:   the means of the same over each whole window of hop samples   To = length // hop

`cross` computes them in the dtype it is given: complex128 gives the reference, the complex64
output of filter_bank_fft32 the float32 restatement.

Error measures, per (b, s) row, TOL = 1e-5 as in wavelet_local:

    sxx, syy:  max_j |out - ref| / max_j ref                               <= 2 TOL
    sxy:       max_j |out - ref| / sqrt(max_j Sxx_ref max_j Syy_ref)       <= 2 TOL

The cross spectrum is measured on the product scale of the two powers, not on its own row
maximum: d(conj(Wx) Wy) = conj(dWx) Wy + conj(Wx) dWy is bounded by TOL (max|Wx| max|Wy|) twice
over whatever the coherence, while a row of low coherence and few outputs has a small max |Sxy|.

Coherence, per element, with gamma^2 = coh_ref, M the row maximum of a (smoothed) spectrum and
everything taken from the float64 reference, is the first-order propagation of those three:

    |coh - coh_ref| <= 2 TOL (2 gamma sqrt(Mxx Myy / (Sxx Syy)) + gamma^2 (Mxx / Sxx + Myy / Syy))

The inputs are seeded pairs, B = 3: x of the configuration's kind, y_b = x_b delayed by d
samples plus m_b e_b with e white and m = (0.1, 1, 3), so the coherence runs from near 1 to
near 0.1. d = 3 for the Morlet banks, 0 for the random-tap banks (their output decorrelates
within one lag, so a delayed copy would leave no coherence).
"""
import functools

import numpy as np

import wavelet_local as wl

TOL = wl.TOL
POINT, MEAN = 0, 1
B = 3
MIX = (0.1, 1.0, 3.0)
COH_ALLOWED_MAX = 2e-3   # no element's allowed coherence error may exceed this on the inputs used


def n_out(length, hop, mode):
    return length // hop if mode == MEAN else (length - 1) // hop + 1


def fb_mode(mode):
    """The filter bank's mode with the same To rule."""
    return wl.MEAN if mode == MEAN else wl.POWER


def cross(Wx, Wy, hop, mode):
    """(sxy, sxx, syy), each [B, S, To], from the full Wx, Wy [B, S, length], in their dtype."""
    assert Wx.shape == Wy.shape and Wx.dtype == Wy.dtype
    real = Wx.real.dtype
    sxy = np.conj(Wx) * Wy
    sxx = Wx.real * Wx.real + Wx.imag * Wx.imag
    syy = Wy.real * Wy.real + Wy.imag * Wy.imag
    assert sxy.dtype == Wx.dtype and sxx.dtype == real
    if mode == POINT:
        return sxy[..., ::hop], sxx[..., ::hop], syy[..., ::hop]
    To = Wx.shape[-1] // hop

    def mean(v):
        return v[..., :To * hop].reshape(v.shape[:-1] + (To, hop)).mean(-1, dtype=v.dtype)

    return mean(sxy), mean(sxx), mean(syy)


def boxcar(v, widths):
    """v[..., S, T] smoothed along the last axis, row s by a centred boxcar of the odd length
    widths[s], truncated at the ends and normalised by the count of values present; float64,
    one slice mean per element."""
    v = np.asarray(v)
    out = np.empty(v.shape, dtype=np.complex128 if np.iscomplexobj(v) else np.float64)
    T = v.shape[-1]
    for s, w in enumerate(widths):
        assert w >= 1 and w % 2 == 1
        h = int(w) // 2
        for j in range(T):
            out[..., s, j] = v[..., s, max(0, j - h):min(T, j + h + 1)].astype(out.dtype).mean(-1)
    return out


def coherence(sxy, sxx, syy, widths=None):
    """(coh, phase, smoothed sxy, sxx, syy) in float64: min(1, |Sxy|^2 / (Sxx Syy)) of the
    smoothed spectra, 0 where Sxx Syy == 0."""
    if widths is None:
        widths = np.ones(sxy.shape[-2], dtype=np.int64)
    sxy, sxx, syy = boxcar(sxy, widths), boxcar(sxx, widths), boxcar(syy, widths)
    den = sxx * syy
    with np.errstate(divide="ignore", invalid="ignore"):
        coh = np.where(den > 0, np.minimum(1.0, np.abs(sxy) ** 2 / den), 0.0)
    return coh, np.angle(sxy), sxy, sxx, syy


def coherence_allowance(coh_ref, sxx, syy):
    """The allowed |coh - coh_ref| of every element from the float64 (smoothed) spectra; inf
    where a power is zero (there both sides are 0 by definition and nothing is propagated)."""
    mxx, myy = sxx.max(-1, keepdims=True), syy.max(-1, keepdims=True)
    g = np.sqrt(coh_ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = 2 * TOL * (2 * g * np.sqrt(mxx * myy / (sxx * syy))
                       + coh_ref * (mxx / sxx + myy / syy))
    return np.where(sxx * syy > 0, a, np.inf)


def compare(out, ref):
    """The three row-scaled errors (sxy, sxx, syy) of out = (sxy, sxx, syy) against ref, each
    the maximum over the rows (b, s)."""
    (oxy, oxx, oyy), (rxy, rxx, ryy) = out, ref
    for o, r in zip(out, ref):
        o = np.asarray(o)
        assert o.shape == r.shape, (o.shape, r.shape)
        assert np.isfinite(o).all(), "an element is NaN or Inf (unwritten?)"
    mxx, myy = rxx.max(-1), ryy.max(-1)
    assert (mxx > 0).all() and (myy > 0).all(), "a row of the reference is empty of signal"
    exy = np.abs(np.asarray(oxy).astype(np.complex128) - rxy).max(-1) / np.sqrt(mxx * myy)
    exx = np.abs(np.asarray(oxx).astype(np.float64) - rxx).max(-1) / mxx
    eyy = np.abs(np.asarray(oyy).astype(np.float64) - ryy).max(-1) / myy
    return float(exy.max()), float(exx.max()), float(eyy.max())


BOUND = 2 * TOL


# ---------------------------------------------------------------- inputs and references
def delay_of(name):
    return 3 if wl.CONFIGS[name][2][0] == "morlet" else 0


def make_pair(kind, length, seed, d):
    """(x, y) float32 [B, length], read-only: y_b = x_b delayed by d (zeros shifted in) plus
    MIX[b] times white noise."""
    x = wl.signal(kind, B, length, seed)
    e = wl.signal("white", B, length, seed + 1000)
    xd = np.zeros((B, length), dtype=np.float64)
    xd[:, d:] = x[:, :length - d] if d else x
    y = (xd + np.asarray(MIX)[:, None] * e).astype(np.float32)
    y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def pair_of(name):
    _, _, _, length, _, kind = wl.CONFIGS[name]
    return make_pair(kind, length, sum(map(ord, name)) + 7, min(delay_of(name), length - 1))


@functools.lru_cache(maxsize=None)
def reference(name):
    """(Wx, Wy) [B, S, length] complex128 of a configuration by the direct sum, read-only."""
    x, y = pair_of(name)
    taps = wl.taps_of(name)
    Wx, Wy = wl.filter_bank_direct(x, taps), wl.filter_bank_direct(y, taps)
    Wx.setflags(write=False)
    Wy.setflags(write=False)
    return Wx, Wy


def cases(name):
    """(hop, mode) pairs a configuration is compared at: wavelet_local's hops, both modes."""
    length = wl.CONFIGS[name][3]
    return [(h, m) for h in wl.hops_of(name) for m in (POINT, MEAN)
            if not (m == MEAN and length < h)]


@functools.lru_cache(maxsize=2)
def _w32(name):
    """(Wx, Wy) complex64 by the overlap-save formulation in float32, blocks of nfft - 2 Lmax."""
    nfft, lmax = wl.CONFIGS[name][:2]
    x, y = pair_of(name)
    taps = wl.taps_of(name)
    return wl.filter_bank_fft32(x, taps, nfft, lmax), wl.filter_bank_fft32(y, taps, nfft, lmax)


def restatement32(name, hop, mode):
    """(sxy, sxx, syy) of a configuration by the overlap-save formulation in float32."""
    Wx, Wy = _w32(name)
    assert Wx.dtype == np.complex64
    out = cross(Wx, Wy, hop, mode)
    assert out[0].dtype == np.complex64 and out[1].dtype == np.float32
    return out


# the bank of the chunk test: wavelet_local's (33 filters, nfft 256, Lmax 32, length 401)
CHUNK_CASES = ((1, POINT), (5, POINT), (37, MEAN))


def chunk_pair(nb):
    cfg = wl.CHUNK_CFG
    x = wl.signal("white", nb, cfg["length"], seed=58)
    e = wl.signal("white", nb, cfg["length"], seed=59)
    y = (x.astype(np.float64) + np.asarray(MIX)[np.arange(nb) % 3, None] * e).astype(np.float32)
    return x, y
