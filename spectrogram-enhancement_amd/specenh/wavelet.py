"""The continuous wavelet transform of device signals and the complex FIR filter bank it runs
on: a time-frequency image whose window shrinks with the period, for modes that sweep in
frequency within a few periods (chirping Alfven eigenmodes, fishbones, ELM precursors), where
the fixed window of ``specgr`` / ``stft`` is too long at the top or too short at the bottom.

A bank of ``S`` complex filters, filter ``s`` with the taps ``h_s[m]``, ``m = -L_s .. L_s``,
applied to a real signal ``x`` of ``length`` samples extended by zeros on both sides::

    W[b, s, n] = sum_m h_s[m] * x_b[n - m]            n = 0 .. length - 1
               = np.convolve(x_b, h_s)[L_s : L_s + length]

With the Morlet taps of ``morlet_filters``,
``h_s[m] = pi^(-1/4) s^(-1/2) exp(i w0 m / s - m^2 / (2 s^2))`` (``s`` in samples), this is the
wavelet transform ``W_n(s)`` of Torrence & Compo (1998), eq. 1-2 with ``dt = 1``: for Morlet
``conj psi(-eta) = psi(eta)``, so their correlation with the conjugate wavelet is the
convolution above. A unit-variance white signal has ``E |W|^2 = 1`` at every scale.

Outputs are decimated by ``hop``: the complex values ``W[.., j hop]``, their power, or the mean
power of each whole window of ``hop`` samples (the time-smoothed scalogram of Torrence & Compo
section 6; it turns a 65,536-sample shot into an image a few hundred columns wide without
sampling a fluctuating power). The scalogram is a ``scales x time`` image of the same kind as
``specgr``'s, so ``specenh.svd.denoiseSignal`` and the autoencoder take it unchanged.

One fused pass (csrc/filterbank.hip through ``torch.ops.specenh.filterbank`` ->
``specenh_filterbank``): overlap-save blocks of ``nfft`` points, each transformed once on the
chip and multiplied with every filter's table there; the products and inverse transforms never
reach memory. Results stay on the device; scales, frequencies and times are float64 numpy
arrays computed on the host. The longest filter has ``L <= 1024``; there is no CPU fallback.

Two channels: ``cross_filter_bank`` / ``cross_wavelet`` give ``conj(Wx) Wy``, ``|Wx|^2`` and
``|Wy|^2`` per scale, sampled or as hop-window means, in one fused pass of their own
(csrc/filterbank_cross.hip through ``torch.ops.specenh.filterbank_cross``: neither ``Wx`` nor
``Wy`` is written), and ``wavelet_coherence`` the time-resolved coherence and phase per scale
(Torrence & Webster 1999; Grinsted et al. 2004): whether a chirp on one probe is coherent with
the one on another, and with what phase (phase over probe separation is the mode number).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .spectral import _gpu_only

_MODES = {"complex": _lib.FB_COMPLEX, "power": _lib.FB_POWER, "mean_power": _lib.FB_POWER_MEAN}
W0 = 6.0       # the Morlet wavelet's centre frequency (Torrence & Compo's choice)
SUPPORT = 4.0  # taps out to |m| <= ceil(SUPPORT s): exp(-8) of the peak


def _scales(scales):
    s = np.atleast_1d(np.asarray(scales, dtype=np.float64))
    if s.ndim != 1 or s.size < 1 or not np.isfinite(s).all() or (s <= 0).any():
        raise ValueError("scales must be positive and finite, [S]")
    return s


def scale_to_frequency(scales, fs: float = 1.0, w0: float = W0) -> np.ndarray:
    """The Fourier frequency of each Morlet scale (in samples),
    ``f = fs (w0 + sqrt(2 + w0^2)) / (4 pi s)``: Torrence & Compo Table 1 (a period of 1.03 s
    for ``w0 = 6``). Host, float64."""
    return float(fs) * (w0 + math.sqrt(2.0 + w0 * w0)) / (4.0 * math.pi * _scales(scales))


def frequency_to_scale(freqs, fs: float = 1.0, w0: float = W0) -> np.ndarray:
    """The inverse of ``scale_to_frequency``: the scale in samples of each frequency."""
    return scale_to_frequency(freqs, fs, w0)  # s and f enter symmetrically


def morlet_scales(fmin: float, fmax: float, fs: float = 1.0, voices_per_octave: int = 16,
                  w0: float = W0) -> np.ndarray:
    """Scales in samples, geometric with ``voices_per_octave`` per factor of two, ascending,
    whose frequencies span ``[fmin, fmax]``: the first is the scale of ``fmax``, the last the
    first of the sequence at or past the scale of ``fmin``."""
    if not 0 < fmin <= fmax:
        raise ValueError("0 < fmin <= fmax is required")
    if int(voices_per_octave) != voices_per_octave or voices_per_octave < 1:
        raise ValueError("voices_per_octave must be a positive integer")
    s0 = float(frequency_to_scale(fmax, fs, w0)[0])
    n = int(math.ceil(voices_per_octave * math.log2(fmax / fmin) - 1e-9))
    return s0 * 2.0 ** (np.arange(n + 1, dtype=np.float64) / voices_per_octave)


def morlet_filters(scales, w0: float = W0, support: float = SUPPORT):
    """The Morlet taps of each scale: a list of complex128 arrays, filter ``s`` of
    ``2 L_s + 1`` taps from ``m = -L_s``, ``L_s = ceil(support * s)``,
    ``h_s[m] = pi^(-1/4) s^(-1/2) exp(i w0 m / s - m^2 / (2 s^2))``."""
    out = []
    for s in _scales(scales):
        L = int(math.ceil(support * s))
        m = np.arange(-L, L + 1, dtype=np.float64)
        out.append(math.pi ** -0.25 / math.sqrt(s) * np.exp(1j * w0 * m / s - m * m / (2 * s * s)))
    return out


def cone_of_influence(scales, length: int, hop: int = 1) -> np.ndarray:
    """bool ``[S, To]``, ``To = (length - 1) // hop + 1``: True where output ``j`` (sample
    ``j hop``) of scale ``s`` lies within the e-folding time ``sqrt(2) s`` of an end of the
    signal, where the zero extension is felt (Torrence & Compo section 3g)."""
    n = np.arange(0, int(length), int(hop), dtype=np.float64)
    edge = np.minimum(n, (int(length) - 1) - n)
    return edge[None, :] < math.sqrt(2.0) * _scales(scales)[:, None]


class FilterBank:
    """The device tables of a bank of complex FIR filters.

    ``taps``: a sequence of 1-D complex arrays of odd lengths ``2 L_s + 1`` (tap ``m = -L_s``
    first). ``nfft``: the overlap-save transform length, one of 256, 512, 1024, 2048, 4096;
    None: the smallest of them ``>= 4 Lmax`` and at least 1024. ``lmax``: the half length the
    blocks are laid out for, by default the longest filter's; two banks with the same ``nfft``
    and ``lmax`` give bit-identical rows for the same taps."""

    def __init__(self, taps, nfft=None, device="cuda", lmax=None):
        from . import ops
        taps = [np.asarray(h, dtype=np.complex128) for h in taps]
        if not taps:
            raise ValueError("a filter bank needs at least one filter")
        for h in taps:
            if h.ndim != 1 or h.size % 2 != 1:
                raise ValueError("every filter must be 1-D with an odd number of taps")
        self.half_lengths = np.array([h.size // 2 for h in taps], dtype=np.intc)
        own = int(self.half_lengths.max())
        self.lmax = own if lmax is None else int(lmax)
        if self.lmax < own:
            raise ValueError(f"lmax = {self.lmax} is shorter than the longest filter ({own})")
        if self.lmax > _lib.FB_MAX_HALF:
            raise ValueError(f"the longest filter has L = {self.lmax}; L <= {_lib.FB_MAX_HALF} "
                             "is required")
        if nfft is not None and int(nfft) not in _lib.FB_NFFT:
            raise ValueError(f"nfft must be one of {_lib.FB_NFFT}, got {nfft}")
        self.nfft = ops.filterbank_nfft(self.lmax, nfft)
        self.nscales = len(taps)
        self.tables = ops.filterbank_tables(np.concatenate(taps), self.half_lengths, self.nfft,
                                            device)
        self.device = self.tables.device  # "cuda" resolved to the current device's index

    def block(self, hop: int = 1) -> int:
        """Outputs of ``W`` a block yields: ``nfft - 2 lmax`` rounded down to a multiple of hop."""
        return (self.nfft - 2 * self.lmax) // int(hop) * int(hop)


def _check_call(bank, hop, mean, shape_msg, *signals) -> int:
    """The checks filter_bank and cross_filter_bank make alike, in their order: the bank, the
    signals' ``[..., length]`` shape (one length), hop, the block and the length. Returns the
    length."""
    if not isinstance(bank, FilterBank):
        raise TypeError("bank must be a FilterBank")
    if any(v.dim() < 1 or v.shape[-1] != signals[0].shape[-1] for v in signals):
        raise ValueError(shape_msg)
    if int(hop) != hop or hop < 1:
        raise ValueError(f"hop must be a positive integer, got {hop}")
    if 2 * bank.lmax + hop > bank.nfft:
        raise ValueError(f"2 lmax + hop must not exceed nfft: 2 * {bank.lmax} + {hop} > "
                         f"{bank.nfft}")
    L = signals[0].shape[-1]
    if L < 1 or (mean and L < hop):
        raise ValueError(f"signal of {L} samples is shorter than " +
                         (f"hop = {hop}" if L else "one sample"))
    return L


def _check_device(bank, **signals):
    """Every signal on a ROCm device, and on the bank's."""
    for v in signals.values():
        _gpu_only(v, "wavelet")
    if any(v.device != bank.device for v in signals.values()):
        where = ", ".join(f"{n} on {v.device}" for n, v in signals.items())
        raise ValueError(f"{where}, the bank on {bank.device}".replace(" on ", " is on ", 1))


def _rows(v, lead, L):
    """``v`` broadcast to ``lead + (L,)`` as float32 rows ``[B, L]`` the kernels can stride."""
    v = v.expand(lead + (L,)).reshape(-1, L)
    if v.dtype != torch.float32:
        v = v.float()
    if v.stride(1) != 1 or (v.shape[0] > 1 and v.stride(0) < L):
        v = v.contiguous()  # a broadcast signal (stride 0) is materialised
    return v


def filter_bank(x: torch.Tensor, bank: FilterBank, hop: int = 1, mode: str = "complex"):
    """``bank`` applied to ``x[..., length]`` on a ROCm device: ``[..., S, To]``, complex64
    ``W[.., j hop]`` (``mode="complex"``), float32 ``|W[.., j hop]|^2`` (``"power"``), both with
    ``To = (length - 1) // hop + 1``, or float32 mean of ``|W|^2`` over each whole window of
    ``hop`` samples (``"mean_power"``, ``To = length // hop``)."""
    try:
        kind = _MODES[mode]
    except (KeyError, TypeError):
        raise ValueError(f"mode must be 'complex', 'power' or 'mean_power', got {mode!r}") from None
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    L = _check_call(bank, hop, kind == _lib.FB_POWER_MEAN, "x must be [..., length]", x)
    _check_device(bank, x=x)
    lead = x.shape[:-1]
    out = torch.ops.specenh.filterbank(_rows(x, lead, L), bank.tables, bank.lmax, int(hop), kind)
    return out.reshape(lead + out.shape[1:])


def _morlet_bank(scales, x, w0, support, nfft, bank):
    if bank is not None:
        return bank
    return FilterBank(morlet_filters(scales, w0, support), nfft=nfft, device=x.device)


def cwt(x: torch.Tensor, scales, hop: int = 1, w0: float = W0, support: float = SUPPORT,
        nfft=None, bank: FilterBank | None = None) -> torch.Tensor:
    """The Morlet wavelet transform of ``x[..., length]`` at ``scales`` (in samples): complex64
    ``[..., S, To]``, ``W[.., j hop]``. ``bank``: a ``FilterBank`` of ``morlet_filters(scales,
    ...)`` built once for many calls."""
    if isinstance(x, torch.Tensor):
        _gpu_only(x, "wavelet")
    return filter_bank(x, _morlet_bank(scales, x, w0, support, nfft, bank), hop, "complex")


def scalogram(x: torch.Tensor, scales, hop: int = 1, mean: bool = True, w0: float = W0,
              support: float = SUPPORT, nfft=None, bank: FilterBank | None = None):
    """The Morlet scalogram ``|W|^2`` of ``x[..., length]``: float32 ``[..., S, To]``, the mean
    over each whole window of ``hop`` samples (``mean=True``, ``To = length // hop``) or the
    power at every ``hop``-th sample (``To = (length - 1) // hop + 1``)."""
    if isinstance(x, torch.Tensor):
        _gpu_only(x, "wavelet")
    return filter_bank(x, _morlet_bank(scales, x, w0, support, nfft, bank), hop,
                       "mean_power" if mean else "power")


# ---------------------------------------------------------------- two channels
def cross_filter_bank(x: torch.Tensor, y: torch.Tensor, bank: FilterBank, hop: int = 1,
                      mean: bool = True):
    """The cross spectrum of ``x[..., length]`` and ``y[..., length]`` through ``bank`` on a ROCm
    device, in one fused pass (csrc/filterbank_cross.hip; ``Wx`` and ``Wy`` never reach memory):
    ``(Sxy, Sxx, Syy)``, complex64 ``conj(Wx) Wy`` and float32 ``|Wx|^2``, ``|Wy|^2``, each
    ``[..., S, To]``; the means over each whole window of ``hop`` samples (``mean=True``,
    ``To = length // hop``) or the values at every ``hop``-th sample
    (``To = (length - 1) // hop + 1``). The leading dimensions of ``x`` and ``y`` broadcast
    against each other. ``conj(x) y`` as in ``specenh.spectral.csd``: a ``y`` that lags ``x``
    has a negative phase at the scales that carry the signal."""
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise TypeError("x and y must be torch.Tensors")
    L = _check_call(bank, hop, mean, "x and y must be [..., length] with the same length", x, y)
    try:
        lead = torch.broadcast_shapes(x.shape[:-1], y.shape[:-1])
    except RuntimeError:
        raise ValueError(f"the leading dimensions of x {tuple(x.shape[:-1])} and y "
                         f"{tuple(y.shape[:-1])} do not broadcast") from None
    _check_device(bank, x=x, y=y)
    out = torch.ops.specenh.filterbank_cross(_rows(x, lead, L), _rows(y, lead, L), bank.tables,
                                             bank.lmax, int(hop),
                                             _lib.XWT_MEAN if mean else _lib.XWT_POINT)
    return tuple(o.reshape(lead + o.shape[1:]) for o in out)


def cross_wavelet(x: torch.Tensor, y: torch.Tensor, scales, hop: int = 1, mean: bool = True,
                  w0: float = W0, support: float = SUPPORT, nfft=None,
                  bank: FilterBank | None = None):
    """The Morlet cross-wavelet spectrum of ``x`` and ``y`` at ``scales`` (in samples):
    ``cross_filter_bank`` with the bank of ``morlet_filters(scales, ...)``;
    ``(Sxy, Sxx, Syy)``, ``Sxy = conj(Wx) Wy`` (Torrence & Compo 1998 section 6c with the
    project's conjugation), ``Sxx`` and ``Syy`` the two scalograms."""
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise TypeError("x and y must be torch.Tensors")
    _gpu_only(x, "wavelet")
    _gpu_only(y, "wavelet")
    return cross_filter_bank(x, y, _morlet_bank(scales, x, w0, support, nfft, bank), hop, mean)


def smoothing_windows(scales, hop: int, cycles: float = 3.0, w0: float = W0) -> np.ndarray:
    """The time smoothing of wavelet coherence in hop windows, host int64 ``[S]``:
    ``n_s = 2 floor(cycles period_s / (2 hop)) + 1`` with ``period_s = 1 /
    scale_to_frequency(s)`` samples, odd and at least 1: a length proportional to the scale
    (Torrence & Webster 1999), without which the coherence of any two signals is 1."""
    if int(hop) != hop or hop < 1:
        raise ValueError(f"hop must be a positive integer, got {hop}")
    if not cycles >= 0:
        raise ValueError("cycles must be >= 0")
    period = 1.0 / scale_to_frequency(scales, 1.0, w0)
    return 2 * np.floor(cycles * period / (2.0 * int(hop))).astype(np.int64) + 1


def _boxcar(v: torch.Tensor, widths) -> torch.Tensor:
    """``v[..., S, T]`` smoothed along the last axis, row ``s`` by a centred boxcar of the odd
    length ``widths[s]``, truncated at the ends and normalised by the count of values present;
    cumulative sums in float64 (complex128). Returns the wide dtype."""
    T = v.shape[-1]
    wide = v.to(torch.complex128 if v.is_complex() else torch.float64)
    c = torch.cat([torch.zeros_like(wide[..., :1]), wide.cumsum(-1)], dim=-1)  # [..., S, T + 1]
    half = torch.as_tensor(np.asarray(widths, dtype=np.int64) // 2, device=v.device)[:, None]
    j = torch.arange(T, device=v.device)[None, :]
    lo = (j - half).clamp(min=0)           # [S, T]
    hi = (j + half + 1).clamp(max=T)
    lo_b, hi_b = lo.expand(v.shape), hi.expand(v.shape)
    return (c.gather(-1, hi_b) - c.gather(-1, lo_b)) / (hi - lo).to(torch.float64)


def _smooth_widths(smooth, scales, hop, w0):
    S = _scales(scales).size
    if smooth is None:
        return smoothing_windows(scales, hop, w0=w0)
    n = np.asarray(smooth)
    if n.ndim == 0:
        n = np.full(S, n)
    if (n.shape != (S,) or not np.issubdtype(n.dtype, np.number) or (n != np.floor(n)).any()
            or (n < 1).any() or (n.astype(np.int64) % 2 != 1).any()):
        raise ValueError("smooth must be None, an odd positive integer or [S] of them")
    return n.astype(np.int64)


def wavelet_coherence(x: torch.Tensor, y: torch.Tensor, scales, hop: int = 1, smooth=None,
                      w0: float = W0, support: float = SUPPORT, nfft=None,
                      bank: FilterBank | None = None):
    """Wavelet coherence and phase of ``x`` and ``y`` (Torrence & Webster 1999; Grinsted et al.
    2004): ``(coh, phase, Sxy)``, float32, float32 and complex64 ``[..., S, length // hop]``.

    The three mean spectra of ``cross_wavelet(mean=True)`` are smoothed along time by a centred
    sliding boxcar of ``n_s`` hop windows at scale ``s``, truncated at the ends and normalised
    by the count of windows present (in torch, by cumulative sums in float64). ``smooth``: None
    for ``smoothing_windows(scales, hop)``, an odd integer for every scale, or ``[S]`` of them;
    1 means no smoothing beyond the hop mean. Then ``coh = min(1, |Sxy|^2 / (Sxx Syy))``, 0
    where ``Sxx Syy == 0``, and ``phase = angle(Sxy)``; ``Sxy`` is returned smoothed. Phase over
    probe separation is the mode number."""
    widths = _smooth_widths(smooth, scales, hop, w0)
    sxy, sxx, syy = cross_wavelet(x, y, scales, hop, True, w0, support, nfft, bank)
    sxy, sxx, syy = _boxcar(sxy, widths), _boxcar(sxx, widths), _boxcar(syy, widths)
    den = sxx * syy
    num = sxy.real * sxy.real + sxy.imag * sxy.imag
    coh = torch.where(den > 0, num / den.clamp(min=torch.finfo(torch.float64).tiny), 0.0)
    return (coh.clamp(max=1.0).float(), torch.angle(sxy).float(), sxy.to(torch.complex64))
