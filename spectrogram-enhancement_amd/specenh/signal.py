"""numpy-in / numpy-out ``stft``, ``istft``, ``welch``, ``csd`` and ``coherence`` with
scipy.signal's signatures.

Like the other compat entries (``pipeline_data.specgr``, ``cross.cross_spectrogram``) these
upload, run the tensor path (``specenh.stft.stft`` / ``specenh.stft.istft``: the HIP kernels
of csrc/stft_complex.hip through ``torch.ops.specenh``) and return float64 / complex128
arrays of scipy's shapes. ``welch`` / ``csd`` / ``coherence`` run ``specenh.spectral`` (one
fused launch of csrc/spectral_mean.hip; ``average='mean'`` only). ``cross_spectral_matrix``
(not in scipy) gives ``csd`` / ``coherence`` of every channel pair of an array in one call
(csrc/spectral_matrix.hip), ``array_modes`` the eigendecomposition of those matrices
(csrc/herm_eig.hip), ``array_spectrum`` (not in scipy) the Bartlett, Capon and MUSIC
steered-response spectra of an array (csrc/steered_power.hip), ``bicoherence`` (not in scipy) the squared bicoherence of one to three
signals (csrc/bispectrum.hip), ``wavenumber_spectrum`` (not in scipy) the two-point
wavenumber-frequency spectrum ``S(k, f)`` of two channels (csrc/wavenumber.hip), ``correlate``
the block-averaged lagged cross-correlation of two channels (csrc/correlation.hip; per frame
``scipy.signal.correlate(y_t, x_t)``), ``cwt`` (no longer in scipy) the Morlet continuous
wavelet transform (csrc/filterbank.hip), ``wavelet_coherence`` (not in scipy) the wavelet
coherence and phase of two channels (csrc/filterbank_cross.hip). There is no CPU fallback.

Differences from scipy, each one an exception rather than another result:
``nfft != nperseg``, two-sided spectra, axes other than the defaults, and the ``'even'``,
``'odd'`` and ``'constant'`` boundaries raise ``NotImplementedError``; ``nperseg`` must be a
power of two in [64, 4096]; a signal shorter than ``nperseg`` raises ``ValueError``
(scipy shrinks ``nperseg`` with a warning).
"""
from __future__ import annotations

import numpy as np
import torch

from . import beamform as _beamform
from . import bispectrum as _bispectrum
from . import correlation as _correlation
from . import spectral as _spectral
from . import stft as _stft
from . import wavelet as _wavelet
from . import wavenumber as _wavenumber
from ._lib import FB_MAX_HALF as _FB_MAX_HALF


def _upload(t: torch.Tensor) -> torch.Tensor:
    """To the current ROCm device. Without one the host tensor goes on: the tensor path
    validates the arguments first and then refuses it (no CPU fallback)."""
    return t.cuda() if torch.cuda.is_available() else t


def _leading(a: np.ndarray, keep: int):
    """Flatten the leading (batch) axes: returns (array [B, ...], leading shape)."""
    lead = a.shape[:a.ndim - keep]
    return a.reshape((-1,) + a.shape[a.ndim - keep:]), lead


def stft(x, fs=1.0, window="hann", nperseg=256, noverlap=None, nfft=None, detrend=False,
         return_onesided=True, boundary="zeros", padded=True, axis=-1, scaling="spectrum"):
    """``scipy.signal.stft``: returns ``(f, t, Zxx)``, ``Zxx`` complex128 ``[..., F, T]``."""
    if nfft is not None and int(nfft) != int(nperseg):
        raise NotImplementedError("nfft != nperseg is not supported on the GPU path")
    if not return_onesided:
        raise NotImplementedError("two-sided spectra are not supported on the GPU path")
    x = np.asarray(x)
    if np.iscomplexobj(x):
        raise NotImplementedError("complex input is not supported on the GPU path")
    if x.ndim == 0:
        raise ValueError("x must be at least 1-D")
    if axis not in (-1, x.ndim - 1):
        raise NotImplementedError("only axis=-1 is supported on the GPU path")
    xb, lead = _leading(np.array(x, dtype=np.float32, order="C"), 1)
    xt = torch.from_numpy(xb)
    f, t, Z = _stft.stft(_upload(xt), fs=fs, window=window, nperseg=nperseg,
                         noverlap=noverlap, detrend=detrend, boundary=boundary, padded=padded,
                         scaling=scaling)
    Z = Z.cpu().numpy().astype(np.complex128)
    return f, t, Z.reshape(lead + Z.shape[1:])


def istft(Zxx, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None,
          input_onesided=True, boundary=True, time_axis=-1, freq_axis=-2, scaling="spectrum",
          gain=None):
    """``scipy.signal.istft``: returns ``(t, x)``, ``x`` float64 ``[..., n]``. ``gain`` (not in
    scipy): an optional real mask ``[..., F, T]`` or ``[..., F-1, T]`` multiplied into ``Zxx``
    on the device while the bins are loaded. ``t`` has one entry per output sample (for a batched
    ``Zxx`` scipy 1.15 sizes it by the leading axis instead)."""
    if not input_onesided:
        raise NotImplementedError("two-sided spectra are not supported on the GPU path")
    Zxx = np.asarray(Zxx)
    if Zxx.ndim < 2:
        raise ValueError("Input stft must be at least 2d!")
    if time_axis not in (-1, Zxx.ndim - 1) or freq_axis not in (-2, Zxx.ndim - 2):
        raise NotImplementedError("only time_axis=-1, freq_axis=-2 are supported on the GPU path")
    if nfft is not None and int(nfft) != 2 * (Zxx.shape[-2] - 1):
        raise NotImplementedError("nfft != nperseg is not supported on the GPU path")
    Zb, lead = _leading(np.array(Zxx, dtype=np.complex64, order="C"), 2)
    g = None
    if gain is not None:
        g = np.asarray(gain)
        if g.ndim != Zxx.ndim or g.shape[:-2] != Zxx.shape[:-2]:
            raise ValueError(f"gain must be {Zxx.shape[:-2] + ('F or F-1', Zxx.shape[-1])}, got "
                             f"{g.shape}")
        g = torch.from_numpy(np.array(g, dtype=np.float32, order="C").reshape(
            (-1,) + g.shape[-2:]))
    t, x = _stft.istft(_upload(torch.from_numpy(Zb)), fs=fs, window=window,
                       nperseg=nperseg, noverlap=noverlap, boundary=boundary, scaling=scaling,
                       gain=g)
    x = x.cpu().numpy().astype(np.float64)
    return t, x.reshape(lead + x.shape[1:])


def _averaged(which, x, y, fs, window, nperseg, noverlap, nfft, detrend, return_onesided,
              scaling, axis, average):
    nperseg = 256 if nperseg is None else int(nperseg)
    if nfft is not None and int(nfft) != nperseg:
        raise NotImplementedError("nfft != nperseg is not supported on the GPU path")
    if not return_onesided:
        raise NotImplementedError("two-sided spectra are not supported on the GPU path")
    if average != "mean":
        if average == "median":
            raise NotImplementedError("average='median' is not supported on the GPU path")
        raise ValueError(f"average must be 'median' or 'mean', got {average}")
    arrs = [np.asarray(v) for v in (x, y) if v is not None]
    for a in arrs:
        if np.iscomplexobj(a):
            raise NotImplementedError("complex input is not supported on the GPU path")
        if a.ndim == 0:
            raise ValueError("x must be at least 1-D")
        if axis not in (-1, a.ndim - 1):
            raise NotImplementedError("only axis=-1 is supported on the GPU path")
    if len(arrs) == 2 and arrs[0].shape != arrs[1].shape:
        raise ValueError("x and y must have the same shape (scipy would broadcast / zero-pad)")
    lead = arrs[0].shape[:-1]
    ts = [_upload(torch.from_numpy(_leading(np.array(a, dtype=np.float32, order="C"), 1)[0]))
          for a in arrs]
    f, _, est = _spectral.spectral_estimates(
        ts[0], ts[1] if len(ts) == 2 else None, fs=fs, window=window, nperseg=nperseg,
        noverlap=noverlap, detrend=detrend, scaling=scaling, want=(which,))
    P = est[which][..., 0].cpu().numpy()
    P = P.astype(np.complex128 if which == "pxy" else np.float64)
    return f, P.reshape(lead + P.shape[1:])


def welch(x, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, detrend="constant",
          return_onesided=True, scaling="density", axis=-1, average="mean"):
    """``scipy.signal.welch``: returns ``(f, Pxx)``, ``Pxx`` float64 ``[..., F]``."""
    return _averaged("pxx", x, None, fs, window, nperseg, noverlap, nfft, detrend,
                     return_onesided, scaling, axis, average)


def csd(x, y, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None, detrend="constant",
        return_onesided=True, scaling="density", axis=-1, average="mean"):
    """``scipy.signal.csd``: returns ``(f, Pxy)``, ``Pxy`` complex128 ``[..., F]``."""
    return _averaged("pxy", x, y, fs, window, nperseg, noverlap, nfft, detrend, return_onesided,
                     scaling, axis, average)


def coherence(x, y, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None,
              detrend="constant", axis=-1):
    """``scipy.signal.coherence``: returns ``(f, Cxy)``, ``Cxy`` float64 ``[..., F]``."""
    return _averaged("coh", x, y, fs, window, nperseg, noverlap, nfft, detrend, True, "density",
                     axis, "mean")


def cross_spectral_matrix(x, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None,
                          detrend="constant", return_onesided=True, scaling="density", axis=-1,
                          average="mean", navg=None, want=("csm", "coh")):
    """The cross-spectral matrix of a channel array ``x[..., C, L]`` (not in scipy: one call of
    ``specenh.spectral.cross_spectral_matrix`` instead of ``scipy.signal.csd`` per channel
    pair). Returns ``(f, t_groups, est)``: ``est["csm"]`` complex128 and ``est["coh"]``
    float64, ``[..., F, G, C, C]``; the leading axes are flattened into the batch and
    restored."""
    nperseg = 256 if nperseg is None else int(nperseg)
    if nfft is not None and int(nfft) != nperseg:
        raise NotImplementedError("nfft != nperseg is not supported on the GPU path")
    if not return_onesided:
        raise NotImplementedError("two-sided spectra are not supported on the GPU path")
    if average != "mean":
        if average == "median":
            raise NotImplementedError("average='median' is not supported on the GPU path")
        raise ValueError(f"average must be 'median' or 'mean', got {average}")
    a = np.asarray(x)
    if np.iscomplexobj(a):
        raise NotImplementedError("complex input is not supported on the GPU path")
    if a.ndim < 2:
        raise ValueError("x must be at least 2-D: [..., channels, length]")
    if axis not in (-1, a.ndim - 1):
        raise NotImplementedError("only axis=-1 is supported on the GPU path")
    xb, lead = _leading(np.array(a, dtype=np.float32, order="C"), 2)
    f, t, est = _spectral.cross_spectral_matrix(
        _upload(torch.from_numpy(xb)), fs=fs, window=window, nperseg=nperseg, noverlap=noverlap,
        detrend=detrend, scaling=scaling, navg=navg, want=want)
    out = {}
    for name, v in est.items():
        v = v.cpu().numpy().astype(np.complex128 if name == "csm" else np.float64)
        out[name] = v.reshape(lead + v.shape[1:])
    return f, t, out


def array_modes(x, k=1, fs=1.0, window="hann", nperseg=None, noverlap=None, nfft=None,
                detrend="constant", return_onesided=True, scaling="density", axis=-1,
                average="mean", navg=None):
    """Mode decomposition of a channel array ``x[..., C, L]`` (not in scipy): one call of
    ``specenh.spectral.array_modes``, the eigendecomposition of the cross-spectral matrix of
    every frequency and averaging group (csrc/spectral_matrix.hip, csrc/herm_eig.hip).
    Returns ``(f, t_groups, est)``: ``est["power"]`` float64 ``[..., F, G, C]``,
    ``est["modes"]`` complex128 ``[..., F, G, k, C]`` and ``est["fraction"]`` float64
    ``[..., F, G, k]``; the leading axes are flattened into the batch and restored."""
    nperseg = 256 if nperseg is None else int(nperseg)
    if nfft is not None and int(nfft) != nperseg:
        raise NotImplementedError("nfft != nperseg is not supported on the GPU path")
    if not return_onesided:
        raise NotImplementedError("two-sided spectra are not supported on the GPU path")
    if average != "mean":
        if average == "median":
            raise NotImplementedError("average='median' is not supported on the GPU path")
        raise ValueError(f"average must be 'median' or 'mean', got {average}")
    a = np.asarray(x)
    if np.iscomplexobj(a):
        raise NotImplementedError("complex input is not supported on the GPU path")
    if a.ndim < 2:
        raise ValueError("x must be at least 2-D: [..., channels, length]")
    if axis not in (-1, a.ndim - 1):
        raise NotImplementedError("only axis=-1 is supported on the GPU path")
    xb, lead = _leading(np.array(a, dtype=np.float32, order="C"), 2)
    f, t, est = _spectral.array_modes(
        _upload(torch.from_numpy(xb)), k=k, fs=fs, window=window, nperseg=nperseg,
        noverlap=noverlap, detrend=detrend, scaling=scaling, navg=navg)
    out = {}
    for name, v in est.items():
        v = v.cpu().numpy().astype(np.complex128 if name == "modes" else np.float64)
        out[name] = v.reshape(lead + v.shape[1:])
    return f, t, out


def array_spectrum(x, A, method="bartlett", nsources=1, loading=1e-2, fs=1.0, window="hann",
                   nperseg=None, noverlap=None, nfft=None, detrend="constant",
                   return_onesided=True, scaling="density", axis=-1, average="mean", navg=None):
    """The steered-response spectrum of a channel array ``x[..., C, L]`` on the steering vectors
    ``A[K, C]`` or ``A[F, K, C]`` (complex; not in scipy): one call of
    ``specenh.beamform.array_spectrum``, the Bartlett, Capon or MUSIC estimator of every
    frequency and averaging group (csrc/steered_power.hip). Returns ``(f, t_groups, P)``, ``P``
    float64 ``[..., F, G, K]``; the leading axes are flattened into the batch and restored."""
    nperseg = 256 if nperseg is None else int(nperseg)
    if nfft is not None and int(nfft) != nperseg:
        raise NotImplementedError("nfft != nperseg is not supported on the GPU path")
    if not return_onesided:
        raise NotImplementedError("two-sided spectra are not supported on the GPU path")
    if average != "mean":
        if average == "median":
            raise NotImplementedError("average='median' is not supported on the GPU path")
        raise ValueError(f"average must be 'median' or 'mean', got {average}")
    a = np.asarray(x)
    if np.iscomplexobj(a):
        raise NotImplementedError("complex input is not supported on the GPU path")
    if a.ndim < 2:
        raise ValueError("x must be at least 2-D: [..., channels, length]")
    if axis not in (-1, a.ndim - 1):
        raise NotImplementedError("only axis=-1 is supported on the GPU path")
    if not isinstance(A, torch.Tensor):
        A = np.asarray(A)
        if not np.iscomplexobj(A):
            raise ValueError("A must be complex [K, C] or [F, K, C]")
        A = torch.from_numpy(np.array(A, dtype=np.complex64, order="C"))
    xb, lead = _leading(np.array(a, dtype=np.float32, order="C"), 2)
    f, t, P = _beamform.array_spectrum(
        _upload(torch.from_numpy(xb)), _upload(A), method=method, nsources=nsources,
        loading=loading, fs=fs, window=window, nperseg=nperseg, noverlap=noverlap,
        detrend=detrend, scaling=scaling, navg=navg)
    P = P.cpu().numpy().astype(np.float64)
    return f, t, P.reshape(lead + P.shape[1:])


def bicoherence(x, y=None, z=None, fs=1.0, window="hann", nperseg=None, noverlap=None,
                detrend="constant", nbins=None):
    """The squared bicoherence ``|<X_k Y_l conj(Z_{k+l})>|^2 / (<|X_k Y_l|^2> <|Z_{k+l}|^2>)``
    of the whole signal (not in scipy: one call of ``specenh.bispectrum.bicoherence``,
    csrc/bispectrum.hip); ``y`` and ``z`` default to ``x``. Returns ``(f[:K], b2)``, ``b2``
    float64 ``[..., K, K]`` with ``K = nbins`` (default ``nperseg // 2 + 1``), 0 where
    ``k + l > nperseg // 2``; the leading axes are flattened into the batch and restored."""
    nperseg = 256 if nperseg is None else int(nperseg)
    arrs = [np.asarray(v) for v in (x, y, z) if v is not None]
    for a in arrs:
        if np.iscomplexobj(a):
            raise NotImplementedError("complex input is not supported on the GPU path")
        if a.ndim == 0:
            raise ValueError("x must be at least 1-D")
        if a.shape != arrs[0].shape:
            raise ValueError("x, y and z must have the same shape")
    lead = arrs[0].shape[:-1]
    ts = [None if v is None else
          _upload(torch.from_numpy(_leading(np.array(v, dtype=np.float32, order="C"), 1)[0]))
          for v in (x, y, z)]
    f, b2 = _bispectrum.bicoherence(ts[0], ts[1], ts[2], fs=fs, window=window, nperseg=nperseg,
                                    noverlap=noverlap, detrend=detrend, nbins=nbins)
    b2 = b2.cpu().numpy().astype(np.float64)
    return f, b2.reshape(lead + b2.shape[1:])


def wavenumber_spectrum(x, y, fs=1.0, window="hann", nperseg=None, noverlap=None,
                        detrend="constant", scaling="density", navg=None, nk=64, dx=1.0):
    """The two-point wavenumber-frequency spectrum ``S(k, f)`` of two channels ``dx`` apart
    (Beall, Kim & Powers 1982; not in scipy: one call of
    ``specenh.wavenumber.wavenumber_spectrum``, csrc/wavenumber.hip): the power-weighted
    histogram of the per-frame cross-phase of ``y`` relative to ``x`` over ``nk`` centred bins.
    Returns ``(f, k, t_groups, S)``, ``S`` float64 ``[..., G, F, nk]``; the leading axes are
    flattened into the batch and restored."""
    nperseg = 256 if nperseg is None else int(nperseg)
    arrs = [np.asarray(v) for v in (x, y)]
    for a in arrs:
        if np.iscomplexobj(a):
            raise NotImplementedError("complex input is not supported on the GPU path")
        if a.ndim == 0:
            raise ValueError("x must be at least 1-D")
        if a.shape != arrs[0].shape:
            raise ValueError("x and y must have the same shape")
    lead = arrs[0].shape[:-1]
    ts = [_upload(torch.from_numpy(_leading(np.array(a, dtype=np.float32, order="C"), 1)[0]))
          for a in arrs]
    f, k, t, S = _wavenumber.wavenumber_spectrum(
        ts[0], ts[1], fs=fs, window=window, nperseg=nperseg, noverlap=noverlap, detrend=detrend,
        scaling=scaling, navg=navg, nk=nk, dx=dx)
    S = S.cpu().numpy().astype(np.float64)
    return f, k, t, S.reshape(lead + S.shape[1:])


def correlate(x, y, window="boxcar", nperseg=None, noverlap=None, detrend="constant", navg=None,
              maxlag=None, normalize="coeff", unbiased=False, fs=1.0):
    """The block-averaged lagged cross-correlation of two channels (one call of
    ``specenh.correlation.correlate``, csrc/correlation.hip): per frame
    ``scipy.signal.correlate(y_t, x_t, 'full')[N - 1 + m]`` of the detrended, windowed frames,
    averaged over each group, as the coefficient (``normalize="coeff"``) or raw. A positive lag
    means ``y`` lags ``x``. Returns ``(lags, t_groups, R)``, ``lags`` in seconds, ``R`` float64
    ``[..., G, 2 maxlag + 1]``; the leading axes are flattened into the batch and restored."""
    nperseg = 256 if nperseg is None else int(nperseg)
    arrs = [np.asarray(v) for v in (x, y)]
    for a in arrs:
        if np.iscomplexobj(a):
            raise NotImplementedError("complex input is not supported on the GPU path")
        if a.ndim == 0:
            raise ValueError("x must be at least 1-D")
        if a.shape != arrs[0].shape:
            raise ValueError("x and y must have the same shape")
    lead = arrs[0].shape[:-1]
    tx = _upload(torch.from_numpy(_leading(np.array(arrs[0], dtype=np.float32, order="C"), 1)[0]))
    ty = tx if y is x else _upload(
        torch.from_numpy(_leading(np.array(arrs[1], dtype=np.float32, order="C"), 1)[0]))
    lags, t, R = _correlation.correlate(
        tx, ty, window=window, nperseg=nperseg, noverlap=noverlap, detrend=detrend, navg=navg,
        maxlag=maxlag, normalize=normalize, unbiased=unbiased, fs=fs)
    R = R.cpu().numpy().astype(np.float64)
    return lags, t, R.reshape(lead + R.shape[1:])


def _cwt_scales(fs, freqs, fmin, fmax, voices_per_octave, w0, support):
    """The Morlet scales (samples) of ``freqs``, or the default geometric ladder of ``cwt``."""
    if freqs is not None:
        return _wavelet.frequency_to_scale(freqs, fs, w0)
    fmax = fs / 4.0 if fmax is None else fmax
    if fmin is None:
        fmin = float(_wavelet.scale_to_frequency(_FB_MAX_HALF / support, fs, w0)[0])
    scales = _wavelet.morlet_scales(fmin, fmax, fs, voices_per_octave, w0)
    while np.ceil(support * scales[-1]) > _FB_MAX_HALF:  # the step past fmin
        scales = scales[:-1]
    return scales


def cwt(x, fs=1.0, freqs=None, fmin=None, fmax=None, voices_per_octave=16, hop=1, w0=6.0,
        support=4.0, nfft=None):
    """The Morlet continuous wavelet transform (one call of ``specenh.wavelet.cwt``,
    csrc/filterbank.hip; not in scipy since ``scipy.signal.cwt`` was removed): Torrence &
    Compo's ``W_n(s)`` with ``dt = 1`` at the scales of ``freqs`` (Hz), or, ``freqs`` None, at
    ``wavelet.morlet_scales(fmin, fmax, fs, voices_per_octave)`` with ``fmin`` defaulting to
    the lowest frequency whose wavelet has a half length of 1024 samples and ``fmax`` to
    ``fs / 4``. Returns ``(freqs, t, W)``: ``freqs`` float64 ``[S]``
    (``wavelet.scale_to_frequency``), ``t = arange(To) * hop / fs`` and ``W`` complex128
    ``[..., S, To]``; the leading axes are flattened into the batch and restored."""
    a = np.asarray(x)
    if np.iscomplexobj(a):
        raise NotImplementedError("complex input is not supported on the GPU path")
    if a.ndim == 0:
        raise ValueError("x must be at least 1-D")
    scales = _cwt_scales(fs, freqs, fmin, fmax, voices_per_octave, w0, support)
    flat, lead = _leading(np.array(a, dtype=np.float32, order="C"), 1)
    W = _wavelet.cwt(_upload(torch.from_numpy(flat)), scales, hop=hop, w0=w0, support=support,
                     nfft=nfft)
    W = W.cpu().numpy().astype(np.complex128)
    t = np.arange(W.shape[-1], dtype=np.float64) * hop / float(fs)
    return _wavelet.scale_to_frequency(scales, fs, w0), t, W.reshape(lead + W.shape[1:])


def wavelet_coherence(x, y, fs=1.0, freqs=None, fmin=None, fmax=None, voices_per_octave=16,
                      hop=1, smooth=None, w0=6.0, support=4.0, nfft=None):
    """Wavelet coherence and phase of two channels (one call of
    ``specenh.wavelet.wavelet_coherence``, csrc/filterbank_cross.hip; not in scipy), at the
    scales ``cwt`` would use for the same ``freqs`` / ``fmin`` / ``fmax`` /
    ``voices_per_octave``. Returns ``(freqs, t, coh, phase)``: ``freqs`` float64 ``[S]``,
    ``t = (arange(To) + 0.5) * hop / fs`` the centres of the ``To = length // hop`` windows,
    ``coh`` in [0, 1] and ``phase = angle(conj(Wx) Wy)`` float64 ``[..., S, To]`` (negative
    where ``y`` lags ``x``). ``x`` and ``y`` broadcast on their leading axes; ``smooth`` as in
    ``specenh.wavelet.wavelet_coherence``."""
    a, b = np.asarray(x), np.asarray(y)
    if np.iscomplexobj(a) or np.iscomplexobj(b):
        raise NotImplementedError("complex input is not supported on the GPU path")
    if a.ndim == 0 or b.ndim == 0:
        raise ValueError("x and y must be at least 1-D")
    scales = _cwt_scales(fs, freqs, fmin, fmax, voices_per_octave, w0, support)
    tx = _upload(torch.from_numpy(np.array(a, dtype=np.float32, order="C")))
    ty = tx if y is x else _upload(torch.from_numpy(np.array(b, dtype=np.float32, order="C")))
    coh, phase, _ = _wavelet.wavelet_coherence(tx, ty, scales, hop=hop, smooth=smooth, w0=w0,
                                               support=support, nfft=nfft)
    t = (np.arange(coh.shape[-1], dtype=np.float64) + 0.5) * hop / float(fs)
    return (_wavelet.scale_to_frequency(scales, fs, w0), t,
            coh.cpu().numpy().astype(np.float64), phase.cpu().numpy().astype(np.float64))
