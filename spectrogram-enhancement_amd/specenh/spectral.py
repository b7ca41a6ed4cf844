"""Time-averaged spectra of device signals: Welch PSD, averaged cross-spectral density and
magnitude-squared coherence, over the whole shot or over blocks of ``navg`` frames (the
coherogram), with ``scipy.signal.welch`` / ``csd`` / ``coherence`` (``average='mean'``)
semantics.

What the interferometer comparison of two chords is read from
(interferometer/crosspowerspec.py in the reference). One fused launch per call
(csrc/spectral_mean.hip through ``torch.ops.specenh.spectral_mean`` ->
``specenh_spectral_mean``): the frames are transformed and summed on the chip, no per-frame
spectrogram is written. Results stay on the device; ``f`` and the group times are float64
numpy arrays computed on the host.

Differences from scipy, each an exception rather than another result: ``nperseg`` must be a
power of two in [64, 4096]; a signal shorter than ``nperseg`` and ``x``, ``y`` of different
shapes raise ``ValueError`` (scipy shrinks ``nperseg`` / zero-pads); ``average='median'``
raises ``NotImplementedError``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .stft import _check_nperseg, _norm_detrend, _norm_scaling, frame_count, frequencies

CHUNK_FRAMES = _lib.SPECTRAL_CHUNK  # groups longer than this take the fp64 workspace path
_BITS = {"pxx": _lib.SPECTRAL_PXX, "pyy": _lib.SPECTRAL_PYY, "pxy": _lib.SPECTRAL_PXY,
         "coh": _lib.SPECTRAL_COH}


def group_count(frames: int, navg) -> int:
    """Averaging groups over ``frames`` frames (specenh_spectral_groups): 1 for ``navg``
    None or <= 0, else ``frames // navg``; ``navg > frames`` is a ``ValueError``."""
    return int(_lib.check(_lib.lib().specenh_spectral_groups(int(frames), int(navg or 0)),
                          "spectral_groups"))


def group_times(length: int, nperseg: int, noverlap: int, fs: float, navg=None) -> np.ndarray:
    """Centre time of every averaging group: the mean of scipy.signal.spectrogram's frame
    times over the group, ``(N/2 + (g navg + (navg - 1)/2) hop) / fs`` (host, float64)."""
    T = frame_count(length, nperseg, noverlap)
    navg = int(navg or 0)
    G = group_count(T, navg)
    n = navg if navg >= 1 else T
    hop = nperseg - noverlap
    return (nperseg / 2 + (np.arange(G, dtype=np.float64) * n + (n - 1) / 2) * hop) / float(fs)


def _signals(x, y):
    for name, v in (("x", x), ("y", y)):
        if v is not None and not isinstance(v, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    if x.dim() not in (1, 2):
        raise ValueError("x must be [batch, length]")
    if y is not None and (y.shape != x.shape or y.device != x.device):
        raise ValueError("x and y must have the same shape and device")
    return x.dim() == 1


def _prep(v):
    if v.dim() == 1:
        v = v.unsqueeze(0)
    if v.dtype != torch.float32:
        v = v.float()
    return v if v.stride(1) == 1 else v.contiguous()


def spectral_estimates(x: torch.Tensor, y: torch.Tensor | None = None, fs: float = 1.0,
                       window="hann", nperseg: int = 256, noverlap=None, detrend="constant",
                       scaling="density", average="mean", navg=None,
                       want=("pxx", "pyy", "pxy", "coh")):
    """Averaged spectra of ``x[B, L]`` (and ``y[B, L]``) on a ROCm device.

    Returns ``(f, t_groups, est)``: ``est[name]`` is ``[B, F, G]`` for every name in ``want``
    — ``pxx``, ``pyy`` (Welch PSDs, float32), ``pxy`` (averaged cross-spectral density,
    complex64), ``coh`` (``|Pxy|^2 / (Pxx Pyy)``, float32; 0/0 is NaN). ``navg`` None or
    <= 0: one group of all frames (scipy's welch / csd / coherence). ``navg >= 1``:
    ``G = T // navg`` groups of ``navg`` consecutive frames, the leftover frames dropped;
    group ``g`` equals scipy on the slice ``x[g navg hop : g navg hop + (navg-1) hop +
    nperseg]``. Without ``y`` only ``pxx`` exists. 1-D input gives ``[F, G]``.
    """
    from .ops import ops, window_key
    if average != "mean":
        if average == "median":
            raise NotImplementedError("average='median' is not supported on the GPU path")
        raise ValueError(f"average must be 'median' or 'mean', got {average}")
    nperseg, noverlap = _check_nperseg(nperseg, noverlap)
    sc, dt = _norm_scaling(scaling), _norm_detrend(detrend)
    squeeze = _signals(x, y)
    want = tuple(want)
    if not want or any(w not in _BITS for w in want):
        raise ValueError(f"want must name some of {tuple(_BITS)}, got {want}")
    if y is None and any(w != "pxx" for w in want):
        raise ValueError("pyy, pxy and coh need a second signal y")
    L = x.shape[-1]
    if L < nperseg:
        raise ValueError(f"signal of {L} samples is shorter than nperseg = {nperseg}")
    navg = int(navg or 0)
    T = (L - nperseg) // (nperseg - noverlap) + 1
    if navg > T:
        raise ValueError(f"navg = {navg} exceeds the number of frames ({T})")
    if x.device.type != "cuda":
        raise RuntimeError("specenh.spectral runs on the GPU only (no CPU fallback); "
                           "move the signals to a ROCm device first")
    mask = 0
    for w in want:
        mask |= _BITS[w]
    outs = ops.spectral_mean(_prep(x), None if y is None else _prep(y), nperseg, noverlap,
                             window_key(window, nperseg), float(fs), sc, dt, navg, mask)
    est = {w: (outs[i][0] if squeeze else outs[i])
           for i, w in enumerate(_BITS) if w in want}
    return frequencies(nperseg, fs), group_times(L, nperseg, noverlap, fs, navg), est


def welch(x: torch.Tensor, fs: float = 1.0, window="hann", nperseg: int = 256, noverlap=None,
          detrend="constant", scaling="density", average="mean"):
    """``scipy.signal.welch``: ``(f, Pxx[B, F])`` float32 on the device."""
    f, _, est = spectral_estimates(x, None, fs, window, nperseg, noverlap, detrend, scaling,
                                   average, None, ("pxx",))
    return f, est["pxx"][..., 0]


def csd(x: torch.Tensor, y: torch.Tensor, fs: float = 1.0, window="hann", nperseg: int = 256,
        noverlap=None, detrend="constant", scaling="density", average="mean"):
    """``scipy.signal.csd``: ``(f, Pxy[B, F])`` complex64 on the device."""
    f, _, est = spectral_estimates(x, y, fs, window, nperseg, noverlap, detrend, scaling,
                                   average, None, ("pxy",))
    return f, est["pxy"][..., 0]


def coherence(x: torch.Tensor, y: torch.Tensor, fs: float = 1.0, window="hann",
              nperseg: int = 256, noverlap=None, detrend="constant"):
    """``scipy.signal.coherence``: ``(f, Cxy[B, F])`` float32 on the device."""
    f, _, est = spectral_estimates(x, y, fs, window, nperseg, noverlap, detrend, "density",
                                   "mean", None, ("coh",))
    return f, est["coh"][..., 0]
