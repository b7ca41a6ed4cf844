"""The two-point (local) wavenumber-frequency spectrum ``S(k, f)`` of device signals (Beall,
Kim & Powers, J. Appl. Phys. 53, 3933, 1982): which way, and how fast, a fluctuation moves
between two channels ``dx`` apart, over the whole shot or over blocks of ``navg`` frames.
``coherence`` and ``csd`` of ``specenh.spectral`` give one mean cross-phase per frequency;
``S(k, f)`` gives the distribution of the per-frame phase, weighted by power. Its ridge is the
dispersion relation ``k(f)``, its width the turbulent broadening a mean phase averages away.

With ``X_t[f]``, ``Y_t[f]`` column ``t`` of ``scipy.signal.spectrogram(s, ..., mode='complex')``
on a group's slice (the groups and slices of ``specenh.spectral.spectral_estimates``), for an
even bin count ``K`` in [4, 256]::

    c      = conj(X_t[f]) * Y_t[f]                 (the sign of scipy.signal.csd)
    theta  = atan2(Im c, Re c);  c == 0 -> theta = 0
    j      = (rint(theta * K / (2 pi)) + K/2) mod K
    w      = o[f] * (|X_t[f]|^2 + |Y_t[f]|^2) / 2       o = 2 for 0 < f < N/2, else 1
    S[b, g, f, j] = (1/T_g) * sum over the group's frames t with j_t[f] == j of w_t[f]

Bin ``j`` is centred on ``theta_j = 2 pi (j - K/2) / K``, so ``k_j = theta_j / dx``;
``theta = +-pi`` both fall in ``j = 0``. ``S.sum(-1)`` is ``(Pxx + Pyy) / 2`` of
``spectral_estimates`` with the same arguments.

Two kernels on one stream (csrc/wavenumber.hip through ``torch.ops.specenh.wavenumber_spectrum``
-> ``specenh_wavenumber_spectrum``): the frames of both signals are transformed once, then a
per-bin histogram is accumulated in fp64 on the chip, without atomics. Results stay on the
device; ``f``, ``k`` and the group times are float64 numpy arrays computed on the host.
``nperseg`` must be a power of two in [64, 4096]; there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .spectral import (_capped, _gpu_only, _groups, _plan_args, _prep, _same, _signals, _spectra,
                       _spectra_groups, group_times)
from .stft import frequencies

# One launch's workspace (the spectra of every frame of both signals) stays under this many
# bytes: the batch is split into several launches, a single shot above it still runs alone.
# Results do not depend on the split.
CSM_WORKSPACE_CAP = _lib.CSM_WORKSPACE_CAP


def _nk(nk):
    if int(nk) != nk or int(nk) % 2 or not _lib.WAVENUMBER_MIN_NK <= nk <= _lib.WAVENUMBER_MAX_NK:
        raise ValueError(f"nk must be even and in [{_lib.WAVENUMBER_MIN_NK}, "
                         f"{_lib.WAVENUMBER_MAX_NK}], got {nk}")
    return int(nk)


def wavenumbers(nk: int, dx: float = 1.0) -> np.ndarray:
    """The bin centres ``2 pi (j - K/2) / (K dx)``, ``fftshift(fftfreq(K)) * 2 pi / dx``
    (host, float64)."""
    return np.fft.fftshift(np.fft.fftfreq(_nk(nk))) * 2 * np.pi / float(dx)


def wavenumber_spectrum(x: torch.Tensor, y: torch.Tensor, fs: float = 1.0, window="hann",
                        nperseg: int = 256, noverlap=None, detrend="constant",
                        scaling="density", navg=None, nk: int = 64, dx: float = 1.0):
    """``S(k, f)`` of ``x[B, L]`` and ``y[B, L]``, two channels ``dx`` apart, on a ROCm device.

    Returns ``(f, k, t_groups, S)``: ``S`` float32 ``[B, G, F, K]``, ``K = nk``. ``navg`` None
    or <= 0: one group of all frames; ``navg >= 1``: ``G = T // navg`` groups of ``navg``
    consecutive frames, the leftover frames dropped. 1-D input drops ``B``.
    """
    from .ops import ops, wavenumber_workspace, window_key
    nperseg, noverlap, sc, dt = _plan_args(nperseg, noverlap, scaling, detrend)
    squeeze = _signals(True, x=x, y=y)
    K = _nk(nk)
    k = wavenumbers(K, dx)
    L = x.shape[-1]
    navg, _, G = _groups(L, nperseg, noverlap, navg)
    _gpu_only(x, "wavenumber")
    xs = _prep(x)
    ys = xs if _same(y, x) else _prep(y)  # a signal given twice is transformed once
    B = xs.shape[0]
    args = (nperseg, noverlap, window_key(window, nperseg), float(fs), sc, dt, navg)
    S = torch.empty((B, G, nperseg // 2 + 1, K), dtype=torch.float32, device=x.device)
    for cut, ws in _capped(B, CSM_WORKSPACE_CAP,
                           lambda: wavenumber_workspace(xs[:1], ys[:1], *args)):
        ops.wavenumber_spectrum_out(cut(xs), cut(ys), *args, K, cut(S), ws)
    return (frequencies(nperseg, fs), k, group_times(L, nperseg, noverlap, fs, navg),
            S[0] if squeeze else S)


def wavenumber_spectrum_from_spectra(X: torch.Tensor, Y: torch.Tensor, navg=None, nk: int = 64):
    """The same histogram from spectra the caller already has: ``X[B, T, F]`` and ``Y`` complex,
    frame-major with the bins contiguous. No scaling and no one-sided doubling is applied:
    ``w = (|X|^2 + |Y|^2) / 2``. Returns ``S`` float32 ``[B, G, F, K]``; ``X[T, F]`` drops
    ``B``."""
    from .ops import ops
    squeeze, T, _, prep = _spectra(True, X=X, Y=Y)
    K = _nk(nk)
    navg = _spectra_groups(T, navg)
    _gpu_only(X, "wavenumber", "spectra")
    S = ops.wavenumber_spectra(prep(X), prep(Y), navg, K)
    return S[0] if squeeze else S


def conditional_spectrum(S: torch.Tensor) -> torch.Tensor:
    """``s(k | f) = S / S.sum(-1)``: the distribution of the wavenumber at each frequency.
    Plain torch on the result, on any device; a row without power (0/0) is NaN."""
    return S / S.sum(-1, keepdim=True)


def dispersion(S: torch.Tensor, k):
    """Beall's first and second moments of the conditional spectrum of ``S[..., F, K]`` on the
    grid ``k[K]``: ``(kbar, sigma_k)``, each ``[..., F]`` float64, with
    ``kbar = sum_j k_j s(k_j | f)`` and ``sigma_k^2 = sum_j (k_j - kbar)^2 s(k_j | f)``. Plain
    torch, on any device; NaN where a row has no power."""
    k = torch.as_tensor(np.asarray(k, dtype=np.float64), device=S.device)
    if S.dim() < 1 or k.dim() != 1 or k.shape[0] != S.shape[-1]:
        raise ValueError("S must be [..., F, K] and k [K]")
    s = conditional_spectrum(S.double())
    kbar = (s * k).sum(-1)
    var = (s * (k - kbar.unsqueeze(-1)) ** 2).sum(-1)
    return kbar, var.clamp_min(0).sqrt()
