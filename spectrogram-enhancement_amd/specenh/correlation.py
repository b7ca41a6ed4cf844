"""The block-averaged lagged cross-correlation of two device signals, and what is read off it:
the time delay ``tau(t)`` at its peak (``dx / tau`` is the velocity between two channels ``dx``
apart: cross-correlation time-delay estimation) and the correlation time from the width of the
auto-correlation. ``csd`` and ``wavenumber_spectrum`` answer "which phase at which frequency";
the correlation function answers "which delay, broadband".

Frames, groups, detrend and window are those of ``specenh.spectral.spectral_estimates``. With
``x_t``, ``y_t`` the detrended, windowed frames of ``N = nperseg`` samples and a maximum lag
``0 <= M <= N - 1``::

    r_t[m]       = sum_n x_t[n] * y_t[n + m]      m = -M .. M, terms outside [0, N) are zero
                 = scipy.signal.correlate(y_t, x_t, 'full')[N - 1 + m]
    R[b, g, m]   = (1/T_g) * sum over the group's frames t of r_t[m]
    Ex[b, g]     = (1/T_g) * sum_t sum_n x_t[n]^2         (Ey likewise)
    rho[b, g, m] = R[b, g, m] / sqrt(Ex * Ey),  defined as 0 where Ex * Ey == 0

``y[n] = x[n - d]`` peaks at ``m = +d``: a positive lag means ``y`` lags ``x`` (the CSD phase is
likewise that of ``y`` relative to ``x``). ``R`` is in signal units squared, ``rho`` is
dimensionless with ``|rho| <= 1``; lag ``m`` is at index ``m + M``. This is the linear
correlation of zero-padded frames, not the circular one the inverse transform of an averaged
CSD would give.

One fused pass (csrc/correlation.hip through ``torch.ops.specenh.correlation`` ->
``specenh_correlation``): the cross-spectra of a group's padded frames are summed on the chip
and inverted once per group; no per-frame spectrum reaches memory. Results stay on the device;
the lags and group times are float64 numpy arrays computed on the host. ``nperseg`` must be a
power of two in [64, 2048] (4096 is not supported: the padded transform would be 8192 points);
there is no CPU fallback.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from .spectral import (_capped, _gpu_only, _groups, _plan_args, _prep, _same, _signals,
                       group_times)
from .stft import get_window

# One launch's workspace (a record per chunk of 32 frames when a group is longer than a chunk)
# stays under this many bytes: the batch is split into several launches, a single shot above it
# still runs alone. Results do not depend on the split.
CSM_WORKSPACE_CAP = _lib.CSM_WORKSPACE_CAP

_MODES = {"coeff": _lib.CORR_COEFF, "raw": _lib.CORR_RAW, None: _lib.CORR_RAW,
          False: _lib.CORR_RAW}


def _maxlag(maxlag, nperseg):
    M = nperseg - 1 if maxlag is None else maxlag
    if int(M) != M or not 0 <= M < nperseg:
        raise ValueError(f"maxlag must be an integer in [0, nperseg - 1] = [0, {nperseg - 1}], "
                         f"got {maxlag}")
    return int(M)


def correlation_lags(maxlag: int, fs: float = 1.0) -> np.ndarray:
    """The lags ``-M .. M`` in seconds, ``arange(-M, M + 1) / fs`` (host, float64): those of
    ``scipy.signal.correlation_lags(N, N)`` within ``|m| <= M``."""
    if int(maxlag) != maxlag or maxlag < 0:
        raise ValueError(f"maxlag must be a non-negative integer, got {maxlag}")
    return np.arange(-int(maxlag), int(maxlag) + 1, dtype=np.float64) / float(fs)


def window_lag_product(window, nperseg: int, maxlag=None) -> np.ndarray:
    """``c[m] = sum_n w[n] w[n + m]``, ``m = -M .. M`` (host, float64): the correlation of the
    window with itself, ``N - |m|`` for boxcar. It is what a frame pair of unit covariance
    contributes to ``R[m]``, the divisor of ``unbiased=True``."""
    w = np.asarray(get_window(window, int(nperseg)), dtype=np.float64)
    M = _maxlag(maxlag, int(nperseg))
    N = w.shape[0]
    pos = np.array([np.dot(w[:N - m], w[m:]) for m in range(M + 1)])
    return np.concatenate([pos[:0:-1], pos])


def correlate(x: torch.Tensor, y: torch.Tensor, window="boxcar", nperseg: int = 256,
              noverlap=None, detrend="constant", navg=None, maxlag=None, normalize="coeff",
              unbiased: bool = False, fs: float = 1.0):
    """The block-averaged cross-correlation of ``x[B, L]`` and ``y[B, L]`` on a ROCm device.

    Returns ``(lags, t_groups, R)``: ``lags`` in seconds (``correlation_lags(M, fs)``), ``R``
    float32 ``[B, G, 2 M + 1]`` — the coefficient ``rho`` with ``normalize="coeff"``, the mean
    raw correlation with ``normalize="raw"``. ``maxlag`` None: ``M = nperseg - 1``. ``navg`` None
    or <= 0: one group of all frames; ``navg >= 1``: ``G = T // navg`` groups of ``navg``
    consecutive frames, the leftover frames dropped. 1-D input drops ``B``.

    ``unbiased=True`` divides lag ``m`` by the window's own lag product
    ``c[m] = sum_n w[n] w[n + m]`` (``N - |m|`` for boxcar; ``window_lag_product``) — by
    ``c[m] / c[0]`` for the coefficient, so that lag 0 stays 1 — in plain torch on the result. A
    lag at which the product is 0 (the ends of a window that starts at 0) is then Inf or NaN.
    """
    from .ops import ops, correlation_workspace, window_key
    nperseg, noverlap, _, dt = _plan_args(nperseg, noverlap, "density", detrend)
    if nperseg > _lib.CORR_MAX_NPERSEG:
        raise NotImplementedError(
            f"correlate: nperseg = {nperseg} is not supported (the padded transform would be "
            f"{2 * nperseg} points); nperseg must be a power of two in [64, 2048]")
    try:
        mode = _MODES[normalize]
    except (KeyError, TypeError):
        raise ValueError(f"normalize must be 'coeff' or 'raw', got {normalize!r}") from None
    squeeze = _signals(True, x=x, y=y)
    M = _maxlag(maxlag, nperseg)
    L = x.shape[-1]
    navg, _, G = _groups(L, nperseg, noverlap, navg)
    div = None
    if unbiased:
        c = window_lag_product(window, nperseg, M)
        div = c / c[M] if mode == _lib.CORR_COEFF else c
    _gpu_only(x, "correlation")
    xs = _prep(x)
    ys = xs if _same(y, x) else _prep(y)  # a signal given twice is loaded and transformed once
    B = xs.shape[0]
    args = (nperseg, noverlap, window_key(window, nperseg), float(fs), 0, dt, navg, M)
    R = torch.empty((B, G, 2 * M + 1), dtype=torch.float32, device=x.device)
    # a group of one chunk needs no workspace: then the batch is one launch
    for cut, ws in _capped(B, CSM_WORKSPACE_CAP,
                           lambda: correlation_workspace(xs[:1], ys[:1], *args)):
        ops.correlation_out(cut(xs), cut(ys), *args, mode, cut(R), None, ws)
    if div is not None:
        R = (R.double() / torch.as_tensor(div, device=R.device)).float()
    return (correlation_lags(M, fs), group_times(L, nperseg, noverlap, fs, navg),
            R[0] if squeeze else R)


def autocorrelate(x: torch.Tensor, **kw):
    """``correlate(x, x, ...)``: the signal is loaded and transformed once."""
    return correlate(x, x, **kw)


def time_delay(R: torch.Tensor, lags):
    """The delay at the peak of ``R[..., G, 2 M + 1]`` on the grid ``lags[2 M + 1]``:
    ``(tau, peak)``, each ``[..., G]`` float64. The argmax over the lags, refined by the
    three-point parabola through the peak and its two neighbours; a peak on the first or last
    lag (or a flat top) is returned unrefined. Plain torch, on any device."""
    lags = torch.as_tensor(np.asarray(lags, dtype=np.float64), device=R.device)
    if R.dim() < 1 or lags.dim() != 1 or lags.shape[0] != R.shape[-1]:
        raise ValueError("R must be [..., 2 M + 1] and lags [2 M + 1]")
    r = R.double()
    n = r.shape[-1]
    i = r.argmax(-1, keepdim=True)
    y0 = r.gather(-1, i)
    ym = r.gather(-1, (i - 1).clamp_min(0))
    yp = r.gather(-1, (i + 1).clamp_max(n - 1))
    den = ym - 2 * y0 + yp
    inner = (i > 0) & (i < n - 1) & (den != 0)
    delta = torch.where(inner, 0.5 * (ym - yp) / torch.where(den != 0, den, torch.ones_like(den)),
                        torch.zeros_like(den))
    step = lags[1] - lags[0] if n > 1 else lags.new_zeros(())
    tau = lags[i] + delta * step
    peak = y0 - 0.25 * (ym - yp) * delta
    return tau.squeeze(-1), peak.squeeze(-1)


def correlation_time(R: torch.Tensor, lags):
    """The correlation time of an auto-correlation ``R[..., G, 2 M + 1]``: the first positive lag
    at which ``R[m] / R[0]`` falls below ``1/e``, linearly interpolated between that lag and the
    one before; NaN if it never does (or if ``R[0]`` is 0). ``[..., G]`` float64, plain torch, on
    any device."""
    lags = torch.as_tensor(np.asarray(lags, dtype=np.float64), device=R.device)
    if R.dim() < 1 or lags.dim() != 1 or lags.shape[0] != R.shape[-1] or not R.shape[-1] % 2:
        raise ValueError("R must be [..., 2 M + 1] and lags [2 M + 1]")
    M = R.shape[-1] // 2
    r = R.double()[..., M:]
    rho = r / r[..., :1]
    t = lags[M:]
    thr = 1.0 / math.e
    below = rho < thr
    first = (below.cumsum(-1) == 0).sum(-1, keepdim=True)  # leading lags not below: >= 1
    found = (first <= M) & (first >= 1)
    j = first.clamp(1, max(M, 1)) if M else first.clamp(0, 0)
    a, b = rho.gather(-1, (j - 1).clamp_min(0)), rho.gather(-1, j)
    frac = (a - thr) / torch.where(a != b, a - b, torch.ones_like(a))
    tc = t[(j - 1).clamp_min(0)] + frac * (t[j] - t[(j - 1).clamp_min(0)])
    nan = torch.full_like(tc, float("nan"))
    return torch.where(found, tc, nan).squeeze(-1)
