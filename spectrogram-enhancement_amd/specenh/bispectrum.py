"""Bispectrum and squared bicoherence of device signals (Kim & Powers 1979): whether three
frequencies ``f1 + f2 = f3`` are phase-locked, over the whole shot or over blocks of ``navg``
frames. What the second-order estimators of ``specenh.spectral`` cannot say: a mode and its
harmonics, two modes beating, turbulence feeding a zonal flow.

With ``X_t[k]`` column ``t`` of ``scipy.signal.spectrogram(s, ..., mode='complex')`` on a
group's slice (the groups and slices of ``specenh.spectral.spectral_estimates``), for
``0 <= k, l < K`` and ``k + l <= N/2``::

    B[k, l]  = mean_t X_t[k] Y_t[l] conj(Z_t[k + l])          bispectrum, complex
    b2[k, l] = |B[k, l]|^2 / (mean_t |X_t[k] Y_t[l]|^2  mean_t |Z_t[k + l]|^2)   in [0, 1]

and 0 in both where ``k + l > N/2``. ``y`` and ``z`` default to ``x`` (the auto-bicoherence,
symmetric in ``(k, l)`` bit for bit); with them it is the cross-bicoherence, for example
density x density -> potential.

Two kernels on one stream (csrc/bispectrum.hip through ``torch.ops.specenh.bispectrum`` ->
``specenh_bispectrum``): every distinct signal's frames are transformed once, then the triple
products of every ``(k, l)`` tile are summed on the chip. Results stay on the device; ``f`` and
the group times are float64 numpy arrays computed on the host. ``nperseg`` must be a power of
two in [64, 4096]; there is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib
from .spectral import (_capped, _gpu_only, _groups, _plan_args, _prep, _same, _signals, _spectra,
                       _spectra_groups, group_times)
from .stft import frequencies

_BITS = {"bispec": _lib.BISPEC_BISPEC, "bicoh": _lib.BISPEC_BICOH}
_DTYPES = {"bispec": torch.complex64, "bicoh": torch.float32}
# One launch's workspace (the spectra of every frame of every distinct signal) stays under
# this many bytes: the batch is split into several launches, a single shot above it still
# runs alone. Results do not depend on the split.
CSM_WORKSPACE_CAP = _lib.CSM_WORKSPACE_CAP


def _want(want):
    want = tuple(want)
    if not want or any(w not in _BITS for w in want):
        raise ValueError(f"want must name some of {tuple(_BITS)}, got {want}")
    return want


def _nbins(nbins, F):
    K = F if nbins is None else int(nbins)
    if not 1 <= K <= F:
        raise ValueError(f"nbins must be in [1, {F}], got {nbins}")
    return K


def bispectrum(x: torch.Tensor, y: torch.Tensor | None = None, z: torch.Tensor | None = None,
               fs: float = 1.0, window="hann", nperseg: int = 256, noverlap=None,
               detrend="constant", scaling="density", navg=None, nbins=None,
               want=("bispec", "bicoh")):
    """Bispectrum and squared bicoherence of ``x[B, L]`` (and ``y``, ``z``) on a ROCm device.

    Returns ``(f[:K], t_groups, est)``: ``est["bispec"]`` complex64 and ``est["bicoh"]``
    float32 (0/0 is NaN), ``[B, G, K, K]`` for the names in ``want``; ``K = nbins`` (default
    ``nperseg // 2 + 1``) keeps the corner ``k, l < K`` of the plane, the same values. ``navg``
    None or <= 0: one group of all frames; ``navg >= 1``: ``G = T // navg`` groups of ``navg``
    consecutive frames, the leftover frames dropped. 1-D input drops ``B``.
    """
    from .ops import ops, bispectrum_workspace, window_key
    nperseg, noverlap, sc, dt = _plan_args(nperseg, noverlap, scaling, detrend)
    squeeze = _signals(x=x, y=y, z=z)
    want = _want(want)
    K = _nbins(nbins, nperseg // 2 + 1)
    L = x.shape[-1]
    navg, _, G = _groups(L, nperseg, noverlap, navg)
    _gpu_only(x, "bispectrum")
    # a signal given twice is transformed once: the same tensor stays the same tensor
    xs = _prep(x)
    ys = xs if y is None or _same(y, x) else _prep(y)
    zs = xs if z is None or _same(z, x) else (ys if y is not None and _same(z, y) else _prep(z))
    ys, zs = (None if ys is xs else ys), (None if zs is xs else zs)
    B = xs.shape[0]
    args = (nperseg, noverlap, window_key(window, nperseg), float(fs), sc, dt, navg)
    outs = [torch.empty((B, G, K, K), dtype=_DTYPES[w], device=x.device) if w in want else None
            for w in _BITS]

    def one_shot():
        return bispectrum_workspace(*(None if v is None else v[:1] for v in (xs, ys, zs)), *args)

    for cut, ws in _capped(B, CSM_WORKSPACE_CAP, one_shot):
        ops.bispectrum_out(cut(xs), cut(ys), cut(zs), *args, K, cut(outs[0]), cut(outs[1]), ws)
    est = {w: (o[0] if squeeze else o) for w, o in zip(_BITS, outs) if o is not None}
    return frequencies(nperseg, fs)[:K], group_times(L, nperseg, noverlap, fs, navg), est


def bicoherence(x: torch.Tensor, y: torch.Tensor | None = None, z: torch.Tensor | None = None,
                fs: float = 1.0, window="hann", nperseg: int = 256, noverlap=None,
                detrend="constant", nbins=None):
    """The squared bicoherence of the whole shot: ``(f[:K], b2[B, K, K])`` float32 on the
    device (``[K, K]`` for 1-D input)."""
    f, _, est = bispectrum(x, y, z, fs, window, nperseg, noverlap, detrend, "density", None,
                           nbins, ("bicoh",))
    return f, est["bicoh"][..., 0, :, :]


def bispectrum_from_spectra(X: torch.Tensor, Y: torch.Tensor | None = None,
                            Z: torch.Tensor | None = None, navg=None, nbins=None,
                            want=("bispec", "bicoh")):
    """The same estimators from spectra the caller already has: ``X[B, T, F]`` complex (and
    ``Y``, ``Z``), frame-major with the bins contiguous, ``F = N/2 + 1`` (the domain is
    ``k + l <= F - 1``). No scaling is applied. Returns ``est`` as ``bispectrum`` does,
    ``[B, G, K, K]``; ``X[T, F]`` drops ``B``."""
    from .ops import ops
    squeeze, T, F, prep = _spectra(X=X, Y=Y, Z=Z)
    want = _want(want)
    K = _nbins(nbins, F)
    navg = _spectra_groups(T, navg)
    _gpu_only(X, "bispectrum", "spectra")
    Xs = prep(X)
    Ys = None if Y is None or _same(Y, X) else prep(Y)
    Zs = None if Z is None or _same(Z, X) else prep(Z)
    mask = 0
    for w in want:
        mask |= _BITS[w]
    outs = ops.bispectrum_spectra(Xs, Ys, Zs, navg, K, mask)
    return {w: (outs[i][0] if squeeze else outs[i]) for i, w in enumerate(_BITS) if w in want}


def summed_bicoherence(b2: torch.Tensor, nfreq=None) -> torch.Tensor:
    """``sum over k + l = m`` of ``b2[..., K, K]`` for ``m < F``: ``[..., F]``, ``F = nfreq``
    (default ``K``, right for a full plane; pass ``nperseg // 2 + 1`` for a plane cut by
    ``nbins``). Plain torch on the result, on any device; NaN elements propagate."""
    if b2.dim() < 2 or b2.shape[-1] != b2.shape[-2]:
        raise ValueError("b2 must be [..., K, K]")
    K = b2.shape[-1]
    F = K if nfreq is None else int(nfreq)
    if F < K:
        raise ValueError(f"nfreq must be at least K = {K}, got {nfreq}")
    k = torch.arange(K, device=b2.device)
    m = (k[:, None] + k[None, :]).reshape(-1)
    keep = m < F
    out = torch.zeros(b2.shape[:-2] + (F,), dtype=b2.dtype, device=b2.device)
    return out.index_add_(-1, m[keep], b2.reshape(b2.shape[:-2] + (K * K,))[..., keep])
