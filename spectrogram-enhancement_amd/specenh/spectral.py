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

Channel arrays: ``cross_spectral_matrix`` / ``coherence_matrix`` give the Hermitian matrix of
all channel pairs ``[B, F, G, C, C]`` in one call (csrc/spectral_matrix.hip through
``torch.ops.specenh.csm`` -> ``specenh_csm``): every frame is transformed once, then summed as
a Gram product per frequency on the fp32 matrix cores. ``array_modes`` / ``hermitian_modes``
decompose those matrices (csrc/herm_eig.hip through ``torch.ops.specenh.herm_eig``): mode powers
and the leading mode structures, without holding the matrices of the whole batch.
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


# ---------------------------------------------------------------- channel arrays
_CSM_BITS = {"csm": _lib.CSM_CSM, "coh": _lib.CSM_COH}
# One launch's workspace stays under this many bytes (the batch is split into several
# launches; a single shot above it still runs alone). Results do not depend on the split.
CSM_WORKSPACE_CAP = _lib.CSM_WORKSPACE_CAP


def _prep_array(x):
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dtype != torch.float32:
        x = x.float()
    B, C, L = x.shape
    cs = x.stride(1) if C > 1 else L
    bs = x.stride(0) if B > 1 else C * cs
    return x if x.stride(2) == 1 and cs >= L and bs >= C * cs else x.contiguous()


def cross_spectral_matrix(x: torch.Tensor, fs: float = 1.0, window="hann", nperseg: int = 256,
                          noverlap=None, detrend="constant", scaling="density", navg=None,
                          want=("csm", "coh")):
    """The cross-spectral matrix of a channel array ``x[B, C, L]`` on a ROCm device
    (csrc/spectral_matrix.hip through ``torch.ops.specenh.csm``): every channel's frames are
    transformed once, then summed as a Gram product per frequency on the matrix cores.

    Returns ``(f, t_groups, est)``: ``est["csm"]`` complex64 ``[B, F, G, C, C]`` with
    ``[..., i, j]`` what ``scipy.signal.csd(x_i, x_j, ..., average='mean')`` gives on group
    ``g``'s slice (the groups of ``spectral_estimates``), Hermitian bit for bit with a real
    diagonal (the Welch PSDs); ``est["coh"]`` float32 ``|S_ij|^2 / (S_ii S_jj)`` (0/0 is NaN).
    ``2 <= C <= 64``. ``x[C, L]`` gives ``[F, G, C, C]``.
    """
    from .ops import ops, csm_workspace, window_key
    nperseg, noverlap = _check_nperseg(nperseg, noverlap)
    sc, dt = _norm_scaling(scaling), _norm_detrend(detrend)
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() not in (2, 3):
        raise ValueError("x must be [batch, channels, length] or [channels, length]")
    squeeze = x.dim() == 2
    want = tuple(want)
    if not want or any(w not in _CSM_BITS for w in want):
        raise ValueError(f"want must name some of {tuple(_CSM_BITS)}, got {want}")
    C, L = x.shape[-2], x.shape[-1]
    if not 2 <= C <= _lib.CSM_MAX_CHANNELS:
        raise ValueError(f"channels must be in [2, {_lib.CSM_MAX_CHANNELS}], got {C} "
                         "(one channel: welch)")
    if L < nperseg:
        raise ValueError(f"signal of {L} samples is shorter than nperseg = {nperseg}")
    navg = int(navg or 0)
    T = (L - nperseg) // (nperseg - noverlap) + 1
    if navg > T:
        raise ValueError(f"navg = {navg} exceeds the number of frames ({T})")
    if x.device.type != "cuda":
        raise RuntimeError("specenh.spectral runs on the GPU only (no CPU fallback); "
                           "move the signals to a ROCm device first")
    x = _prep_array(x)
    B = x.shape[0]
    G = 1 if navg <= 0 else T // navg
    key = window_key(window, nperseg)
    args = (nperseg, noverlap, key, float(fs), sc, dt, navg)
    shape = (B, nperseg // 2 + 1, G, C, C)
    outs = [torch.empty(shape, dtype=d, device=x.device) if w in want else None
            for w, d in (("csm", torch.complex64), ("coh", torch.float32))]
    per_shot = 8 * shape[1] * G * (navg if navg >= 1 else T) * C  # workspace bytes a shot
    step = max(1, int(CSM_WORKSPACE_CAP) // per_shot)
    ws = csm_workspace(x[:min(step, B)], *args) if B else None
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        ops.csm_out(x[b0:b1], *args, *(None if o is None else o[b0:b1] for o in outs), ws)
    est = {w: (o[0] if squeeze else o) for w, o in zip(("csm", "coh"), outs) if o is not None}
    return frequencies(nperseg, fs), group_times(L, nperseg, noverlap, fs, navg), est


def coherence_matrix(x: torch.Tensor, fs: float = 1.0, window="hann", nperseg: int = 256,
                     noverlap=None, detrend="constant"):
    """``scipy.signal.coherence`` of every channel pair of ``x[B, C, L]``:
    ``(f, Cxy[B, F, C, C])`` float32 on the device (``[F, C, C]`` for ``x[C, L]``)."""
    f, _, est = cross_spectral_matrix(x, fs, window, nperseg, noverlap, detrend, "density", None,
                                      ("coh",))
    return f, est["coh"][..., 0, :, :]


# ---------------------------------------------------------------- mode decomposition
def hermitian_modes(S: torch.Tensor, k: int = 1, return_sweeps: bool = False):
    """Eigenvalues and the ``k`` leading eigenvectors of the Hermitian matrices
    ``S[..., n, n]`` on a ROCm device (csrc/herm_eig.hip through ``torch.ops.specenh.herm_eig``:
    cyclic Jacobi, one wave per matrix, ``2 <= n <= 64``).

    Returns ``(w, v)``: ``w`` float32 ``[..., n]`` descending (not clamped at 0), ``v``
    complex64 ``[..., k, n]``; ``v[..., m, :]`` is ``numpy.linalg.eigh``'s ``V[..., :, m]`` for
    the same (descending) order, of unit norm, its component of largest modulus real positive.
    Only the upper triangle and the real part of the diagonal are read; a matrix with a
    non-finite element there gives NaN for that matrix alone. ``0 <= k <= n``. With
    ``return_sweeps`` a third result: the Jacobi sweeps every matrix ran, int32 ``[...]``.
    """
    from .ops import ops
    if not isinstance(S, torch.Tensor):
        raise TypeError("S must be a torch.Tensor")
    if not S.is_complex() or S.dim() < 2 or S.shape[-1] != S.shape[-2]:
        raise ValueError("S must be complex [..., n, n]")
    n = S.shape[-1]
    if not 2 <= n <= _lib.HERM_EIG_MAX_N:
        raise ValueError(f"n must be in [2, {_lib.HERM_EIG_MAX_N}], got {n}")
    k = int(k)
    if not 0 <= k <= n:
        raise ValueError(f"k must be in [0, {n}], got {k}")
    if S.device.type != "cuda":
        raise RuntimeError("specenh.spectral runs on the GPU only (no CPU fallback); "
                           "move the matrices to a ROCm device first")
    if S.dtype != torch.complex64:
        S = S.to(torch.complex64)
    lead = tuple(S.shape[:-2])
    w = torch.empty(lead + (n,), dtype=torch.float32, device=S.device)
    v = torch.empty(lead + (k, n), dtype=torch.complex64, device=S.device)
    sweeps = torch.empty(lead, dtype=torch.int32, device=S.device) if return_sweeps else None
    ops.herm_eig_out(S, k, w, v, sweeps)
    return (w, v, sweeps) if return_sweeps else (w, v)


def array_modes(x: torch.Tensor, k: int = 1, fs: float = 1.0, window="hann", nperseg: int = 256,
                noverlap=None, detrend="constant", scaling="density", navg=None):
    """Mode decomposition of a channel array ``x[B, C, L]`` on a ROCm device: the
    eigendecomposition of the cross-spectral matrix of every frequency and averaging group
    (``cross_spectral_matrix`` then ``hermitian_modes``), without ever holding
    ``[B, F, G, C, C]``: the batch runs in slices through one reused matrix buffer, sized so
    that the slice's CSM workspace and its matrices each stay under ``CSM_WORKSPACE_CAP`` (a
    single shot above it runs alone). Results do not depend on the split.

    Returns ``(f, t_groups, est)``: ``est["power"]`` float32 ``[B, F, G, C]`` (the eigenvalues,
    descending), ``est["modes"]`` complex64 ``[B, F, G, k, C]`` (the leading eigenvectors, the
    conventions of ``hermitian_modes``), ``est["fraction"]`` float32 ``[B, F, G, k]`` =
    ``power[..., :k] / power.sum(-1)`` (0/0 is NaN). ``1 <= k <= C``. ``x[C, L]`` drops ``B``.
    """
    from .ops import ops, csm_workspace, window_key
    nperseg, noverlap = _check_nperseg(nperseg, noverlap)
    sc, dt = _norm_scaling(scaling), _norm_detrend(detrend)
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() not in (2, 3):
        raise ValueError("x must be [batch, channels, length] or [channels, length]")
    squeeze = x.dim() == 2
    C, L = x.shape[-2], x.shape[-1]
    if not 2 <= C <= _lib.CSM_MAX_CHANNELS:
        raise ValueError(f"channels must be in [2, {_lib.CSM_MAX_CHANNELS}], got {C} "
                         "(one channel: welch)")
    k = int(k)
    if not 1 <= k <= C:
        raise ValueError(f"k must be in [1, {C}], got {k}")
    if L < nperseg:
        raise ValueError(f"signal of {L} samples is shorter than nperseg = {nperseg}")
    navg = int(navg or 0)
    T = (L - nperseg) // (nperseg - noverlap) + 1
    if navg > T:
        raise ValueError(f"navg = {navg} exceeds the number of frames ({T})")
    if x.device.type != "cuda":
        raise RuntimeError("specenh.spectral runs on the GPU only (no CPU fallback); "
                           "move the signals to a ROCm device first")
    x = _prep_array(x)
    B = x.shape[0]
    F, G = nperseg // 2 + 1, (1 if navg <= 0 else T // navg)
    args = (nperseg, noverlap, window_key(window, nperseg), float(fs), sc, dt, navg)
    power = torch.empty((B, F, G, C), dtype=torch.float32, device=x.device)
    modes = torch.empty((B, F, G, k, C), dtype=torch.complex64, device=x.device)
    # bytes a shot: the CSM workspace (spectra of every frame) and the matrices themselves
    per_shot = max(8 * F * G * (navg if navg >= 1 else T) * C, 8 * F * G * C * C)
    step = max(1, int(CSM_WORKSPACE_CAP) // per_shot)
    if B:
        ws = csm_workspace(x[:min(step, B)], *args)
        buf = torch.empty((min(step, B), F, G, C, C), dtype=torch.complex64, device=x.device)
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        ops.csm_out(x[b0:b1], *args, buf[:b1 - b0], None, ws)
        ops.herm_eig_out(buf[:b1 - b0], k, power[b0:b1], modes[b0:b1], None)
    est = {"power": power, "modes": modes,
           "fraction": power[..., :k] / power.sum(-1, keepdim=True)}
    if squeeze:
        est = {name: v[0] for name, v in est.items()}
    return frequencies(nperseg, fs), group_times(L, nperseg, noverlap, fs, navg), est
