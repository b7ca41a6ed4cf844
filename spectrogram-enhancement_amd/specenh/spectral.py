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


# ---------------------------------------------------------------- the averaging wrappers' prologue
# Shared with specenh.bispectrum, specenh.wavenumber and specenh.correlation, in the order the
# wrappers check: plan arguments, tensors, frames and groups, and last the device.
def _plan_args(nperseg, noverlap, scaling, detrend):
    """(nperseg, noverlap, scaling code, detrend code), normalised as scipy's arguments."""
    nperseg, noverlap = _check_nperseg(nperseg, noverlap)
    return nperseg, noverlap, _norm_scaling(scaling), _norm_detrend(detrend)


def _names(sig):
    return ", ".join(list(sig)[:-1]) + " and " + list(sig)[-1]


def _signals(need_all=False, **sig):
    """Tensors by name, each (unless None, where that is allowed) of the first one's shape and
    device, [batch, length] or [length]; whether they are 1-D."""
    first, x = next(iter(sig.items()))
    for name, v in sig.items():
        if not isinstance(v, torch.Tensor) and (need_all or v is not None):
            raise TypeError(f"{name} must be a torch.Tensor")
    if x.dim() not in (1, 2):
        raise ValueError(f"{first} must be [batch, length]")
    for v in sig.values():
        if v is not None and (v.shape != x.shape or v.device != x.device):
            raise ValueError(f"{_names(sig)} must have the same shape and device")
    return x.dim() == 1


def _groups(L, nperseg, noverlap, navg):
    """(navg as an int, frames, groups) of signals of L samples."""
    if L < nperseg:
        raise ValueError(f"signal of {L} samples is shorter than nperseg = {nperseg}")
    navg = int(navg or 0)
    T = (L - nperseg) // (nperseg - noverlap) + 1
    if navg > T:
        raise ValueError(f"navg = {navg} exceeds the number of frames ({T})")
    return navg, T, (1 if navg <= 0 else T // navg)


def _gpu_only(t, module, what="signals"):
    if t.device.type != "cuda":
        raise RuntimeError(f"specenh.{module} runs on the GPU only (no CPU fallback); "
                           f"move the {what} to a ROCm device first")


def _same(a, b):
    return (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()
            and a.dtype == b.dtype)


def _prep(v):
    if v.dim() == 1:
        v = v.unsqueeze(0)
    if v.dtype != torch.float32:
        v = v.float()
    return v if v.stride(1) == 1 else v.contiguous()


def _spectra(need_all=False, **sig):
    """Complex spectra by name, each (unless None, where that is allowed) like the first,
    [batch, frames, F] or [frames, F]: (whether 2-D, frames, F, prep); prep(v) is v as the
    operators take it."""
    first, X = next(iter(sig.items()))
    for name, v in sig.items():
        if not isinstance(v, torch.Tensor) and (need_all or v is not None):
            raise TypeError(f"{name} must be a torch.Tensor")
    if not X.is_complex() or X.dim() not in (2, 3):
        raise ValueError(f"{first} must be complex [batch, frames, F]")
    for v in sig.values():
        if v is not None and (v.shape != X.shape or v.device != X.device or not v.is_complex()):
            raise ValueError(f"{_names(sig)} must be complex and have the same shape and device")
    squeeze = X.dim() == 2
    T, F = X.shape[-2], X.shape[-1]
    if not 1 <= F <= 2049:
        raise ValueError(f"F must be in [1, 2049], got {F}")

    def prep(v):
        v = v.unsqueeze(0) if squeeze else v
        return v.to(torch.complex64).contiguous()

    return squeeze, T, F, prep


def _spectra_groups(T, navg):
    """navg as an int, checked against the T frames of spectra."""
    navg = int(navg or 0)
    if T < 1:
        raise ValueError("the spectra must hold at least one frame")
    if navg > T:
        raise ValueError(f"navg = {navg} exceeds the number of frames ({T})")
    return navg


def _capped(B, cap, one_shot, other_bytes=0):
    """Cuts a batch of B shots into launches whose workspace stays under `cap` bytes (a single
    shot above it still runs alone): yields (cut, workspace), the workspace shared by the
    launches; cut(v) is the launch's shots of v[B, ...] (v itself when the launch is the whole
    batch; None stays None). `one_shot()` is the operator's own ``*_workspace`` for one shot; a
    workspace is linear in the batch, and one byte says that none is needed: then the batch is
    one launch. `other_bytes`: what else a shot of a launch holds under the cap."""
    if not B:
        return
    ws = one_shot()
    per_shot = ws.numel() if ws.numel() > 1 else 0
    step = B
    if per_shot or other_bytes:
        step = min(B, max(1, int(cap) // max(per_shot, other_bytes)))
    if per_shot and step > 1:
        ws = ws.new_empty(per_shot * step)
    if step == B:  # one launch: the tensors as they are, no views
        yield (lambda v: v), ws
        return
    for b0 in range(0, B, step):
        yield (lambda v, b0=b0: None if v is None else v[b0:b0 + step]), ws


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
    nperseg, noverlap, sc, dt = _plan_args(nperseg, noverlap, scaling, detrend)
    squeeze = _signals(x=x, y=y)
    want = tuple(want)
    if not want or any(w not in _BITS for w in want):
        raise ValueError(f"want must name some of {tuple(_BITS)}, got {want}")
    if y is None and any(w != "pxx" for w in want):
        raise ValueError("pyy, pxy and coh need a second signal y")
    L = x.shape[-1]
    navg, _, _ = _groups(L, nperseg, noverlap, navg)
    _gpu_only(x, "spectral")
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


def _array(x):
    """x[batch, channels, length] or [channels, length] of 2 to 64 channels; whether 2-D."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("x must be a torch.Tensor")
    if x.dim() not in (2, 3):
        raise ValueError("x must be [batch, channels, length] or [channels, length]")
    if not 2 <= x.shape[-2] <= _lib.CSM_MAX_CHANNELS:
        raise ValueError(f"channels must be in [2, {_lib.CSM_MAX_CHANNELS}], got {x.shape[-2]} "
                         "(one channel: welch)")
    return x.dim() == 2


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
    nperseg, noverlap, sc, dt = _plan_args(nperseg, noverlap, scaling, detrend)
    squeeze = _array(x)
    want = tuple(want)
    if not want or any(w not in _CSM_BITS for w in want):
        raise ValueError(f"want must name some of {tuple(_CSM_BITS)}, got {want}")
    C, L = x.shape[-2], x.shape[-1]
    navg, _, G = _groups(L, nperseg, noverlap, navg)
    _gpu_only(x, "spectral")
    x = _prep_array(x)
    B = x.shape[0]
    args = (nperseg, noverlap, window_key(window, nperseg), float(fs), sc, dt, navg)
    shape = (B, nperseg // 2 + 1, G, C, C)
    outs = [torch.empty(shape, dtype=d, device=x.device) if w in want else None
            for w, d in (("csm", torch.complex64), ("coh", torch.float32))]
    for cut, ws in _capped(B, CSM_WORKSPACE_CAP, lambda: csm_workspace(x[:1], *args)):
        ops.csm_out(cut(x), *args, cut(outs[0]), cut(outs[1]), ws)
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
    _gpu_only(S, "spectral", "matrices")
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
    nperseg, noverlap, sc, dt = _plan_args(nperseg, noverlap, scaling, detrend)
    squeeze = _array(x)
    C, L = x.shape[-2], x.shape[-1]
    k = int(k)
    if not 1 <= k <= C:
        raise ValueError(f"k must be in [1, {C}], got {k}")
    navg, _, G = _groups(L, nperseg, noverlap, navg)
    _gpu_only(x, "spectral")
    x = _prep_array(x)
    B, F = x.shape[0], nperseg // 2 + 1
    args = (nperseg, noverlap, window_key(window, nperseg), float(fs), sc, dt, navg)
    power = torch.empty((B, F, G, C), dtype=torch.float32, device=x.device)
    modes = torch.empty((B, F, G, k, C), dtype=torch.complex64, device=x.device)
    buf = None  # the matrices of a launch: 8 F G C C bytes a shot, under the cap too
    for cut, ws in _capped(B, CSM_WORKSPACE_CAP, lambda: csm_workspace(x[:1], *args),
                           8 * F * G * C * C):
        shots = cut(x)
        n = shots.shape[0]
        if buf is None:  # the first launch is the largest
            buf = torch.empty((n, F, G, C, C), dtype=torch.complex64, device=x.device)
        ops.csm_out(shots, *args, buf[:n], None, ws)
        ops.herm_eig_out(buf[:n], k, cut(power), cut(modes), None)
    est = {"power": power, "modes": modes,
           "fraction": power[..., :k] / power.sum(-1, keepdim=True)}
    if squeeze:
        est = {name: v[0] for name, v in est.items()}
    return frequencies(nperseg, fs), group_times(L, nperseg, noverlap, fs, navg), est
