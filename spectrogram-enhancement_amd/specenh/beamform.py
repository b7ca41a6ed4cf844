"""Steered-response spectra of a channel array on a ROCm device: the Bartlett (conventional),
Capon (minimum-variance; Capon, Proc. IEEE 57, 1408, 1969) and MUSIC (Schmidt, IEEE Trans.
Antennas Propag. 34, 276, 1986) estimators, per frequency bin and averaging group. What a
toroidal or poloidal mode number, or the wavenumber on a linear BES or interferometer array, is
read from: the many-channel counterpart of the two-point ``specenh.wavenumber`` spectrum.

Conventions. ``S_ij = mean_t conj(X_i) X_j`` (the sign of ``scipy.signal.csd``). A steering
vector is ``a_c(kappa) = exp(i kappa p_c)``, ``p_c`` the position (m) or angle (rad) of channel
``c``, ``kappa`` a wavenumber or a mode number. A fluctuation ``X_c ~ exp(i kappa0 p_c)``, that
is ``arg S_ij = kappa0 (p_j - p_i)``, peaks at ``kappa = kappa0`` (the sign of ``k = theta / dx``
in ``specenh.wavenumber``). With ``|a|^2 = sum_c |a_c|^2`` and ``(lambda_m, v_m)`` the
eigenpairs of ``S`` (``v_m`` row ``m`` of ``hermitian_modes``' ``v``)::

    P_bartlett = sum_ij a_i S_ij conj(a_j) / |a|^4 = mean_t |sum_c conj(a_c) X_c|^2 / |a|^4
    P_capon    = 1 / sum_m |sum_c a_c v_m[c]|^2 / (max(lambda_m, 0) + delta),
                 delta = loading * sum_m lambda_m / C
    P_music    = |a|^2 / sum_{m >= nsources} |sum_c a_c v_m[c]|^2

One plane wave of PSD ``p`` gives ``P_bartlett = p``; ``P_music`` is dimensionless and >= 1.
A Capon term whose ``max(lambda_m, 0) + delta`` is exactly 0 (a mode without power and without
loading) carries no weight, as in the pseudo-inverse of ``S``. The last division is IEEE's:
``1 / 0`` is ``inf``, so an array without any power gives ``P_bartlett = 0`` and
``P_capon = inf``. A non-finite sample makes the outputs of its shot non-finite and of no other.

All three are one kernel (csrc/steered_power.hip through ``torch.ops.specenh.steered_power``
-> ``specenh_steered_power``): ``q[n] = sum_m w[m] |sum_c V[m, c] A[n, c]|^2`` on the fp32
matrix cores. Bartlett is fused (``torch.ops.specenh.array_spectrum_out`` ->
``specenh_array_spectrum``): the rows are the frame spectra the CSM's transform kernel writes
to its workspace, read in place; the matrix ``[B, F, G, C, C]`` is never formed. Capon and MUSIC
take the eigenvectors of ``torch.ops.specenh.herm_eig``. Results stay on the device; ``f`` and
the group times are float64 numpy arrays computed on the host. There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from . import spectral as _spectral
from .spectral import _array, _capped, _gpu_only, _groups, _plan_args, _prep_array, group_times
from .stft import frequencies

METHODS = ("bartlett", "capon", "music")
_POST = {"sum": _lib.STEER_SUM, "bartlett": _lib.STEER_BARTLETT, "inverse": _lib.STEER_INVERSE,
         "music": _lib.STEER_MUSIC}


def steering_vectors(positions, kappa, device=None) -> torch.Tensor:
    """``a[k, c] = exp(i kappa_k p_c)`` as complex64 ``[K, C]`` on ``device``: the phase is
    computed in float64 on the host and the result rounded once."""
    p = np.asarray(positions, dtype=np.float64)
    k = np.asarray(kappa, dtype=np.float64)
    if p.ndim != 1 or k.ndim != 1 or not p.size or not k.size:
        raise ValueError("positions must be [C] and kappa [K], neither empty")
    a = np.exp(1j * k[:, None] * p[None, :]).astype(np.complex64)
    return torch.from_numpy(a).to(device) if device is not None else torch.from_numpy(a)


def delay_steering(f, delays, device=None) -> torch.Tensor:
    """``a[f, k, c] = exp(-2 pi i f tau_kc)`` as complex64 ``[F, K, C]`` on ``device``, a table
    per frequency bin for broadband direction finding: ``delays[K, C]`` (s) is the arrival time
    at channel ``c`` of a wave from direction ``k``, ``f`` (Hz) the bin frequencies. The phase is
    computed in float64 on the host and the result rounded once."""
    f = np.asarray(f, dtype=np.float64)
    tau = np.asarray(delays, dtype=np.float64)
    if f.ndim != 1 or tau.ndim != 2 or not f.size or not tau.size:
        raise ValueError("f must be [F] and delays [K, C], neither empty")
    a = np.exp(-2j * np.pi * f[:, None, None] * tau[None, :, :]).astype(np.complex64)
    return torch.from_numpy(a).to(device) if device is not None else torch.from_numpy(a)


def _table(A, C, F=None):
    """A steering table as the operators take it: contiguous complex64 [K, C] or [F, K, C]."""
    if not isinstance(A, torch.Tensor):
        raise TypeError("A must be a torch.Tensor")
    if not A.is_complex():
        raise ValueError("A must be complex [K, C] or [F, K, C]")
    if A.dim() not in (2, 3) or A.shape[-1] != C or (A.dim() == 3 and F is not None
                                                     and A.shape[0] != F):
        where = f"[K, {C}]" + (f" or [{F}, K, {C}]" if F is not None else " or [F, K, C]")
        raise ValueError(f"A must be complex {where}, got {tuple(A.shape)}")
    K = A.shape[-2]
    if not 1 <= K <= _lib.STEER_MAX_NSTEER:
        raise ValueError(f"K must be in [1, {_lib.STEER_MAX_NSTEER}], got {K}")
    return A.to(torch.complex64).contiguous()


def steered_power(V: torch.Tensor, w, A: torch.Tensor, post: str = "sum", scale=1.0,
                  conj: bool = False) -> torch.Tensor:
    """The generic operator: ``q[..., n] = sum_m w[..., m] |sum_c V[..., m, c] A[n, c]|^2`` of
    rows ``V[..., M, C]`` (complex), weights ``w[..., M]`` (None: all ones) and a table
    ``A[K, C]``, or ``A[F, K, C]`` for ``V[..., F, G, M, C]`` (one table per bin). ``conj``
    takes ``conj(A)``. ``post``: ``"sum"`` gives ``q scale``, ``"bartlett"``
    ``q scale / |a_n|^4``, ``"inverse"`` ``scale / q``, ``"music"`` ``|a_n|^2 / q``; ``scale`` is
    a number or one factor per table ``[F]``. Returns float32 ``[..., K]``."""
    from .ops import ops
    if not isinstance(V, torch.Tensor):
        raise TypeError("V must be a torch.Tensor")
    if not V.is_complex() or V.dim() < 2:
        raise ValueError("V must be complex [..., M, C]")
    if post not in _POST:
        raise ValueError(f"post must be one of {tuple(_POST)}, got {post!r}")
    A = _table(A, V.shape[-1])
    if w is not None and (not isinstance(w, torch.Tensor) or w.shape != V.shape[:-1]):
        raise ValueError(f"w must be a tensor {tuple(V.shape[:-1])} or None")
    _gpu_only(V, "beamform", "rows")
    table = None
    if not isinstance(scale, (int, float)):
        table = torch.as_tensor(scale, dtype=torch.float64, device=V.device).contiguous()
        scale = 1.0
    return ops.steered_power(V.to(torch.complex64), None if w is None else w.float(),
                             A.to(V.device), _POST[post], float(scale), bool(conj), table)


def array_spectrum(x: torch.Tensor, A: torch.Tensor, method: str = "bartlett",
                   nsources: int = 1, loading: float = 1e-2, fs: float = 1.0, window="hann",
                   nperseg: int = 256, noverlap=None, detrend="constant", scaling="density",
                   navg=None):
    """The steered-response spectrum of a channel array ``x[B, C, L]`` on the steering vectors
    ``A[K, C]`` (``steering_vectors``), or ``A[F, K, C]`` (``delay_steering``: one table per
    frequency bin), ``2 <= C <= 64``, ``1 <= K <= 4096``.

    Returns ``(f, t_groups, P)``: ``P`` float32 ``[B, F, G, K]`` (the groups of
    ``spectral_estimates``); ``x[C, L]`` drops ``B``. ``method``:

    ``"bartlett"``  one fused call, the transform of ``cross_spectral_matrix`` followed by the
        steered-power kernel on its workspace: ``a^T S conj(a) / |a|^4`` without ``S``.
    ``"capon"``  ``loading >= 0`` is the diagonal loading relative to the mean eigenvalue.
    ``"music"``  ``nsources`` in ``[1, C - 1]`` leading eigenvectors span the signal subspace.

    Capon and MUSIC decompose the cross-spectral matrices as ``array_modes`` does, in batch
    slices through reused buffers, the slice's workspace, matrices and eigenvectors each under
    ``specenh.spectral.CSM_WORKSPACE_CAP``; results do not depend on the split.
    """
    from .ops import array_spectrum_workspace, csm_workspace, ops, window_key
    nperseg, noverlap, sc, dt = _plan_args(nperseg, noverlap, scaling, detrend)
    squeeze = _array(x)
    C, L = x.shape[-2], x.shape[-1]
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    nsources = int(nsources)
    if not 1 <= nsources <= C - 1:
        raise ValueError(f"nsources must be in [1, {C - 1}], got {nsources}")
    loading = float(loading)
    if not loading >= 0:
        raise ValueError(f"loading must be >= 0, got {loading}")
    F = nperseg // 2 + 1
    A = _table(A, C, F)
    K = A.shape[-2]
    navg, _, G = _groups(L, nperseg, noverlap, navg)
    _gpu_only(x, "beamform")
    x = _prep_array(x)
    A = A.to(x.device)
    B = x.shape[0]
    args = (nperseg, noverlap, window_key(window, nperseg), float(fs), sc, dt, navg)
    P = torch.empty((B, F, G, K), dtype=torch.float32, device=x.device)
    cap = _spectral.CSM_WORKSPACE_CAP
    if method == "bartlett":
        for cut, ws in _capped(B, cap, lambda: array_spectrum_workspace(x[:1], *args)):
            ops.array_spectrum_out(cut(x), *args, A, cut(P), ws)
    else:
        S = lam = v = None  # a launch's matrices, eigenvalues and eigenvectors
        for cut, ws in _capped(B, cap, lambda: csm_workspace(x[:1], *args), 8 * F * G * C * C):
            shots = cut(x)
            n = shots.shape[0]
            if S is None:  # the first launch is the largest
                S = torch.empty((n, F, G, C, C), dtype=torch.complex64, device=x.device)
                v = torch.empty_like(S)
                lam = torch.empty((n, F, G, C), dtype=torch.float32, device=x.device)
            ops.csm_out(shots, *args, S[:n], None, ws)
            ops.herm_eig_out(S[:n], C, lam[:n], v[:n], None)
            if method == "capon":
                lam64 = lam[:n].double()
                delta = loading * lam64.sum(-1, keepdim=True) / C
                d = lam64.clamp_min(0) + delta
                # a term without power and without loading has no weight (the pseudo-inverse)
                w = torch.where(d == 0, torch.zeros_like(d), 1.0 / d).float()
                post = _lib.STEER_INVERSE
            else:
                w = torch.ones_like(lam[:n])
                w[..., :nsources] = 0
                post = _lib.STEER_MUSIC
            ops.steered_power_out(v[:n], w, A, post, 1.0, False, None, cut(P))
    return (frequencies(nperseg, fs), group_times(L, nperseg, noverlap, fs, navg),
            P[0] if squeeze else P)


def mode_number_spectrum(x: torch.Tensor, angles, nmax: int, method: str = "bartlett", **kw):
    """``array_spectrum`` on the integer mode numbers ``n = -nmax .. nmax`` of channels at
    ``angles`` (rad): returns ``(f, t_groups, n, P[B, F, G, 2 nmax + 1])``."""
    nmax = int(nmax)
    if nmax < 0:
        raise ValueError(f"nmax must be >= 0, got {nmax}")
    n = np.arange(-nmax, nmax + 1)
    dev = x.device if isinstance(x, torch.Tensor) else None
    f, t, P = array_spectrum(x, steering_vectors(angles, n, dev), method=method, **kw)
    return f, t, n, P
