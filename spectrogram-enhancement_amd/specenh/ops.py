"""``torch.ops.specenh.*``: every entry point of the C-ABI (include/specenh.h) as a PyTorch
operator.

The Python API that keeps the reference's names (``pipeline_data``, ``svd``, ``keras``,
``strips``, ``cross``, ``filters``) reaches the HIP kernels only through these operators:

    reference call site -> specenh.<module> -> torch.ops.specenh.<op> -> C-ABI -> HIP

Each operator is defined with an explicit schema on a ``torch.library.Library`` (its
dispatch costs ~2.5 us a call, a sixth of ``torch.library.custom_op``'s), implemented for
the CUDA (= HIP on ROCm) dispatch key only — a CPU tensor raises NotImplementedError, there
is no fallback — and has a fake (meta) kernel, so shapes propagate through FakeTensor /
``torch.compile`` tracing. Operators ending in ``_out`` write caller-owned buffers (the
autoencoder engine reuses its activations across calls); the others allocate.
``tests/test_ops_gpu.py`` runs ``torch.library.opcheck`` on each.

Every launch goes on the current HIP stream of the tensors' device.
"""
from __future__ import annotations

import ctypes
import hashlib
import threading

import numpy as np
import torch

from . import _lib

F32, BF16, F16, F64 = 0, 1, 2, 3
_CODE = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16, torch.float64: F64}


def _vp(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _st(t) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _code(t: torch.Tensor, allowed=(F32, BF16, F16)) -> int:
    c = _CODE.get(t.dtype)
    if c is None or c not in allowed:
        raise TypeError(f"unsupported dtype {t.dtype}")
    return c


def _need(t: torch.Tensor, name: str):
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


_LIB = torch.library.Library("specenh", "DEF")


def _op(schema: str, impl, fake):
    name = schema.split("(", 1)[0]
    _LIB.define(schema)
    _LIB.impl(name, impl, "CUDA")
    torch.library.register_fake(f"specenh::{name}", fake, lib=_LIB)


# ---------------------------------------------------------------- windows / plans
_windows: dict = {}
_wlock = threading.Lock()


def window_key(window, nperseg: int) -> str:
    """A string naming a window for the STFT / CSD operators: scipy window names pass
    through; tuples and coefficient arrays are registered under their sha1 digest."""
    if isinstance(window, str):
        return window
    from .stft import get_window
    w = np.ascontiguousarray(get_window(window, int(nperseg)), dtype=np.float64)
    key = "sha1:" + hashlib.sha1(w.tobytes()).hexdigest()
    with _wlock:
        _windows.setdefault(key, w)
    return key


def window_coefs(key: str, nperseg: int) -> np.ndarray:
    if key.startswith("sha1:"):
        w = _windows.get(key)
        if w is None or w.shape[0] != nperseg:
            raise ValueError(f"unknown window {key!r} (register it with ops.window_key)")
        return w
    from .stft import get_window
    return get_window(key, int(nperseg))


# ---------------------------------------------------------------- STFT-PSD
def _stft_shape(x, nperseg, noverlap, flags):
    T = (x.shape[-1] - nperseg) // (nperseg - noverlap) + 1
    F = nperseg // 2 + (0 if flags & _lib.STFT_DROP_NYQUIST else 1)
    return x.shape[0], F, T


def _stft_out(x, nperseg, noverlap, window, fs, scaling, detrend, eps, flags, out):
    from . import stft
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("x must be [batch, length] with unit stride along length")
    if x.dtype not in (torch.float32, torch.float16):
        raise TypeError("x must be float32 or float16")
    if tuple(out.shape) != _stft_shape(x, nperseg, noverlap, flags) or \
            out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be contiguous float32 [batch, F, T]")
    plan = stft.get_plan_key(x.device, nperseg, noverlap, window, fs, scaling, detrend, eps)
    L = _lib.lib()
    if x.dtype == torch.float16 and nperseg > 1024:
        x = x.float()  # the fp16-sample kernel covers nperseg <= 1024
    if x.dtype == torch.float16:  # fp16 samples widened on load: no conversion pass
        _lib.check(L.specenh_stft_psd_f16(plan.handle, _vp(x), x.shape[0], x.shape[1],
                                          x.stride(0), _vp(out), flags, _st(x)), "stft_psd_f16")
        return
    ws = plan.workspace(x.shape[0], x.device)
    _lib.check(L.specenh_stft_psd(plan.handle, _vp(x), x.shape[0], x.shape[1], x.stride(0),
                                  _vp(out), flags, _vp(ws), _st(x)), "stft_psd")


def _stft(x, nperseg, noverlap, window, fs, scaling, detrend, eps, flags):
    out = torch.empty(_stft_shape(x, nperseg, noverlap, flags), dtype=torch.float32,
                      device=x.device)
    _stft_out(x, nperseg, noverlap, window, fs, scaling, detrend, eps, flags, out)
    return out


_STFT_ARGS = "int nperseg, int noverlap, str window, float fs, int scaling, int detrend, " \
             "float eps, int flags"
_op(f"stft_psd(Tensor x, {_STFT_ARGS}) -> Tensor", _stft,
    lambda x, nperseg, noverlap, window, fs, scaling, detrend, eps, flags:
    x.new_empty(_stft_shape(x, nperseg, noverlap, flags), dtype=torch.float32))
_op(f"stft_psd_out(Tensor x, {_STFT_ARGS}, Tensor(a!) out) -> ()", _stft_out,
    lambda *a: None)


# ---------------------------------------------------------------- complex STFT / inverse
def _cx_frames(length, nperseg, noverlap, boundary, padded):
    """specenh_stft_complex_frames (scipy.signal.stft's frame count), also on symbolic sizes."""
    hop = nperseg - noverlap
    ext = length + (nperseg if boundary else 0)
    nadd = ((-(ext - nperseg)) % hop) % nperseg if padded else 0
    return (ext + nadd - nperseg) // hop + 1


def _istft_len(frames, nperseg, noverlap, boundary):
    return (nperseg - noverlap) * (frames - 1) + (0 if boundary else nperseg)


def _stft_complex_out(x, nperseg, noverlap, window, fs, scaling, detrend, boundary, padded, out):
    from . import stft
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype != torch.float32:
        raise ValueError("x must be float32 [batch, length] with unit stride along length")
    if boundary not in (_lib.BOUNDARY_NONE, _lib.BOUNDARY_ZEROS):
        raise NotImplementedError("boundary must be None or 'zeros' on the GPU path")
    B, L = x.shape
    if L < nperseg:
        raise ValueError("signal shorter than nperseg")
    shape = (B, nperseg // 2 + 1, _cx_frames(L, nperseg, noverlap, boundary, padded))
    if tuple(out.shape) != shape or out.dtype != torch.complex64 or not out.is_contiguous():
        raise ValueError(f"out must be contiguous complex64 {shape}")
    plan = stft.get_plan_key(x.device, nperseg, noverlap, window, fs, scaling, detrend, 0.0)
    _lib.check(_lib.lib().specenh_stft_complex(
        plan.handle, _vp(x), B, L, x.stride(0) if B > 1 else L, _vp(out), int(boundary),
        int(padded), _st(x)), "stft_complex")


def _stft_complex(x, nperseg, noverlap, window, fs, scaling, detrend, boundary, padded):
    if noverlap >= nperseg:
        raise ValueError("noverlap must be less than nperseg.")
    out = torch.empty((x.shape[0], nperseg // 2 + 1,
                       _cx_frames(x.shape[1], nperseg, noverlap, boundary, padded)),
                      dtype=torch.complex64, device=x.device)
    _stft_complex_out(x, nperseg, noverlap, window, fs, scaling, detrend, boundary, padded, out)
    return out


def _istft_out(Z, gain, nperseg, noverlap, window, fs, scaling, boundary, out):
    from . import stft
    if Z.dim() != 3 or Z.dtype != torch.complex64 or not Z.is_contiguous() or Z.is_conj():
        raise ValueError("Z must be contiguous complex64 [batch, F, T]")
    B, F, T = Z.shape
    if nperseg != 2 * (F - 1):
        raise ValueError("nperseg must equal 2*(F - 1) of the one-sided spectrogram")
    rows = 0
    if gain is not None:
        if (gain.dim() != 3 or gain.dtype != torch.float32 or not gain.is_contiguous()
                or gain.device != Z.device or gain.shape[0] != B or gain.shape[2] != T
                or gain.shape[1] not in (F, F - 1)):
            raise ValueError(f"gain must be contiguous float32 [{B}, {F} or {F - 1}, {T}] on Z's "
                             "device")
        rows = gain.shape[1]
    n = _istft_len(T, nperseg, noverlap, boundary)
    if (out.dim() != 2 or out.shape[0] != B or out.shape[1] != n or out.dtype != torch.float32
            or out.stride(1) != 1 or out.device != Z.device):
        raise ValueError(f"out must be float32 [{B}, {n}] with unit stride along samples")
    plan = stft.get_plan_key(Z.device, nperseg, noverlap, window, fs, scaling, 0, 0.0)
    _lib.check(_lib.lib().specenh_istft(
        plan.handle, _vp(Z), _vp(gain), rows, B, T, _vp(out), out.stride(0) if B > 1 else n,
        int(bool(boundary)), _st(Z)), "istft")


def _istft(Z, gain, nperseg, noverlap, window, fs, scaling, boundary):
    if noverlap >= nperseg:
        raise ValueError("noverlap must be less than nperseg.")
    out = torch.empty((Z.shape[0], _istft_len(Z.shape[2], nperseg, noverlap, boundary)),
                      dtype=torch.float32, device=Z.device)
    _istft_out(Z, gain, nperseg, noverlap, window, fs, scaling, boundary, out)
    return out


_CX_ARGS = "int nperseg, int noverlap, str window, float fs, int scaling, int detrend, " \
           "int boundary, bool padded"
_op(f"stft_complex(Tensor x, {_CX_ARGS}) -> Tensor", _stft_complex,
    lambda x, nperseg, noverlap, window, fs, scaling, detrend, boundary, padded:
    x.new_empty((x.shape[0], nperseg // 2 + 1,
                 _cx_frames(x.shape[1], nperseg, noverlap, boundary, padded)),
                dtype=torch.complex64))
_op(f"stft_complex_out(Tensor x, {_CX_ARGS}, Tensor(a!) out) -> ()", _stft_complex_out,
    lambda *a: None)
_IS_ARGS = "int nperseg, int noverlap, str window, float fs, int scaling, bool boundary"
_op(f"istft(Tensor Z, Tensor? gain, {_IS_ARGS}) -> Tensor", _istft,
    lambda Z, gain, nperseg, noverlap, window, fs, scaling, boundary:
    Z.new_empty((Z.shape[0], _istft_len(Z.shape[2], nperseg, noverlap, boundary)),
                dtype=torch.float32))
_op(f"istft_out(Tensor Z, Tensor? gain, {_IS_ARGS}, Tensor(a!) out) -> ()", _istft_out,
    lambda *a: None)


# ---------------------------------------------------------------- cross spectrum
def _csd(x, y, nperseg, noverlap, window, fs, scaling, detrend, mode):
    from . import cross
    if x.shape != y.shape or x.dim() != 2 or x.dtype != torch.float32 or y.dtype != torch.float32:
        raise ValueError("x and y must be float32 [batch, length] of the same shape")
    if x.stride(1) != 1 or y.stride(1) != 1:
        raise ValueError("x and y need unit stride along length")
    plan = cross.get_plan_key(x.device, nperseg, noverlap, window, fs, scaling, detrend)
    B, L = x.shape
    T = (L - nperseg) // (nperseg - noverlap) + 1
    F = nperseg // 2 + 1
    out = torch.empty((B, F, T), dtype=torch.float32 if mode == 1 else torch.complex64,
                      device=x.device)
    for b0 in range(0, B, 65535):
        b1 = min(B, b0 + 65535)
        _lib.check(_lib.lib().specenh_csd(
            plan.handle, _vp(x[b0:b1]), _vp(y[b0:b1]), b1 - b0, L, x.stride(0), y.stride(0),
            _vp(out[b0:b1]), int(mode), _st(x)), "csd")
    return out


def _csd_fake(x, y, nperseg, noverlap, window, fs, scaling, detrend, mode):
    T = (x.shape[1] - nperseg) // (nperseg - noverlap) + 1
    return x.new_empty((x.shape[0], nperseg // 2 + 1, T),
                       dtype=torch.float32 if mode == 1 else torch.complex64)


_op("csd(Tensor x, Tensor y, int nperseg, int noverlap, str window, float fs, int scaling, "
    "int detrend, int mode) -> Tensor", _csd, _csd_fake)


# ---------------------------------------------------------------- averaging operators
# What spectral_mean, csm, bispectrum, wavenumber_spectrum and correlation share. `sig` is
# ((name, tensor or None), ...), its first signal present; `p` is the plan's arguments
# (nperseg, noverlap, window, fs, scaling, detrend). An operator's `_call` runs the checks
# once, takes the caller's outputs or allocates them from the `outputs` mask, and launches.
_F32 = (torch.float32,)


def _avg_split(length, nperseg, noverlap, navg):
    """(frames, groups) of a call; plain arithmetic, on symbolic sizes too."""
    T = (length - nperseg) // (nperseg - noverlap) + 1
    return T, (1 if navg <= 0 else T // navg)


def _avg_check_split(length, nperseg, noverlap, navg):
    if noverlap >= nperseg:
        raise ValueError("noverlap must be less than nperseg.")
    if length < nperseg:
        raise ValueError("signal shorter than nperseg")
    T, G = _avg_split(length, nperseg, noverlap, navg)
    if navg > T:
        raise ValueError(f"navg = {navg} exceeds the number of frames ({T})")
    return T, G


def _avg_names(sig):
    names = [name for name, _ in sig]
    return ", ".join(names[:-1]) + " and " + names[-1]


def _avg_check(sig, nperseg, noverlap, navg):
    """Signals [batch, length], each like the first; (frames, groups) of the call."""
    x = sig[0][1]
    shape, device = x.shape, x.device
    for name, v in sig:
        if v is None:
            continue
        if v.dim() != 2 or v.stride(1) != 1 or v.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 [batch, length] with unit stride along "
                             "length")
        if v is not x and (v.shape != shape or v.device != device):
            raise ValueError(f"{_avg_names(sig)} must have the same shape and device")
    return _avg_check_split(shape[1], nperseg, noverlap, navg)


def _avg_spectra(sig, navg):
    """Spectra [batch, frames, F], each like the first; (B, T, F, groups)."""
    X = sig[0][1]
    for name, v in sig:
        if v is None:
            continue
        if v.dim() != 3 or v.dtype != torch.complex64 or not v.is_contiguous():
            raise ValueError(f"{name} must be contiguous complex64 [batch, frames, F]")
        if v.shape != X.shape or v.device != X.device:
            raise ValueError(f"{_avg_names(sig)} must have the same shape and device")
    B, T, F = X.shape
    if not 1 <= F <= 2049:
        raise ValueError(f"F must be in [1, 2049], got {F}")
    if T < 1:
        raise ValueError("the spectra must hold at least one frame")
    if navg > T:
        raise ValueError(f"navg = {navg} exceeds the number of frames ({T})")
    return B, T, F, (1 if navg <= 0 else T // navg)


def _avg_stride(v):
    """Batch stride of v[B, L], 0 for an absent signal; the stride of a one-element axis is
    free."""
    if v is None:
        return 0
    B, L = v.shape
    s = v.stride(0) if B > 1 else L
    if s < L:
        raise ValueError("a signal must not overlap itself: batch stride >= length")
    return s


def _avg_distinct(signals, strides):
    """How many of the signals are distinct in pointer and stride, as the C entries count."""
    return len({(v.data_ptr(), s) for v, s in zip(signals, strides) if v is not None})


def _avg_plan(x, p, symbol, *extra, may_be_zero=False):
    """The plan of a call and the bytes its workspace needs: specenh_<symbol>(plan, *extra),
    extra[0] the batch. 0 is an error unless the operator can do without a workspace."""
    from . import stft
    plan = stft.get_plan_key(x.device, *p, 0.0)
    need = int(getattr(_lib.lib(), "specenh_" + symbol)(plan.handle, *extra))
    if need == 0 and extra[0] > 0 and not may_be_zero:
        _lib.check(_lib.SPECENH_EINVAL, symbol)
    return plan, need


def _avg_buffer(need, device):
    return torch.empty(max(need, 1), dtype=torch.uint8, device=device)


def _avg_workspace(workspace, need, device):
    """(workspace, its bytes) for a call that needs `need` bytes: the caller's, checked, or a new
    one; (None, 0) when none is needed."""
    if need == 0:
        return None, 0
    if workspace is None:
        workspace = _avg_buffer(need, device)
    nbytes = workspace.numel() * workspace.element_size()
    if (workspace.device != device or not workspace.is_contiguous() or nbytes < need
            or workspace.data_ptr() % 16):
        raise ValueError(f"workspace must be a contiguous, 16-byte aligned buffer of at least "
                         f"{need} bytes on x's device")
    return workspace, nbytes


def _avg_outs(x, outs, mask, shape, dtypes, what):
    """The outputs of a call, one per dtype or None: the caller's `outs`, checked, or (outs
    None) allocated where bit i of `mask` is set."""
    if outs is None:
        outs = [torch.empty(shape, dtype=dt, device=x.device) if mask >> i & 1 else None
                for i, dt in enumerate(dtypes)]
    none, device = True, x.device
    for o, dt in zip(outs, dtypes):
        if o is None:
            continue
        none = False
        if o.shape != shape or o.dtype != dt or not o.is_contiguous() or o.device != device:
            raise ValueError(f"outputs must be contiguous {shape} on x's device ({what})")
    if none:
        raise ValueError("no output requested")
    return outs


def _avg_results(x, outs, dtypes):
    """What an allocating operator returns: an empty placeholder for an output not asked for."""
    return tuple(x.new_empty((0,), dtype=dt) if o is None else o for o, dt in zip(outs, dtypes))


def _avg_fake(x, mask, shape, dtypes):
    return tuple(x.new_empty(shape if mask >> i & 1 else (0,), dtype=dt)
                 for i, dt in enumerate(dtypes))


_SP_ARGS = "int nperseg, int noverlap, str window, float fs, int scaling, int detrend, int navg"

# ---------------------------------------------------------------- averaged spectra
_SP_DTYPES = (torch.float32, torch.float32, torch.complex64, torch.float32)


def _spectral_mean_call(x, y, p, navg, outs, mask, workspace):
    _, G = _avg_check((("x", x), ("y", y)), p[0], p[1], navg)
    B, L = x.shape
    outs = _avg_outs(x, outs, mask, (B, p[0] // 2 + 1, G), _SP_DTYPES,
                     "pxx, pyy, coh float32, pxy complex64")
    if y is None and any(o is not None for o in outs[1:]):
        raise ValueError("pyy, pxy and coh need a second signal y")
    plan, need = _avg_plan(x, p, "spectral_workspace_bytes", B, L, int(navg), may_be_zero=True)
    ws, _ = _avg_workspace(workspace, need, x.device)
    _lib.check(_lib.lib().specenh_spectral_mean(
        plan.handle, _vp(x), _vp(y), B, L, _avg_stride(x), _avg_stride(y), int(navg),
        _vp(outs[0]), _vp(outs[1]), _vp(outs[2]), _vp(outs[3]), _vp(ws), _st(x)), "spectral_mean")
    return outs


def _spectral_mean_out(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, pxx, pyy, pxy,
                       coh, workspace):
    _spectral_mean_call(x, y, (nperseg, noverlap, window, fs, scaling, detrend), navg,
                        (pxx, pyy, pxy, coh), 0, workspace)


def spectral_workspace(x, nperseg, noverlap, window, fs, scaling, detrend, navg):
    """A workspace for ``spectral_mean_out`` on ``x[B, L]`` (uint8; one byte when none is
    needed), from torch's caching allocator."""
    _, need = _avg_plan(x, (nperseg, noverlap, window, fs, scaling, detrend),
                        "spectral_workspace_bytes", x.shape[0], x.shape[1], int(navg),
                        may_be_zero=True)
    return _avg_buffer(need, x.device)


def _spectral_mean(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, outputs):
    return _avg_results(x, _spectral_mean_call(
        x, y, (nperseg, noverlap, window, fs, scaling, detrend), navg, None, outputs, None),
        _SP_DTYPES)


def _spectral_mean_fake(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, outputs):
    G = _avg_split(x.shape[1], nperseg, noverlap, navg)[1]
    return _avg_fake(x, outputs, (x.shape[0], nperseg // 2 + 1, G), _SP_DTYPES)


_op(f"spectral_mean(Tensor x, Tensor? y, {_SP_ARGS}, int outputs) -> "
    "(Tensor, Tensor, Tensor, Tensor)", _spectral_mean, _spectral_mean_fake)
_op(f"spectral_mean_out(Tensor x, Tensor? y, {_SP_ARGS}, Tensor(a!)? pxx, Tensor(b!)? pyy, "
    "Tensor(c!)? pxy, Tensor(d!)? coh, Tensor(e!)? workspace) -> ()", _spectral_mean_out,
    lambda *a: None)


# ---------------------------------------------------------------- cross-spectral matrix
_CSM_DTYPES = (torch.complex64, torch.float32)


def _csm_check(x, nperseg, noverlap, navg):
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
        raise ValueError("x must be float32 [batch, channels, length] with unit stride along "
                         "length")
    if not 2 <= x.shape[1] <= _lib.CSM_MAX_CHANNELS:
        raise ValueError(f"channels must be in [2, {_lib.CSM_MAX_CHANNELS}], got {x.shape[1]}")
    return _avg_check_split(x.shape[2], nperseg, noverlap, navg)


def _csm_strides(x):
    """(channel_stride, batch_stride) of x[B, C, L]; the stride of a one-element axis is free."""
    B, C, L = x.shape
    cs = x.stride(1) if C > 1 else L
    bs = x.stride(0) if B > 1 else C * cs
    if cs < L or bs < C * cs:
        raise ValueError("x must not overlap itself: channel stride >= length and batch stride "
                         ">= channels * channel stride")
    return cs, bs


def csm_workspace(x, nperseg, noverlap, window, fs, scaling, detrend, navg):
    """A workspace for ``csm_out`` on ``x[B, C, L]`` (uint8, from torch's caching allocator):
    the spectra of every frame that enters a group, ``8 B F T C`` bytes."""
    _csm_check(x, nperseg, noverlap, navg)
    _, need = _avg_plan(x, (nperseg, noverlap, window, fs, scaling, detrend),
                        "csm_workspace_bytes", *x.shape, int(navg))
    return _avg_buffer(need, x.device)


def _csm_call(x, p, navg, outs, mask, workspace):
    _, G = _csm_check(x, p[0], p[1], navg)
    cs, bs = _csm_strides(x)
    B, C, L = x.shape
    outs = _avg_outs(x, outs, mask, (B, p[0] // 2 + 1, G, C, C), _CSM_DTYPES,
                     "csm complex64, coh float32")
    plan, need = _avg_plan(x, p, "csm_workspace_bytes", B, C, L, int(navg))
    ws, nbytes = _avg_workspace(workspace, need, x.device)
    _lib.check(_lib.lib().specenh_csm(
        plan.handle, _vp(x), B, C, L, cs, bs, int(navg), _vp(outs[0]), _vp(outs[1]), _vp(ws),
        nbytes, _st(x)), "csm")
    return outs


def _csm_out(x, nperseg, noverlap, window, fs, scaling, detrend, navg, csm, coh, workspace):
    _csm_call(x, (nperseg, noverlap, window, fs, scaling, detrend), navg, (csm, coh), 0, workspace)


def _csm(x, nperseg, noverlap, window, fs, scaling, detrend, navg, outputs):
    return _avg_results(x, _csm_call(x, (nperseg, noverlap, window, fs, scaling, detrend), navg,
                                     None, outputs, None), _CSM_DTYPES)


def _csm_fake(x, nperseg, noverlap, window, fs, scaling, detrend, navg, outputs):
    B, C, L = x.shape
    G = _avg_split(L, nperseg, noverlap, navg)[1]
    return _avg_fake(x, outputs, (B, nperseg // 2 + 1, G, C, C), _CSM_DTYPES)


_op(f"csm(Tensor x, {_SP_ARGS}, int outputs) -> (Tensor, Tensor)", _csm, _csm_fake)
_op(f"csm_out(Tensor x, {_SP_ARGS}, Tensor(a!)? csm, Tensor(b!)? coh, Tensor(c!)? workspace) "
    "-> ()", _csm_out, lambda *a: None)


# ---------------------------------------------------------------- bispectrum, bicoherence
_BISPEC_DTYPES = (torch.complex64, torch.float32)
_BISPEC_OUTS = "bispec complex64, bicoh float32"


def _bispec_bins(F, nbins):
    K = F if nbins <= 0 else int(nbins)
    if not 1 <= K <= F:
        raise ValueError(f"nbins must be in [1, {F}], got {nbins}")
    return K


def bispectrum_workspace(x, y, z, nperseg, noverlap, window, fs, scaling, detrend, navg):
    """A workspace for ``bispectrum_out`` on ``x[B, L]`` (and ``y``, ``z``; uint8, from torch's
    caching allocator): the spectra of every frame that enters a group of every distinct
    signal, ``8 B nsignals T F`` bytes."""
    _avg_check((("x", x), ("y", y), ("z", z)), nperseg, noverlap, navg)
    _, need = _avg_plan(x, (nperseg, noverlap, window, fs, scaling, detrend),
                        "bispectrum_workspace_bytes", x.shape[0],
                        _avg_distinct((x, y, z), [_avg_stride(v) for v in (x, y, z)]), x.shape[1],
                        int(navg))
    return _avg_buffer(need, x.device)


def _bispectrum_call(x, y, z, p, navg, nbins, outs, mask, workspace):
    _, G = _avg_check((("x", x), ("y", y), ("z", z)), p[0], p[1], navg)
    B, L = x.shape
    K = _bispec_bins(p[0] // 2 + 1, nbins)
    outs = _avg_outs(x, outs, mask, (B, G, K, K), _BISPEC_DTYPES, _BISPEC_OUTS)
    strides = [_avg_stride(v) for v in (x, y, z)]
    plan, need = _avg_plan(x, p, "bispectrum_workspace_bytes", B,
                           _avg_distinct((x, y, z), strides), L, int(navg))
    ws, nbytes = _avg_workspace(workspace, need, x.device)
    _lib.check(_lib.lib().specenh_bispectrum(
        plan.handle, _vp(x), _vp(y), _vp(z), B, L, *strides, int(navg), K, _vp(outs[0]),
        _vp(outs[1]), _vp(ws), nbytes, _st(x)), "bispectrum")
    return outs


def _bispectrum_out(x, y, z, nperseg, noverlap, window, fs, scaling, detrend, navg, nbins, bispec,
                    bicoh, workspace):
    _bispectrum_call(x, y, z, (nperseg, noverlap, window, fs, scaling, detrend), navg, nbins,
                     (bispec, bicoh), 0, workspace)


def _bispectrum(x, y, z, nperseg, noverlap, window, fs, scaling, detrend, navg, nbins, outputs):
    return _avg_results(x, _bispectrum_call(
        x, y, z, (nperseg, noverlap, window, fs, scaling, detrend), navg, nbins, None, outputs,
        None), _BISPEC_DTYPES)


def _bispectrum_fake(x, y, z, nperseg, noverlap, window, fs, scaling, detrend, navg, nbins,
                     outputs):
    G = _avg_split(x.shape[1], nperseg, noverlap, navg)[1]
    K = _bispec_bins(nperseg // 2 + 1, nbins)
    return _avg_fake(x, outputs, (x.shape[0], G, K, K), _BISPEC_DTYPES)


def _bispectrum_spectra_call(X, Y, Z, navg, nbins, outs, mask):
    B, T, F, G = _avg_spectra((("X", X), ("Y", Y), ("Z", Z)), navg)
    K = _bispec_bins(F, nbins)
    outs = _avg_outs(X, outs, mask, (B, G, K, K), _BISPEC_DTYPES, _BISPEC_OUTS)
    same = X.data_ptr()  # the same spectra under another tensor: the auto case
    _lib.check(_lib.lib().specenh_bispectrum_spectra(
        _vp(X), _vp(None if Y is None or Y.data_ptr() == same else Y),
        _vp(None if Z is None or Z.data_ptr() == same else Z), B, T, F, int(navg), K,
        _vp(outs[0]), _vp(outs[1]), _st(X)), "bispectrum_spectra")
    return outs


def _bispectrum_spectra_out(X, Y, Z, navg, nbins, bispec, bicoh):
    _bispectrum_spectra_call(X, Y, Z, navg, nbins, (bispec, bicoh), 0)


def _bispectrum_spectra(X, Y, Z, navg, nbins, outputs):
    return _avg_results(X, _bispectrum_spectra_call(X, Y, Z, navg, nbins, None, outputs),
                        _BISPEC_DTYPES)


def _bispectrum_spectra_fake(X, Y, Z, navg, nbins, outputs):
    B, _, F, G = _avg_spectra((("X", X), ("Y", Y), ("Z", Z)), navg)
    K = _bispec_bins(F, nbins)
    return _avg_fake(X, outputs, (B, G, K, K), _BISPEC_DTYPES)


_op(f"bispectrum(Tensor x, Tensor? y, Tensor? z, {_SP_ARGS}, int nbins, int outputs) -> "
    "(Tensor, Tensor)", _bispectrum, _bispectrum_fake)
_op(f"bispectrum_out(Tensor x, Tensor? y, Tensor? z, {_SP_ARGS}, int nbins, "
    "Tensor(a!)? bispec, Tensor(b!)? bicoh, Tensor(c!)? workspace) -> ()", _bispectrum_out,
    lambda *a: None)
_op("bispectrum_spectra(Tensor X, Tensor? Y, Tensor? Z, int navg, int nbins, int outputs) -> "
    "(Tensor, Tensor)", _bispectrum_spectra, _bispectrum_spectra_fake)
_op("bispectrum_spectra_out(Tensor X, Tensor? Y, Tensor? Z, int navg, int nbins, "
    "Tensor(a!)? bispec, Tensor(b!)? bicoh) -> ()", _bispectrum_spectra_out, lambda *a: None)


# ---------------------------------------------------------------- wavenumber-frequency spectrum
def _wn_nk(nk):
    nk = int(nk)
    if nk % 2 or not _lib.WAVENUMBER_MIN_NK <= nk <= _lib.WAVENUMBER_MAX_NK:
        raise ValueError(f"nk must be even and in [{_lib.WAVENUMBER_MIN_NK}, "
                         f"{_lib.WAVENUMBER_MAX_NK}], got {nk}")
    return nk


def wavenumber_workspace(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg):
    """A workspace for ``wavenumber_spectrum_out`` on ``x[B, L]`` and ``y`` (uint8, from torch's
    caching allocator): the spectra of every frame that enters a group of every distinct
    signal, ``8 B nsignals T F`` bytes."""
    _avg_check((("x", x), ("y", y)), nperseg, noverlap, navg)
    _, need = _avg_plan(x, (nperseg, noverlap, window, fs, scaling, detrend),
                        "wavenumber_workspace_bytes", x.shape[0],
                        _avg_distinct((x, y), (_avg_stride(x), _avg_stride(y))), x.shape[1],
                        int(navg))
    return _avg_buffer(need, x.device)


def _wavenumber_spectrum_call(x, y, p, navg, nk, skf, workspace):
    """skf None: allocated. Returns it."""
    _, G = _avg_check((("x", x), ("y", y)), p[0], p[1], navg)
    B, L = x.shape
    K = _wn_nk(nk)
    skf, = _avg_outs(x, None if skf is None else (skf,), 1, (B, G, p[0] // 2 + 1, K), _F32,
                     "skf float32")
    strides = (_avg_stride(x), _avg_stride(y))
    plan, need = _avg_plan(x, p, "wavenumber_workspace_bytes", B, _avg_distinct((x, y), strides),
                           L, int(navg))
    ws, nbytes = _avg_workspace(workspace, need, x.device)
    _lib.check(_lib.lib().specenh_wavenumber_spectrum(
        plan.handle, _vp(x), _vp(y), B, L, *strides, int(navg), K, _vp(skf), _vp(ws), nbytes,
        _st(x)), "wavenumber_spectrum")
    return skf


def _wavenumber_spectrum_out(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, nk,
                             skf, workspace):
    _wavenumber_spectrum_call(x, y, (nperseg, noverlap, window, fs, scaling, detrend), navg, nk,
                              skf, workspace)


def _wavenumber_spectrum(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, nk):
    return _wavenumber_spectrum_call(x, y, (nperseg, noverlap, window, fs, scaling, detrend), navg,
                                     nk, None, None)


def _wavenumber_spectrum_fake(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, nk):
    G = _avg_split(x.shape[1], nperseg, noverlap, navg)[1]
    return x.new_empty((x.shape[0], G, nperseg // 2 + 1, _wn_nk(nk)), dtype=torch.float32)


def _wn_spectra_shape(X, Y, navg, nk):
    B, _, F, G = _avg_spectra((("X", X), ("Y", Y)), navg)
    return B, G, F, _wn_nk(nk)


def _wavenumber_spectra_call(X, Y, navg, nk, skf):
    """skf None: allocated. Returns it."""
    shape = _wn_spectra_shape(X, Y, navg, nk)
    skf, = _avg_outs(X, None if skf is None else (skf,), 1, shape, _F32, "skf float32")
    _lib.check(_lib.lib().specenh_wavenumber_spectra(
        _vp(X), _vp(Y), X.shape[0], X.shape[1], X.shape[2], int(navg), shape[3], _vp(skf),
        _st(X)), "wavenumber_spectra")
    return skf


def _wavenumber_spectra_out(X, Y, navg, nk, skf):
    _wavenumber_spectra_call(X, Y, navg, nk, skf)


def _wavenumber_spectra(X, Y, navg, nk):
    return _wavenumber_spectra_call(X, Y, navg, nk, None)


def _wavenumber_spectra_fake(X, Y, navg, nk):
    return X.new_empty(_wn_spectra_shape(X, Y, navg, nk), dtype=torch.float32)


_op(f"wavenumber_spectrum(Tensor x, Tensor y, {_SP_ARGS}, int nk) -> Tensor",
    _wavenumber_spectrum, _wavenumber_spectrum_fake)
_op(f"wavenumber_spectrum_out(Tensor x, Tensor y, {_SP_ARGS}, int nk, Tensor(a!) skf, "
    "Tensor(b!)? workspace) -> ()", _wavenumber_spectrum_out, lambda *a: None)
_op("wavenumber_spectra(Tensor X, Tensor Y, int navg, int nk) -> Tensor", _wavenumber_spectra,
    _wavenumber_spectra_fake)
_op("wavenumber_spectra_out(Tensor X, Tensor Y, int navg, int nk, Tensor(a!) skf) -> ()",
    _wavenumber_spectra_out, lambda *a: None)


# ---------------------------------------------------------------- block-averaged correlation
def _corr_check(x, y, nperseg, noverlap, navg, maxlag, mode):
    if nperseg == 4096:
        raise NotImplementedError("correlation: nperseg = 4096 is not supported (the padded "
                                  "transform would be 8192 points); nperseg must be a power of "
                                  "two in [64, 2048]")
    if nperseg < 64 or nperseg > _lib.CORR_MAX_NPERSEG or nperseg & (nperseg - 1):
        raise NotImplementedError("correlation: nperseg must be a power of two in [64, 2048]")
    if not 0 <= maxlag < nperseg:
        raise ValueError(f"maxlag must be in [0, nperseg - 1], got {maxlag}")
    if mode not in (_lib.CORR_RAW, _lib.CORR_COEFF):
        raise ValueError(f"mode must be {_lib.CORR_RAW} (raw) or {_lib.CORR_COEFF} (coeff)")
    return _avg_check((("x", x), ("y", y)), nperseg, noverlap, navg)


def correlation_workspace(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, maxlag):
    """A workspace for ``correlation_out`` on ``x[B, L]`` and ``y`` (uint8, from torch's caching
    allocator; one byte when none is needed): one record of ``8 (nperseg + 3)`` bytes per chunk
    of 32 frames when a group is longer than a chunk."""
    _corr_check(x, y, nperseg, noverlap, navg, maxlag, _lib.CORR_RAW)
    _, need = _avg_plan(x, (nperseg, noverlap, window, fs, scaling, detrend),
                        "correlation_workspace_bytes", x.shape[0], x.shape[1], int(navg),
                        int(maxlag), may_be_zero=True)
    return _avg_buffer(need, x.device)


def _correlation_call(x, y, p, navg, maxlag, mode, outs, workspace):
    """outs: (out, energies or None), or None: both are allocated. Returns them."""
    _, G = _corr_check(x, y, p[0], p[1], navg, maxlag, mode)
    B, L = x.shape
    shape = (B, G, 2 * int(maxlag) + 1)
    out, = _avg_outs(x, outs and outs[:1], 1, shape, _F32, "out float32")
    energies = None
    if outs is None or outs[1] is not None:  # energies are optional for the caller's buffers
        energies, = _avg_outs(x, outs and outs[1:], 1, shape[:2] + (2,), _F32,
                              "energies float32")
    plan, need = _avg_plan(x, p, "correlation_workspace_bytes", B, L, int(navg), int(maxlag),
                           may_be_zero=True)
    ws, nbytes = _avg_workspace(workspace, need, x.device)
    _lib.check(_lib.lib().specenh_correlation(
        plan.handle, _vp(x), _vp(y), B, L, _avg_stride(x), _avg_stride(y), int(navg), int(maxlag),
        int(mode), _vp(out), _vp(energies), _vp(ws), nbytes, _st(x)), "correlation")
    return out, energies


def _correlation_out(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, maxlag, mode,
                     out, energies, workspace):
    _correlation_call(x, y, (nperseg, noverlap, window, fs, scaling, detrend), navg, maxlag, mode,
                      (out, energies), workspace)


def _correlation(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, maxlag, mode):
    return _correlation_call(x, y, (nperseg, noverlap, window, fs, scaling, detrend), navg, maxlag,
                             mode, None, None)


def _correlation_fake(x, y, nperseg, noverlap, window, fs, scaling, detrend, navg, maxlag, mode):
    _, G = _corr_check(x, y, nperseg, noverlap, navg, maxlag, mode)
    return (x.new_empty((x.shape[0], G, 2 * int(maxlag) + 1), dtype=torch.float32),
            x.new_empty((x.shape[0], G, 2), dtype=torch.float32))


# the schema calls the mode `normalize`: torch's functionalisation of a mutable operator passes
# a keyword `mode` of its own
_op(f"correlation(Tensor x, Tensor y, {_SP_ARGS}, int maxlag, int normalize) -> "
    "(Tensor, Tensor)", _correlation, _correlation_fake)
_op(f"correlation_out(Tensor x, Tensor y, {_SP_ARGS}, int maxlag, int normalize, "
    "Tensor(a!) out, Tensor(b!)? energies, Tensor(c!)? workspace) -> ()", _correlation_out,
    lambda *a: None)


# ---------------------------------------------------------------- complex FIR filter bank
_FB_KINDS = (_lib.FB_COMPLEX, _lib.FB_POWER, _lib.FB_POWER_MEAN)


def filterbank_nfft(lmax: int, nfft=None) -> int:
    """The transform length of a bank whose longest filter has the half length ``lmax``:
    ``nfft`` checked, or (None / 0) the default, the smallest allowed power of two
    ``>= 4 lmax`` and at least 1024 (specenh_filterbank_nfft)."""
    return _lib.check(_lib.lib().specenh_filterbank_nfft(int(lmax), int(nfft or 0)),
                      "filterbank_nfft")


def filterbank_tables(taps, half_lengths, nfft, device="cuda") -> torch.Tensor:
    """The tables of a bank as the operators take them, complex64 ``[S + 1, nfft]`` on
    ``device``: row ``s`` the DFT of filter ``s`` wrapped circularly, the last row the
    twiddles (specenh_filterbank_tables: host, fp64, rounded once). ``taps``: the filters one
    after the other, complex, filter ``s`` as its ``2 L_s + 1`` taps from ``m = -L_s``;
    ``half_lengths``: the ``L_s``."""
    hl = np.ascontiguousarray(half_lengths, dtype=np.intc).reshape(-1)
    h = np.ascontiguousarray(taps, dtype=np.complex128).reshape(-1)
    S = int(hl.shape[0])
    if S < 1:
        raise ValueError("a filter bank needs at least one filter")
    if (hl < 0).any() or h.shape[0] != int((2 * hl.astype(np.int64) + 1).sum()):
        raise ValueError("taps must hold 2 L_s + 1 values for every half length L_s >= 0")
    nfft = int(nfft)
    L = _lib.lib()
    need = int(L.specenh_filterbank_tables_bytes(S, nfft))
    if need == 0:
        _lib.check(_lib.SPECENH_EINVAL, "filterbank_tables")
    host = np.empty((S + 1, nfft), dtype=np.complex64)
    assert host.nbytes == need
    _lib.check(L.specenh_filterbank_tables(
        S, hl.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
        h.view(np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)), nfft,
        ctypes.c_void_p(host.ctypes.data)), "filterbank_tables")
    return torch.from_numpy(host).to(device)


def _fb_check(x, tables, lmax, hop, kind):
    """(filters, nfft, outputs per filter) of a call; plain arithmetic, on meta tensors too."""
    if x.dim() != 2 or x.stride(1) != 1 or x.dtype != torch.float32:
        raise ValueError("x must be float32 [batch, length] with unit stride along length")
    if (tables.dim() != 2 or tables.dtype != torch.complex64 or tables.shape[0] < 2
            or not tables.is_contiguous() or tables.device != x.device):
        raise ValueError("tables must be contiguous complex64 [filters + 1, nfft] on x's device")
    S, nfft = tables.shape[0] - 1, tables.shape[1]
    if nfft not in _lib.FB_NFFT:
        raise ValueError(f"nfft must be one of {_lib.FB_NFFT}, got {nfft}")
    if not 0 <= lmax <= _lib.FB_MAX_HALF:
        raise ValueError(f"lmax must be in [0, {_lib.FB_MAX_HALF}], got {lmax}")
    if hop < 1:
        raise ValueError(f"hop must be >= 1, got {hop}")
    if 2 * lmax + hop > nfft:
        raise ValueError(f"2 lmax + hop must not exceed nfft: 2 * {lmax} + {hop} > {nfft}")
    if kind not in _FB_KINDS:
        raise ValueError(f"kind must be {_lib.FB_COMPLEX} (complex), {_lib.FB_POWER} (power) or "
                         f"{_lib.FB_POWER_MEAN} (mean power)")
    L = x.shape[1]
    if L < 1:
        raise ValueError("length must be >= 1")
    if kind == _lib.FB_POWER_MEAN:
        if L < hop:
            raise ValueError(f"signal of {L} samples is shorter than hop = {hop}")
        return S, nfft, L // hop
    return S, nfft, (L - 1) // hop + 1


def _fb_dtype(kind):
    return torch.complex64 if kind == _lib.FB_COMPLEX else torch.float32


def _filterbank_out(x, tables, lmax, hop, kind, out):
    S, nfft, To = _fb_check(x, tables, lmax, hop, kind)
    B, L = x.shape
    shape = (B, S, To)
    if (out.shape != shape or out.dtype != _fb_dtype(kind) or not out.is_contiguous()
            or out.device != x.device):
        raise ValueError(f"out must be contiguous {_fb_dtype(kind)} {shape} on x's device")
    _lib.check(_lib.lib().specenh_filterbank(
        _vp(tables), S, nfft, int(lmax), _vp(x), B, L, _avg_stride(x), int(hop), int(kind),
        _vp(out), _st(x)), "filterbank")


def _filterbank(x, tables, lmax, hop, kind):
    S, _, To = _fb_check(x, tables, lmax, hop, kind)
    out = torch.empty((x.shape[0], S, To), dtype=_fb_dtype(kind), device=x.device)
    _filterbank_out(x, tables, lmax, hop, kind, out)
    return out


def _filterbank_fake(x, tables, lmax, hop, kind):
    S, _, To = _fb_check(x, tables, lmax, hop, kind)
    return x.new_empty((x.shape[0], S, To), dtype=_fb_dtype(kind))


# `kind` is the C entry's mode (see the note on `normalize` above)
_op("filterbank(Tensor x, Tensor tables, int lmax, int hop, int kind) -> Tensor", _filterbank,
    _filterbank_fake)
_op("filterbank_out(Tensor x, Tensor tables, int lmax, int hop, int kind, Tensor(a!) out) -> ()",
    _filterbank_out, lambda *a: None)


# ---------------------------------------------------------------- cross spectrum of a pair
def _fbx_check(x, y, tables, lmax, hop, kind):
    """(filters, nfft, outputs per filter) of a call; plain arithmetic, on meta tensors too."""
    if kind not in (_lib.XWT_POINT, _lib.XWT_MEAN):
        raise ValueError(f"kind must be {_lib.XWT_POINT} (every hop-th sample) or "
                         f"{_lib.XWT_MEAN} (hop-window means)")
    if (y.dim() != 2 or y.stride(1) != 1 or y.dtype != torch.float32 or y.shape != x.shape
            or y.device != x.device):
        raise ValueError("y must be float32 [batch, length] like x, on x's device, with unit "
                         "stride along length")
    return _fb_check(x, tables, lmax, hop,
                     _lib.FB_POWER_MEAN if kind == _lib.XWT_MEAN else _lib.FB_POWER)


def filterbank_cross_chunk(nscales, nfft, lmax, batch, length, hop, kind, cus=0) -> int:
    """The filters a workgroup of the cross kernel loops over for this launch on a device of
    ``cus`` compute units (0: the current device); host arithmetic
    (specenh_filterbank_cross_chunk). The outputs do not depend on it."""
    return _lib.check(_lib.lib().specenh_filterbank_cross_chunk(
        int(nscales), int(nfft), int(lmax), int(batch), int(length), int(hop), int(kind),
        int(cus)), "filterbank_cross_chunk")


def _filterbank_cross_out(x, y, tables, lmax, hop, kind, sxy, sxx, syy):
    S, nfft, To = _fbx_check(x, y, tables, lmax, hop, kind)
    B, L = x.shape
    shape = (B, S, To)
    if (sxx is None) != (syy is None):
        raise ValueError("sxx and syy must be both given or both None")
    for t, name, dt in ((sxy, "sxy", torch.complex64), (sxx, "sxx", torch.float32),
                        (syy, "syy", torch.float32)):
        if t is not None and (t.shape != shape or t.dtype != dt or not t.is_contiguous()
                              or t.device != x.device):
            raise ValueError(f"{name} must be contiguous {dt} {shape} on x's device")
    _lib.check(_lib.lib().specenh_filterbank_cross(
        _vp(tables), S, nfft, int(lmax), _vp(x), _vp(y), B, L, _avg_stride(x), _avg_stride(y),
        int(hop), int(kind), _vp(sxy), _vp(sxx), _vp(syy), _st(x)), "filterbank_cross")


def _filterbank_cross(x, y, tables, lmax, hop, kind):
    S, _, To = _fbx_check(x, y, tables, lmax, hop, kind)
    shape = (x.shape[0], S, To)
    sxy = torch.empty(shape, dtype=torch.complex64, device=x.device)
    sxx = torch.empty(shape, dtype=torch.float32, device=x.device)
    syy = torch.empty(shape, dtype=torch.float32, device=x.device)
    _filterbank_cross_out(x, y, tables, lmax, hop, kind, sxy, sxx, syy)
    return sxy, sxx, syy


def _filterbank_cross_fake(x, y, tables, lmax, hop, kind):
    S, _, To = _fbx_check(x, y, tables, lmax, hop, kind)
    shape = (x.shape[0], S, To)
    return (x.new_empty(shape, dtype=torch.complex64), x.new_empty(shape), x.new_empty(shape))


_op("filterbank_cross(Tensor x, Tensor y, Tensor tables, int lmax, int hop, int kind) -> "
    "(Tensor, Tensor, Tensor)", _filterbank_cross, _filterbank_cross_fake)
_op("filterbank_cross_out(Tensor x, Tensor y, Tensor tables, int lmax, int hop, int kind, "
    "Tensor(a!) sxy, Tensor(b!)? sxx, Tensor(c!)? syy) -> ()", _filterbank_cross_out,
    lambda *a: None)


# ---------------------------------------------------------------- Hermitian eigensolver
def _eig_check(a, k):
    if a.dtype != torch.complex64 or a.dim() < 2 or a.shape[-1] != a.shape[-2]:
        raise ValueError("a must be complex64 [..., n, n]")
    n = a.shape[-1]
    if not 2 <= n <= _lib.HERM_EIG_MAX_N:
        raise ValueError(f"n must be in [2, {_lib.HERM_EIG_MAX_N}], got {n}")
    if not 0 <= k <= n:
        raise ValueError(f"k must be in [0, {n}], got {k}")


def _eig_layout(a):
    """(a, count, matrix_stride): ``a`` as it is when every matrix is contiguous and the
    leading axes step through memory by one stride >= n * n, else its contiguous copy."""
    n = a.shape[-1]
    lead = a.shape[:-2]
    count = int(np.prod(lead, dtype=np.int64)) if lead else 1
    ok = a.stride(-1) == 1 and a.stride(-2) == n
    ms = n * n
    dims = [(s, st) for s, st in zip(lead, a.stride()[:-2]) if s != 1]
    if ok and count > 1 and dims:
        ms = dims[-1][1]
        for (_, st0), (s1, st1) in zip(dims[:-1], dims[1:]):
            ok = ok and st0 == st1 * s1
        ok = ok and ms >= n * n
    if not ok:
        a, ms = a.contiguous(), n * n
    return a, count, ms


def _herm_eig_out(a, k, w, v, sweeps):
    _eig_check(a, k)
    n, lead = a.shape[-1], tuple(a.shape[:-2])
    if w is None and sweeps is None and k == 0:
        raise ValueError("no output requested")
    if k > 0 and v is None:
        raise ValueError("v is needed for k > 0")
    for o, shape, dt, name in ((w, lead + (n,), torch.float32, "w float32"),
                               (v, lead + (k, n), torch.complex64, "v complex64"),
                               (sweeps, lead, torch.int32, "sweeps int32")):
        if o is not None and (tuple(o.shape) != shape or o.dtype != dt or not o.is_contiguous()
                              or o.device != a.device):
            raise ValueError(f"{name} must be contiguous {shape} on a's device")
    a, count, ms = _eig_layout(a)
    if count == 0:
        return
    _lib.check(_lib.lib().specenh_herm_eig(
        _vp(a), count, n, ms, int(k), _vp(w), _vp(v if k > 0 else None), _vp(sweeps), _st(a)),
        "herm_eig")


def _herm_eig(a, k):
    _eig_check(a, k)
    n, lead = a.shape[-1], tuple(a.shape[:-2])
    w = torch.empty(lead + (n,), dtype=torch.float32, device=a.device)
    v = torch.empty(lead + (k, n), dtype=torch.complex64, device=a.device)
    _herm_eig_out(a, k, w, v, None)
    return w, v


def _herm_eig_fake(a, k):
    n, lead = a.shape[-1], tuple(a.shape[:-2])
    return (a.new_empty(lead + (n,), dtype=torch.float32),
            a.new_empty(lead + (k, n), dtype=torch.complex64))


_op("herm_eig(Tensor a, int k) -> (Tensor, Tensor)", _herm_eig, _herm_eig_fake)
_op("herm_eig_out(Tensor a, int k, Tensor(a!)? w, Tensor(b!)? v, Tensor(c!)? sweeps) -> ()",
    _herm_eig_out, lambda *a: None)


# ---------------------------------------------------------------- steered-response spectra
def _steer_check(V, w, A, post, scale_table):
    """Rows V[..., M, C] complex64, weights w[..., M] float32 or None, table A[K, C] or
    [Fa, K, C] complex64 (then V is [..., Fa, G, M, C]); (lead, M, C, K, a_count, a_inner)."""
    if V.dtype != torch.complex64 or V.dim() < 2:
        raise ValueError("V must be complex64 [..., M, C]")
    M, C = V.shape[-2], V.shape[-1]
    lead = tuple(V.shape[:-2])
    if M < 1 or not 1 <= C <= _lib.STEER_MAX_CHANNELS:
        raise ValueError(f"V must hold at least one row of 1 to {_lib.STEER_MAX_CHANNELS} "
                         f"channels, got [M, C] = [{M}, {C}]")
    if (A.dtype != torch.complex64 or A.dim() not in (2, 3) or A.shape[-1] != C
            or not A.is_contiguous() or A.device != V.device):
        raise ValueError(f"A must be contiguous complex64 [K, {C}] or [F, K, {C}] on V's device")
    K = A.shape[-2]
    if not 1 <= K <= _lib.STEER_MAX_NSTEER:
        raise ValueError(f"K must be in [1, {_lib.STEER_MAX_NSTEER}], got {K}")
    a_count, a_inner = 1, 1
    if A.dim() == 3:
        if len(lead) < 2 or lead[-2] != A.shape[0]:
            raise ValueError("a table per bin A[F, K, C] needs V[..., F, G, M, C]")
        a_count, a_inner = A.shape[0], lead[-1]
    if w is not None and (w.dtype != torch.float32 or tuple(w.shape) != lead + (M,)
                          or w.device != V.device):
        raise ValueError(f"w must be float32 {lead + (M,)} on V's device")
    if scale_table is not None and (scale_table.dtype != torch.float64
                                    or tuple(scale_table.shape) != (a_count,)
                                    or scale_table.device != V.device):
        raise ValueError(f"scale_table must be float64 [{a_count}] on V's device")
    if not _lib.STEER_SUM <= post <= _lib.STEER_MUSIC:
        raise ValueError(f"post must be in [0, 3], got {post}")
    return lead, M, C, K, a_count, a_inner


def _steer_layout(V):
    """(V, count, matrix_stride, row_stride): ``V`` as it is when its rows have unit stride and
    the leading axes step through memory by one stride that clears a matrix, else its
    contiguous copy."""
    M, C = V.shape[-2], V.shape[-1]
    lead = V.shape[:-2]
    count = int(np.prod(lead, dtype=np.int64)) if lead else 1
    rs = V.stride(-2) if M > 1 else C
    ok = (V.stride(-1) == 1 or C == 1) and rs >= C
    extent = (M - 1) * rs + C
    ms = extent
    dims = [(s, st) for s, st in zip(lead, V.stride()[:-2]) if s != 1]
    if ok and count > 1 and dims:
        ms = dims[-1][1]
        for (_, st0), (s1, st1) in zip(dims[:-1], dims[1:]):
            ok = ok and st0 == st1 * s1
        ok = ok and ms >= extent
    if not ok:
        V = V.contiguous()
        ms, rs = M * C, C
    return V, count, ms, rs


def _steered_power_out(V, w, A, post, scale, conj_a, scale_table, out):
    lead, M, C, K, a_count, a_inner = _steer_check(V, w, A, post, scale_table)
    if (tuple(out.shape) != lead + (K,) or out.dtype != torch.float32 or not out.is_contiguous()
            or out.device != V.device):
        raise ValueError(f"out must be contiguous float32 {lead + (K,)} on V's device")
    V, count, ms, rs = _steer_layout(V)
    if count == 0:
        return
    if w is not None:
        w = w.contiguous()
    _lib.check(_lib.lib().specenh_steered_power(
        _vp(V), _vp(w), _vp(A), count, M, C, K, ms, rs, a_count, a_inner, int(bool(conj_a)),
        float(scale), _vp(scale_table), int(post), _vp(out), _st(V)), "steered_power")


def _steered_power(V, w, A, post, scale, conj_a, scale_table):
    lead, _, _, K, _, _ = _steer_check(V, w, A, post, scale_table)
    out = torch.empty(lead + (K,), dtype=torch.float32, device=V.device)
    _steered_power_out(V, w, A, post, scale, conj_a, scale_table, out)
    return out


def _steered_power_fake(V, w, A, post, scale, conj_a, scale_table):
    return V.new_empty(tuple(V.shape[:-2]) + (A.shape[-2],), dtype=torch.float32)


_STEER_ARGS = "Tensor V, Tensor? w, Tensor A, int post, float scale, bool conj_a, " \
              "Tensor? scale_table"
_op(f"steered_power({_STEER_ARGS}) -> Tensor", _steered_power, _steered_power_fake)
_op(f"steered_power_out({_STEER_ARGS}, Tensor(a!) out) -> ()", _steered_power_out,
    lambda *a: None)


def _array_spectrum_check(x, nperseg, noverlap, navg, A):
    if x.dim() != 3 or x.dtype != torch.float32 or x.stride(2) != 1:
        raise ValueError("x must be float32 [batch, channels, length] with unit stride along "
                         "length")
    C, F = x.shape[1], nperseg // 2 + 1
    if not 1 <= C <= _lib.STEER_MAX_CHANNELS:
        raise ValueError(f"channels must be in [1, {_lib.STEER_MAX_CHANNELS}], got {C}")
    if (A.dtype != torch.complex64 or A.dim() not in (2, 3) or A.shape[-1] != C
            or (A.dim() == 3 and A.shape[0] != F) or not A.is_contiguous()
            or A.device != x.device):
        raise ValueError(f"A must be contiguous complex64 [K, {C}] or [{F}, K, {C}] on x's "
                         "device")
    K = A.shape[-2]
    if not 1 <= K <= _lib.STEER_MAX_NSTEER:
        raise ValueError(f"K must be in [1, {_lib.STEER_MAX_NSTEER}], got {K}")
    return _avg_check_split(x.shape[2], nperseg, noverlap, navg)[1], K


def array_spectrum_workspace(x, nperseg, noverlap, window, fs, scaling, detrend, navg):
    """A workspace for ``array_spectrum_out`` on ``x[B, C, L]`` (uint8, from torch's caching
    allocator): the spectra of every frame that enters a group, ``8 B F T C`` bytes."""
    _, need = _avg_plan(x, (nperseg, noverlap, window, fs, scaling, detrend),
                        "array_spectrum_workspace_bytes", *x.shape, int(navg))
    return _avg_buffer(need, x.device)


def _array_spectrum_out(x, nperseg, noverlap, window, fs, scaling, detrend, navg, A, out,
                        workspace):
    G, K = _array_spectrum_check(x, nperseg, noverlap, navg, A)
    cs, bs = _csm_strides(x)
    B, C, L = x.shape
    shape = (B, nperseg // 2 + 1, G, K)
    if (tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous()
            or out.device != x.device):
        raise ValueError(f"out must be contiguous float32 {shape} on x's device")
    plan, need = _avg_plan(x, (nperseg, noverlap, window, fs, scaling, detrend),
                           "array_spectrum_workspace_bytes", B, C, L, int(navg))
    ws, nbytes = _avg_workspace(workspace, need, x.device)
    _lib.check(_lib.lib().specenh_array_spectrum(
        plan.handle, _vp(x), B, C, L, cs, bs, int(navg), _vp(A), K, int(A.dim() == 3), _vp(out),
        _vp(ws), nbytes, _st(x)), "array_spectrum")


_op(f"array_spectrum_out(Tensor x, {_SP_ARGS}, Tensor A, Tensor(a!) out, "
    "Tensor(b!)? workspace) -> ()", _array_spectrum_out, lambda *a: None)


# ---------------------------------------------------------------- SVD denoiser
def _bstride(A):
    """Batch stride for the C-ABI: a batch of one may carry any stride (e.g. 0 from a numpy
    [None] view); the kernels only need it to reach matrix b for b >= 1."""
    return A.stride(0) if A.shape[0] > 1 else A.shape[1] * A.shape[2]


def _svd_check(A):
    if A.dim() != 3 or A.dtype != torch.float32 or A.stride(2) != 1 or A.stride(1) != A.shape[2]:
        raise ValueError("A must be float32 [batch, m, n] with row-major matrices")


def _svd_out(A, start, stop, out):
    _svd_check(A)
    B, m, n = A.shape
    if out.shape != A.shape or not out.is_contiguous() or out.device != A.device:
        raise ValueError("out must be a contiguous [B, m, n] tensor on A's device")
    L = _lib.lib()
    ws = torch.empty(max(16, int(L.specenh_svd_denoise_workspace_bytes(B, m, n, start, stop))),
                     dtype=torch.uint8, device=A.device)
    _lib.check(L.specenh_svd_denoise_ex(_vp(A), B, m, n, _bstride(A), start, stop, _vp(out),
                                        _code(out), _vp(ws), _st(A)), "svd_denoise")


def _svd(A, start, stop, out_dtype):
    out = torch.empty(A.shape, dtype=out_dtype, device=A.device)
    _svd_out(A, start, stop, out)
    return out


def _svd_opt_out(A, kind, out, num_sing, median):
    _svd_check(A)
    B, m, n = A.shape
    if (out.shape != A.shape or out.dtype != torch.float32 or not out.is_contiguous()
            or out.device != A.device):
        raise ValueError("out must be a contiguous float32 [B, m, n] tensor on A's device")
    if (num_sing.numel() != B or num_sing.dtype != torch.int32 or median.numel() != B
            or median.dtype != torch.float64 or num_sing.device != A.device
            or median.device != A.device):
        raise ValueError("num_sing / median must be int32 / float64 [B] tensors on A's device")
    L = _lib.lib()
    ws = torch.empty(max(16, int(L.specenh_svd_optimal_workspace_bytes(B, m, n))),
                     dtype=torch.uint8, device=A.device)
    _lib.check(L.specenh_svd_denoise_optimal(_vp(A), B, m, n, _bstride(A), int(kind), _vp(out),
                                             _vp(num_sing), _vp(median), _vp(ws), _st(A)),
               "svd_denoise_optimal")


def _svd_opt(A, mode):
    out = torch.empty(A.shape, dtype=torch.float32, device=A.device)
    ns = torch.empty(A.shape[0], dtype=torch.int32, device=A.device)
    med = torch.empty(A.shape[0], dtype=torch.float64, device=A.device)
    _svd_opt_out(A, mode, out, ns, med)
    return out, ns, med


_op("svd_denoise(Tensor A, int start, int stop, ScalarType out_dtype) -> Tensor", _svd,
    lambda A, start, stop, out_dtype: A.new_empty(A.shape, dtype=out_dtype))
_op("svd_denoise_out(Tensor A, int start, int stop, Tensor(a!) out) -> ()", _svd_out,
    lambda *a: None)
_op("svd_denoise_optimal(Tensor A, int mode) -> (Tensor, Tensor, Tensor)", _svd_opt,
    lambda A, mode: (A.new_empty(A.shape), A.new_empty((A.shape[0],), dtype=torch.int32),
                     A.new_empty((A.shape[0],), dtype=torch.float64)))
# (the mode argument is "kind" here: auto_functionalized reserves the name "mode")
_op("svd_denoise_optimal_out(Tensor A, int kind, Tensor(a!) out, Tensor(b!) num_sing, "
    "Tensor(c!) median) -> ()", _svd_opt_out, lambda *a: None)


# ---------------------------------------------------------------- convolutions
def _conv_out(x, w, bias, kh, kw, cout, stride, pad_t, pad_l, in_dil, oh, ow, act, mask,
              logits, out, pool, argmax):
    if x.dim() != 4:
        raise ValueError("x must be NHWC [N, H, W, C]")
    _need(x, "x")
    _need(out, "out")
    N, IH, IW, C = x.shape
    dt = _code(x)
    if w.dtype != x.dtype or w.numel() != cout * kh * kw * C:
        raise ValueError("w must be the [CO][KH][KW][C] GEMM weights in x's dtype")
    _need(w, "w")
    oshape = (N, oh // 2, ow // 2, cout) if pool else (N, oh, ow, cout)
    if tuple(out.shape) != oshape or out.dtype not in (x.dtype, torch.float32):
        raise ValueError(f"out must be {oshape} in x's dtype or float32")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != cout):
        raise ValueError("bias must be float32 [CO]")
    if mask is not None and (mask.dtype != x.dtype or mask.numel() != N * oh * ow * cout):
        raise ValueError("mask must match the output (compute dtype)")
    if logits is not None and (logits.dtype != torch.float32 or
                               logits.numel() != N * oh * ow * cout):
        raise ValueError("logits must be float32 [N, OH, OW, CO]")
    if argmax is not None and (argmax.dtype != torch.uint8 or tuple(argmax.shape) != oshape):
        raise ValueError("argmax must be uint8 like the pooled output")
    out_f32 = int(out.dtype == torch.float32)
    _lib.check(_lib.lib().specenh_conv2d(
        dt, _vp(x), N, IH, IW, C, _vp(w), kh, kw, cout, _vp(bias), stride, pad_t, pad_l, in_dil,
        oh, ow, act, _vp(mask), _vp(logits), _vp(out), out_f32, int(pool), _vp(argmax), _st(x)),
        "conv2d")


def _conv(x, w, bias, kh, kw, cout, stride, pad_t, pad_l, in_dil, oh, ow, act):
    out = torch.empty((x.shape[0], oh, ow, cout), dtype=x.dtype, device=x.device)
    _conv_out(x, w, bias, kh, kw, cout, stride, pad_t, pad_l, in_dil, oh, ow, act, None, None,
              out, False, None)
    return out


_CONV_ARGS = "int kh, int kw, int cout, int stride, int pad_t, int pad_l, int in_dil, int oh, " \
             "int ow, int act"
_op(f"conv2d(Tensor x, Tensor w, Tensor? bias, {_CONV_ARGS}) -> Tensor", _conv,
    lambda x, w, bias, kh, kw, cout, stride, pad_t, pad_l, in_dil, oh, ow, act:
    x.new_empty((x.shape[0], oh, ow, cout)))
_op(f"conv2d_out(Tensor x, Tensor w, Tensor? bias, {_CONV_ARGS}, Tensor? mask, "
    "Tensor(a!)? logits, Tensor(b!) out, bool pool, Tensor(c!)? argmax) -> ()", _conv_out,
    lambda *a: None)


def wgrad_workspace(x, dout, kh, kw):
    N, _, _, C = x.shape
    _, OH, OW, CO = dout.shape
    n = int(_lib.lib().specenh_conv2d_wgrad_workspace_bytes(N, OH, OW, kh, kw, C, CO))
    return torch.empty(max(16, n), dtype=torch.uint8, device=x.device)


def _wgrad_out(x, dout, kh, kw, stride, pad_t, pad_l, in_dil, dw, dbias, workspace,
               overwrite=False):
    _need(x, "x")
    _need(dout, "dout")
    N, IH, IW, C = x.shape
    _, OH, OW, CO = dout.shape
    if dout.dtype != x.dtype or dout.shape[0] != N:
        raise ValueError("dout must be [N, OH, OW, CO] in x's dtype")
    if dw.dtype != torch.float32 or dw.numel() != CO * kh * kw * C or not dw.is_contiguous():
        raise ValueError("dw must be contiguous float32 [CO][KH][KW][C]")
    if dbias is not None and (dbias.dtype != torch.float32 or dbias.numel() != CO):
        raise ValueError("dbias must be float32 [CO]")
    need = int(_lib.lib().specenh_conv2d_wgrad_workspace_bytes(N, OH, OW, kh, kw, C, CO))
    if workspace.numel() < need:
        raise ValueError(f"workspace needs {need} bytes")
    if overwrite:  # dw / dbias = the gradient (no zeroing beforehand)
        _lib.check(_lib.lib().specenh_conv2d_wgrad_ex(
            _code(x), _vp(x), N, IH, IW, C, _vp(dout), kh, kw, CO, stride, pad_t, pad_l, in_dil,
            OH, OW, _vp(dw), _vp(dbias), 1, _vp(workspace), _st(x)), "conv2d_wgrad")
        return
    _lib.check(_lib.lib().specenh_conv2d_wgrad(
        _code(x), _vp(x), N, IH, IW, C, _vp(dout), kh, kw, CO, stride, pad_t, pad_l, in_dil, OH,
        OW, _vp(dw), _vp(dbias), _vp(workspace), _st(x)), "conv2d_wgrad")


def _wgrad(x, dout, kh, kw, stride, pad_t, pad_l, in_dil):
    C, CO = x.shape[3], dout.shape[3]
    dw = torch.zeros((CO, kh, kw, C), dtype=torch.float32, device=x.device)
    db = torch.zeros((CO,), dtype=torch.float32, device=x.device)
    _wgrad_out(x, dout, kh, kw, stride, pad_t, pad_l, in_dil, dw, db,
               wgrad_workspace(x, dout, kh, kw))
    return dw, db


_WG_ARGS = "int kh, int kw, int stride, int pad_t, int pad_l, int in_dil"
_op(f"conv2d_wgrad(Tensor x, Tensor dout, {_WG_ARGS}) -> (Tensor, Tensor)", _wgrad,
    lambda x, dout, kh, kw, stride, pad_t, pad_l, in_dil:
    (x.new_empty((dout.shape[3], kh, kw, x.shape[3]), dtype=torch.float32),
     x.new_empty((dout.shape[3],), dtype=torch.float32)))
_op(f"conv2d_wgrad_out(Tensor x, Tensor dout, {_WG_ARGS}, Tensor(a!) dw, Tensor(b!)? dbias, "
    "Tensor(c!) workspace, bool overwrite=False) -> ()", _wgrad_out, lambda *a, **k: None)


def _wgrad_pooled_out(x, dpool, argmax, pooled, kh, kw, stride, pad_t, pad_l, in_dil, dw, dbias,
                      workspace):
    _need(x, "x")
    _need(dpool, "dpool")
    N, IH, IW, C = x.shape
    _, PH, PW, CO = dpool.shape
    OH, OW = 2 * PH, 2 * PW
    if dpool.dtype != x.dtype or dpool.shape[0] != N:
        raise ValueError("dpool must be [N, OH/2, OW/2, CO] in x's dtype")
    if argmax.dtype != torch.uint8 or argmax.shape != dpool.shape:
        raise ValueError("argmax must be uint8 like dpool")
    if pooled is not None and (pooled.dtype != x.dtype or pooled.shape != dpool.shape):
        raise ValueError("pooled must be like dpool")
    if dw.dtype != torch.float32 or dw.numel() != CO * kh * kw * C or not dw.is_contiguous():
        raise ValueError("dw must be contiguous float32 [CO][KH][KW][C]")
    if dbias is not None and (dbias.dtype != torch.float32 or dbias.numel() != CO):
        raise ValueError("dbias must be float32 [CO]")
    need = int(_lib.lib().specenh_conv2d_wgrad_workspace_bytes(N, OH, OW, kh, kw, C, CO))
    if workspace.numel() < need:
        raise ValueError(f"workspace needs {need} bytes")
    _lib.check(_lib.lib().specenh_conv2d_wgrad_pooled(
        _code(x), _vp(x), N, IH, IW, C, _vp(dpool), _vp(argmax), _vp(pooled), kh, kw, CO, stride,
        pad_t, pad_l, in_dil, OH, OW, _vp(dw), _vp(dbias), _vp(workspace), _st(x)),
        "conv2d_wgrad_pooled")


_op(f"conv2d_wgrad_pooled_out(Tensor x, Tensor dpool, Tensor argmax, Tensor? pooled, {_WG_ARGS}, "
    "Tensor(a!) dw, Tensor(b!)? dbias, Tensor(c!) workspace) -> ()", _wgrad_pooled_out,
    lambda *a: None)


def _conv_pooled_in_out(dpool, argmax, pooled, w, bias, kh, kw, cout, pad_t, pad_l, oh, ow, act,
                        mask, out):
    """specenh_conv2d_pooled_in: a stride-1 conv of the full-resolution gradient of a ReLU +
    MaxPooling2D((2,2)) given as the pool's gradient dpool [N, IH/2, IW/2, C] (+ argmax, pooled
    output): bitwise maxpool2_bwd followed by conv2d_out, without the full-resolution tensor."""
    _need(dpool, "dpool")
    _need(out, "out")
    N, PH, PW, C = dpool.shape
    IH, IW = 2 * PH, 2 * PW
    if argmax.dtype != torch.uint8 or argmax.shape != dpool.shape:
        raise ValueError("argmax must be uint8 like dpool")
    if pooled is not None and (pooled.dtype != dpool.dtype or pooled.shape != dpool.shape):
        raise ValueError("pooled must be like dpool")
    if w.dtype != dpool.dtype or w.numel() != cout * kh * kw * C:
        raise ValueError("w must be the [CO][KH][KW][C] GEMM weights in dpool's dtype")
    _need(w, "w")
    if tuple(out.shape) != (N, oh, ow, cout) or out.dtype != dpool.dtype:
        raise ValueError(f"out must be {(N, oh, ow, cout)} in dpool's dtype")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != cout):
        raise ValueError("bias must be float32 [CO]")
    if mask is not None and (mask.dtype != dpool.dtype or mask.numel() != N * oh * ow * cout):
        raise ValueError("mask must match the output (compute dtype)")
    _lib.check(_lib.lib().specenh_conv2d_pooled_in(
        _code(dpool), _vp(dpool), _vp(argmax), _vp(pooled), N, IH, IW, C, _vp(w), kh, kw, cout,
        _vp(bias), pad_t, pad_l, oh, ow, act, _vp(mask), _vp(out), _st(dpool)),
        "conv2d_pooled_in")


_op("conv2d_pooled_in_out(Tensor dpool, Tensor argmax, Tensor? pooled, Tensor w, Tensor? bias, "
    "int kh, int kw, int cout, int pad_t, int pad_l, int oh, int ow, int act, Tensor? mask, "
    "Tensor(a!) out) -> ()", _conv_pooled_in_out, lambda *a: None)


def _tail_out(x, wt, bt, cout, kt, wo, bo, ko, out):
    _need(x, "x")
    _need(out, "out")
    N, H, W, C = x.shape
    if wt.dtype != x.dtype or wo.dtype != x.dtype or wt.numel() != cout * kt * kt * C or \
            wo.numel() != ko * ko * cout:
        raise ValueError("wt / wo must be the two layers' GEMM weights in x's dtype")
    if bt.dtype != torch.float32 or bt.numel() != cout or bo.dtype != torch.float32 or \
            bo.numel() != 1:
        raise ValueError("biases must be float32 [CO] and [1]")
    if out.dtype != torch.float32 or out.numel() != N * 4 * H * W:
        raise ValueError("out must be float32 [N, 2H, 2W(, 1)]")
    _lib.check(_lib.lib().specenh_convt_conv_out(
        _code(x), _vp(x), N, H, W, C, _vp(wt), _vp(bt), cout, kt, _vp(wo), _vp(bo), ko, _vp(out),
        _st(x)), "convt_conv_out")


def _tail(x, wt, bt, cout, kt, wo, bo, ko):
    N, H, W, _ = x.shape
    out = torch.empty((N, 2 * H, 2 * W, 1), dtype=torch.float32, device=x.device)
    _tail_out(x, wt, bt, cout, kt, wo, bo, ko, out)
    return out


_op("convt_conv_out(Tensor x, Tensor wt, Tensor bt, int cout, int kt, Tensor wo, Tensor bo, "
    "int ko) -> Tensor", _tail,
    lambda x, wt, bt, cout, kt, wo, bo, ko:
    x.new_empty((x.shape[0], 2 * x.shape[1], 2 * x.shape[2], 1), dtype=torch.float32))
_op("convt_conv_out_out(Tensor x, Tensor wt, Tensor bt, int cout, int kt, Tensor wo, Tensor bo, "
    "int ko, Tensor(a!) out) -> ()", _tail_out, lambda *a: None)


def _tail_train_out(x, wt, bt, cout, kt, wo, bo, ko, map_out, logits, out):
    _need(x, "x")
    for t, n in ((map_out, "map_out"), (logits, "logits"), (out, "out")):
        _need(t, n)
    N, H, W, C = x.shape
    if wt.dtype != x.dtype or wo.dtype != x.dtype or wt.numel() != cout * kt * kt * C or \
            wo.numel() != ko * ko * cout:
        raise ValueError("wt / wo must be the two layers' GEMM weights in x's dtype")
    if bt.dtype != torch.float32 or bt.numel() != cout or bo.dtype != torch.float32 or \
            bo.numel() != 1:
        raise ValueError("biases must be float32 [CO] and [1]")
    if tuple(map_out.shape) != (N, 2 * H, 2 * W, cout) or map_out.dtype != x.dtype:
        raise ValueError("map_out must be [N, 2H, 2W, cout] in x's dtype")
    if logits.dtype != torch.float32 or logits.numel() != N * 4 * H * W:
        raise ValueError("logits must be float32 [N, 2H, 2W(, 1)]")
    if out.dtype != x.dtype or out.numel() != N * 4 * H * W:
        raise ValueError("out must be [N, 2H, 2W(, 1)] in x's dtype")
    _lib.check(_lib.lib().specenh_convt_conv_out_train(
        _code(x), _vp(x), N, H, W, C, _vp(wt), _vp(bt), cout, kt, _vp(wo), _vp(bo), ko,
        _vp(map_out), _vp(logits), _vp(out), _st(x)), "convt_conv_out_train")


_op("convt_conv_out_train_out(Tensor x, Tensor wt, Tensor bt, int cout, int kt, Tensor wo, "
    "Tensor bo, int ko, Tensor(a!) map_out, Tensor(b!) logits, Tensor(c!) out) -> ()",
    _tail_train_out, lambda *a: None)


def _dec3_out(x, w1, b1, cout1, wt, bt, cout2, wo, bo, k, out):
    _need(x, "x")
    _need(out, "out")
    N, H, W, C = x.shape
    if any(t.dtype != x.dtype for t in (w1, wt, wo)) or w1.numel() != cout1 * k * k * C or \
            wt.numel() != cout2 * k * k * cout1 or wo.numel() != k * k * cout2:
        raise ValueError("w1 / wt / wo must be the three layers' GEMM weights in x's dtype")
    if any(t.dtype != torch.float32 for t in (b1, bt, bo)) or b1.numel() != cout1 or \
            bt.numel() != cout2 or bo.numel() != 1:
        raise ValueError("biases must be float32 [CO1], [CO2] and [1]")
    if out.dtype not in (torch.float32, torch.float16) or out.numel() != N * 16 * H * W:
        raise ValueError("out must be float32 or float16 [N, 4H, 4W(, 1)]")
    _lib.check(_lib.lib().specenh_decoder3_ex(
        _code(x), _vp(x), N, H, W, C, _vp(w1), _vp(b1), cout1, _vp(wt), _vp(bt), cout2, _vp(wo),
        _vp(bo), k, _vp(out), _code(out), _st(x)), "decoder3")


def _dec3(x, w1, b1, cout1, wt, bt, cout2, wo, bo, k):
    N, H, W, _ = x.shape
    out = torch.empty((N, 4 * H, 4 * W, 1), dtype=torch.float32, device=x.device)
    _dec3_out(x, w1, b1, cout1, wt, bt, cout2, wo, bo, k, out)
    return out


_D3 = ("Tensor x, Tensor w1, Tensor b1, int cout1, Tensor wt, Tensor bt, int cout2, Tensor wo, "
       "Tensor bo, int k")
_op(f"decoder3({_D3}) -> Tensor", _dec3,
    lambda x, w1, b1, cout1, wt, bt, cout2, wo, bo, k:
    x.new_empty((x.shape[0], 4 * x.shape[1], 4 * x.shape[2], 1), dtype=torch.float32))
_op(f"decoder3_out({_D3}, Tensor(a!) out) -> ()", _dec3_out, lambda *a: None)


def _enc2_out(x, w1, b1, cout1, w2, b2, cout2, k, out):
    _need(x, "x")
    _need(out, "out")
    N, H, W, C = x.shape
    if C != 1:
        raise ValueError("x must be [N, H, W, 1]")
    if any(t.dtype != x.dtype for t in (w1, w2)) or w1.numel() != cout1 * k * k or \
            w2.numel() != cout2 * k * k * cout1:
        raise ValueError("w1 / w2 must be the two layers' GEMM weights in x's dtype")
    if any(t.dtype != torch.float32 for t in (b1, b2)) or b1.numel() != cout1 or \
            b2.numel() != cout2:
        raise ValueError("biases must be float32 [CO1] and [CO2]")
    if out.dtype != x.dtype or tuple(out.shape) != (N, H // 4, W // 4, cout2):
        raise ValueError("out must be [N, H/4, W/4, CO2] in x's dtype")
    _lib.check(_lib.lib().specenh_encoder2(
        _code(x), _vp(x), N, H, W, _vp(w1), _vp(b1), cout1, _vp(w2), _vp(b2), cout2, k, _vp(out),
        _st(x)), "encoder2")


def _enc2(x, w1, b1, cout1, w2, b2, cout2, k):
    N, H, W, _ = x.shape
    out = torch.empty((N, H // 4, W // 4, cout2), dtype=x.dtype, device=x.device)
    _enc2_out(x, w1, b1, cout1, w2, b2, cout2, k, out)
    return out


_E2 = "Tensor x, Tensor w1, Tensor b1, int cout1, Tensor w2, Tensor b2, int cout2, int k"
_op(f"encoder2({_E2}) -> Tensor", _enc2,
    lambda x, w1, b1, cout1, w2, b2, cout2, k:
    x.new_empty((x.shape[0], x.shape[1] // 4, x.shape[2] // 4, cout2)))
_op(f"encoder2_out({_E2}, Tensor(a!) out) -> ()", _enc2_out, lambda *a: None)


def encoder2_supported(dtype: torch.dtype, cin: int, cout1: int, cout2: int, k: int,
                       height: int, width: int) -> bool:
    """specenh_encoder2's configuration: the reference model's first two layers on 128-wide
    one-channel images."""
    return dtype in (torch.float16, torch.bfloat16) and (cin, cout1, cout2, k, width) == \
        (1, 16, 32, 5, 128) and height % 4 == 0


def decoder3_supported(dtype: torch.dtype, cin: int, cout1: int, cout2: int, k: int,
                       width: int) -> bool:
    """specenh_decoder3's configuration: the reference model's decoder on 128-wide images."""
    return dtype in (torch.float16, torch.bfloat16) and (cin, cout1, cout2, k, width) == \
        (64, 32, 16, 5, 32)


def tail_supported(dtype: torch.dtype, cin: int, cout: int, kt: int, ko: int,
                   w_in: int | None = None) -> bool:
    """specenh_convt_conv_out's configurations: the reference model's last two layers
    (32 -> 16, k 5, any width), and the 32 -> 32 tails of the hyperparameter-scan models
    (k = 3 / 5 / 7) and manual_scan.py's 32 -> 64 (k = 3 / 5) on 64-position-wide inputs
    (csrc/tail_rows_g.hip)."""
    if dtype not in (torch.float16, torch.bfloat16):
        return False
    if (cin, cout, kt, ko) == (32, 16, 5, 5):
        return True
    return w_in == 64 and cin == 32 and kt == ko and ((cout == 32 and kt in (3, 5, 7)) or
                                                       (cout == 64 and kt in (3, 5)))


# ---------------------------------------------------------------- pooling, loss, optimizer
def _pool_out(x, out, argmax):
    _need(x, "x")
    N, H, W, C = x.shape
    if tuple(out.shape) != (N, H // 2, W // 2, C) or out.dtype != x.dtype:
        raise ValueError("out must be [N, H/2, W/2, C] in x's dtype")
    if argmax.dtype != torch.uint8 or argmax.shape != out.shape:
        raise ValueError("argmax must be uint8 like out")
    _lib.check(_lib.lib().specenh_maxpool2_fwd(_code(x), _vp(x), N, H, W, C, _vp(out),
                                               _vp(argmax), _st(x)), "maxpool2_fwd")


def _pool(x):
    N, H, W, C = x.shape
    out = torch.empty((N, H // 2, W // 2, C), dtype=x.dtype, device=x.device)
    am = torch.empty(out.shape, dtype=torch.uint8, device=x.device)
    _pool_out(x, out, am)
    return out, am


def _pool_bwd_out(dy, argmax, pooled, dx):
    _need(dy, "dy")
    N, H2, W2, C = dy.shape
    if tuple(dx.shape) != (N, 2 * H2, 2 * W2, C) or dx.dtype != dy.dtype:
        raise ValueError("dx must be [N, 2H, 2W, C] in dy's dtype")
    _lib.check(_lib.lib().specenh_maxpool2_bwd(_code(dy), _vp(dy), _vp(argmax), _vp(pooled), N,
                                               2 * H2, 2 * W2, C, _vp(dx), _st(dy)),
               "maxpool2_bwd")


def _pool_bwd(dy, argmax, pooled):
    N, H2, W2, C = dy.shape
    dx = torch.empty((N, 2 * H2, 2 * W2, C), dtype=dy.dtype, device=dy.device)
    _pool_bwd_out(dy, argmax, pooled, dx)
    return dx


_op("maxpool2(Tensor x) -> (Tensor, Tensor)", _pool,
    lambda x: (x.new_empty((x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.shape[3])),
               x.new_empty((x.shape[0], x.shape[1] // 2, x.shape[2] // 2, x.shape[3]),
                           dtype=torch.uint8)))
_op("maxpool2_out(Tensor x, Tensor(a!) out, Tensor(b!) argmax) -> ()", _pool_out,
    lambda *a: None)
_op("maxpool2_bwd(Tensor dy, Tensor argmax, Tensor? pooled) -> Tensor", _pool_bwd,
    lambda dy, argmax, pooled: dy.new_empty((dy.shape[0], 2 * dy.shape[1], 2 * dy.shape[2],
                                             dy.shape[3])))
_op("maxpool2_bwd_out(Tensor dy, Tensor argmax, Tensor? pooled, Tensor(a!) dx) -> ()",
    _pool_bwd_out, lambda *a: None)


def _bce_out(z, target, grad, loss_sum):
    if z.dtype != torch.float32 or target.numel() != z.numel():
        raise ValueError("z must be float32 and target the same size")
    _need(z, "z")
    _need(target, "target")
    if loss_sum.dtype != torch.float64 or loss_sum.numel() != 1:
        raise ValueError("loss_sum must be a float64 [1] accumulator")
    if grad is not None and grad.numel() != z.numel():
        raise ValueError("grad must have z's size")
    _lib.check(_lib.lib().specenh_bce_logits(
        _vp(z), _vp(target), _code(target), z.numel(), _vp(grad),
        _code(grad) if grad is not None else F32, _vp(loss_sum), _st(z)), "bce_logits")


def _bce(z, target, grad_dtype):
    loss = torch.zeros(1, dtype=torch.float64, device=z.device)
    grad = torch.empty(z.shape, dtype=grad_dtype, device=z.device)
    _bce_out(z, target, grad, loss)
    return loss, grad


_op("bce_logits(Tensor z, Tensor target, ScalarType grad_dtype) -> (Tensor, Tensor)", _bce,
    lambda z, target, grad_dtype: (z.new_empty((1,), dtype=torch.float64),
                                   z.new_empty(z.shape, dtype=grad_dtype)))
_op("bce_logits_out(Tensor z, Tensor target, Tensor(a!)? grad, Tensor(b!) loss_sum) -> ()",
    _bce_out, lambda *a: None)


def _adam(w, g, m, v, lr_t, beta_1, beta_2, epsilon, grad_scale, w_lowp):
    n = w.numel()
    for t, nm in ((g, "g"), (m, "m"), (v, "v")):
        if t.numel() != n or t.dtype != torch.float32:
            raise ValueError(f"{nm} must be float32 like w")
    if w_lowp is not None and w_lowp.numel() != n:
        raise ValueError("w_lowp must have w's size")
    _lib.check(_lib.lib().specenh_adam_step(
        _vp(w), _vp(g), _vp(m), _vp(v), n, lr_t, beta_1, beta_2, epsilon, grad_scale,
        _vp(w_lowp), _code(w_lowp) if w_lowp is not None else F32, _st(w)), "adam_step")


_op("adam_step_(Tensor(a!) w, Tensor g, Tensor(b!) m, Tensor(c!) v, float lr_t, float beta_1, "
    "float beta_2, float epsilon, float grad_scale, Tensor(d!)? w_lowp) -> ()", _adam,
    lambda *a: None)


def _adam_flip(w, g, m, v, lr_t, beta_1, beta_2, epsilon, grad_scale, w_lowp, seg_off, seg_kcc,
               seg_dst):
    """adam_step_ plus the flipped input-gradient weights of len(seg_dst) layers in the same
    launch (specenh_adam_step_flip): seg_off[s] is the layer's flat weight offset in w,
    seg_kcc[3s:3s+3] = (k, ci, co), seg_dst[s] its [ci][k][k][co] buffer."""
    import ctypes
    n = w.numel()
    for t, nm in ((g, "g"), (m, "m"), (v, "v")):
        if t.numel() != n or t.dtype != torch.float32:
            raise ValueError(f"{nm} must be float32 like w")
    if w_lowp is not None and w_lowp.numel() != n:
        raise ValueError("w_lowp must have w's size")
    ns = len(seg_dst)
    if len(seg_off) != ns or len(seg_kcc) != 3 * ns:
        raise ValueError("segment lists")
    want = w_lowp.dtype if w_lowp is not None else torch.float32
    for s, d in enumerate(seg_dst):
        k, ci, co = seg_kcc[3 * s:3 * s + 3]
        if d.dtype != want or d.numel() != k * k * ci * co or not d.is_contiguous():
            raise ValueError(f"segment {s}: destination must be contiguous {want} [{ci}][{k}][{k}][{co}]")
    off = (ctypes.c_longlong * max(ns, 1))(*seg_off)
    kcc = (ctypes.c_int * max(3 * ns, 1))(*seg_kcc)
    dst = (ctypes.c_void_p * max(ns, 1))(*[d.data_ptr() for d in seg_dst])
    _lib.check(_lib.lib().specenh_adam_step_flip(
        _vp(w), _vp(g), _vp(m), _vp(v), n, lr_t, beta_1, beta_2, epsilon, grad_scale,
        _vp(w_lowp), _code(w_lowp) if w_lowp is not None else F32, ns, off, kcc, dst, _st(w)),
        "adam_step_flip")


_op("adam_step_flip_(Tensor(a!) w, Tensor g, Tensor(b!) m, Tensor(c!) v, float lr_t, "
    "float beta_1, float beta_2, float epsilon, float grad_scale, Tensor(d!)? w_lowp, "
    "int[] seg_off, int[] seg_kcc, Tensor(e!)[] seg_dst) -> ()", _adam_flip, lambda *a: None)


def _flip_out(bt, k, ci, co, out):
    if bt.numel() != co * k * k * ci or out.numel() != bt.numel() or out.dtype != bt.dtype:
        raise ValueError("bt / out sizes")
    _lib.check(_lib.lib().specenh_weight_flip_transpose(_code(bt), _vp(bt), k, ci, co, _vp(out),
                                                        _st(bt)), "flip_transpose")


def _flip(bt, k, ci, co):
    out = torch.empty((ci, k, k, co), dtype=bt.dtype, device=bt.device)
    _flip_out(bt, k, ci, co, out)
    return out


_op("weight_flip_transpose(Tensor bt, int k, int ci, int co) -> Tensor", _flip,
    lambda bt, k, ci, co: bt.new_empty((ci, k, k, co)))
_op("weight_flip_transpose_out(Tensor bt, int k, int ci, int co, Tensor(a!) out) -> ()",
    _flip_out, lambda *a: None)


def _cast_out(x, out):
    if out.numel() != x.numel():
        raise ValueError("out must have x's size")
    _need(x, "x")
    _need(out, "out")
    _lib.check(_lib.lib().specenh_cast(_code(x), _vp(x), _code(out), _vp(out), x.numel(), _st(x)),
               "cast")


def _cast(x, dtype):
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    _cast_out(x, out)
    return out


_op("cast(Tensor x, ScalarType dtype) -> Tensor", _cast,
    lambda x, dtype: x.new_empty(x.shape, dtype=dtype))
_op("cast_out(Tensor x, Tensor(a!) out) -> ()", _cast_out, lambda *a: None)


# ---------------------------------------------------------------- label filters
def _batch3(S):
    if S.dim() != 3:
        raise ValueError("S must be [batch, rows, cols]")
    _need(S, "S")
    return S.shape


def _filter(S, op):
    B, rows, cols = _batch3(S)
    L = _lib.lib()
    out = torch.empty_like(S)
    ws = torch.empty(max(16, int(L.specenh_filter_workspace_bytes(B, rows))), dtype=torch.uint8,
                     device=S.device)
    _lib.check(L.specenh_filter(int(op), _code(S, (F32, F64)), _vp(S), B, rows, cols, rows * cols,
                                _vp(out), _vp(ws), _st(S)), "filter")
    return out


def _quantfilt(S, thr):
    B, rows, cols = _batch3(S)
    out = torch.empty_like(S)
    _lib.check(_lib.lib().specenh_quantfilt(_code(S, (F32, F64)), _vp(S), B, rows, cols,
                                            rows * cols, float(thr), _vp(out), _st(S)), "quantfilt")
    return out


def _u8ws(S):
    B, rows, cols = S.shape
    n = int(_lib.lib().specenh_u8filter_workspace_bytes(B, rows, cols))
    return torch.empty(max(16, n), dtype=torch.uint8, device=S.device)


def _gaussblr(S, kw, kh, sigma):
    B, rows, cols = _batch3(S)
    out = torch.empty_like(S)
    _lib.check(_lib.lib().specenh_gaussblr(_code(S, (F32, F64)), _vp(S), B, rows, cols,
                                           rows * cols, int(kw), int(kh), float(sigma), _vp(out),
                                           _vp(_u8ws(S)), _st(S)), "gaussblr")
    return out


def _morph(S):
    B, rows, cols = _batch3(S)
    out = torch.empty_like(S)
    _lib.check(_lib.lib().specenh_morph(_code(S, (F32, F64)), _vp(S), B, rows, cols, rows * cols,
                                        _vp(out), _vp(_u8ws(S)), _st(S)), "morph")
    return out


_op("label_filter(Tensor S, int op) -> Tensor", _filter, lambda S, op: torch.empty_like(S))
_op("quantfilt(Tensor S, float thr) -> Tensor", _quantfilt, lambda S, thr: torch.empty_like(S))
_op("gaussblr(Tensor S, int kw, int kh, float sigma) -> Tensor", _gaussblr,
    lambda S, kw, kh, sigma: torch.empty_like(S))
_op("morph(Tensor S) -> Tensor", _morph, lambda S: torch.empty_like(S))


# ---------------------------------------------------------------- bilateral label filter
def bilateral_taps(d, sigma_space):
    """(radius, taps) cv2.bilateralFilter derives from ``(d, sigma_space)``
    (specenh_bilateral_taps); NotImplementedError above radius 15."""
    r, n = ctypes.c_int(0), ctypes.c_int(0)
    _lib.check(_lib.lib().specenh_bilateral_taps(int(d), float(sigma_space), ctypes.byref(r),
                                                 ctypes.byref(n)), "bilateral_taps")
    return r.value, n.value


def _bilateral_u8_check(img):
    """(batch, rows, cols, batch stride) of uint8 images [B, rows, cols], each row-major; the
    batch stride is free (>= rows * cols)."""
    if img.dim() != 3 or img.dtype != torch.uint8:
        raise ValueError("img must be uint8 [batch, rows, cols]")
    B, rows, cols = img.shape
    if rows < 1 or cols < 1:
        raise ValueError("img must hold at least one row and one column")
    if (cols > 1 and img.stride(2) != 1) or (rows > 1 and img.stride(1) != cols):
        raise ValueError("every image of img must be row-major and contiguous")
    stride = img.stride(0) if B > 1 else rows * cols
    if stride < rows * cols:
        raise ValueError("images must not overlap: batch stride >= rows * cols")
    return B, rows, cols, stride


def _bilateral_u8(img, d, sigma_color, sigma_space):
    B, rows, cols, stride = _bilateral_u8_check(img)
    out = torch.empty((B, rows, cols), dtype=torch.uint8, device=img.device)
    _lib.check(_lib.lib().specenh_bilateral_u8(
        _vp(img), B, rows, cols, stride, int(d), float(sigma_color), float(sigma_space),
        _vp(out), _st(img)), "bilateral_u8")
    return out


def _bilateral_u8_fake(img, d, sigma_color, sigma_space):
    B, rows, cols, _ = _bilateral_u8_check(img)
    return img.new_empty((B, rows, cols), dtype=torch.uint8)


def _bilateral(S, d, sigma_color, sigma_space):
    B, rows, cols = _batch3(S)
    L = _lib.lib()
    out = torch.empty_like(S)
    ws = torch.empty(max(16, int(L.specenh_bilateral_workspace_bytes(B, rows, cols))),
                     dtype=torch.uint8, device=S.device)
    _lib.check(L.specenh_bilateral(_code(S, (F32, F64)), _vp(S), B, rows, cols, rows * cols,
                                   int(d), float(sigma_color), float(sigma_space), _vp(out),
                                   _vp(ws), _st(S)), "bilateral")
    return out


_op("bilateral(Tensor S, int d, float sigma_color, float sigma_space) -> Tensor", _bilateral,
    lambda S, d, sigma_color, sigma_space: torch.empty_like(S))
_op("bilateral_u8(Tensor img, int d, float sigma_color, float sigma_space) -> Tensor",
    _bilateral_u8, _bilateral_u8_fake)


# ---------------------------------------------------------------- non-local means
def _nl_means_shape(S):
    if S.dim() not in (2, 3):
        raise ValueError("S must be [rows, cols] or [batch, rows, cols]")
    if S.shape[-2] < 1 or S.shape[-1] < 1:
        raise ValueError("S must hold at least one row and one column")


def _nl_means(S, patch_size, patch_distance, h, sigma):
    _nl_means_shape(S)
    S3 = (S if S.dim() == 3 else S.unsqueeze(0)).contiguous()
    B, rows, cols = S3.shape
    out = torch.empty_like(S3)
    _lib.check(_lib.lib().specenh_nlmeans(_code(S3, (F32, F64)), _vp(S3), B, rows, cols,
                                          rows * cols, int(patch_size), int(patch_distance),
                                          float(h), float(sigma), _vp(out), _st(S3)), "nl_means")
    return out.view(S.shape)


def _nl_means_fake(S, patch_size, patch_distance, h, sigma):
    _nl_means_shape(S)
    return S.new_empty(S.shape)


_op("nl_means(Tensor S, int patch_size, int patch_distance, float h, float sigma) -> Tensor",
    _nl_means, _nl_means_fake)


# ---------------------------------------------------------------- k-means
def _kmeans_shape(X, C):
    """(batch, n, d, k) of points X [n, d] or [batch, n, d] and centres C [k, d] or [batch, k, d]."""
    if X.dim() not in (2, 3) or C.dim() != X.dim():
        raise ValueError("X must be [n, d] or [batch, n, d] and C [k, d] or [batch, k, d]")
    if X.dtype != torch.float32 or C.dtype != torch.float32:
        raise TypeError("X and C must be float32")
    n, d = X.shape[-2:]
    k = C.shape[-2]
    if C.shape[-1] != d or (X.dim() == 3 and C.shape[0] != X.shape[0]):
        raise ValueError("C must have X's batch and d")
    if n < 1 or d < 1 or k < 1:
        raise ValueError("X and C must hold at least one row and one column")
    return (X.shape[0] if X.dim() == 3 else 1), n, d, k


def _kmeans_layout(X3):
    """X3 as the kernels read it, (X3, ld, batch stride): unit stride along d, rows ld >= d
    apart, items at least n * ld apart; any other view is copied."""
    B, n, d = X3.shape
    ld = X3.stride(1) if n > 1 else d
    stride = X3.stride(0) if B > 1 else n * ld
    if (d > 1 and X3.stride(2) != 1) or ld < d or stride < n * ld:
        return X3.contiguous(), d, n * d
    return X3, ld, stride


def _kmeans_ws(L, B, n, d, k, device):
    return torch.empty(max(16, int(L.specenh_kmeans_workspace_bytes(B, n, d, k))),
                       dtype=torch.uint8, device=device)


def _kmeans_assign(X, C):
    B, n, d, k = _kmeans_shape(X, C)
    X3, ld, stride = _kmeans_layout(X.reshape(B, n, d) if X.dim() == 2 else X)
    C3 = C.reshape(B, k, d).contiguous()
    L = _lib.lib()
    labels = torch.empty((B, n), dtype=torch.int32, device=X.device)
    ws = _kmeans_ws(L, B, n, d, k, X.device)
    _lib.check(L.specenh_kmeans_assign(_vp(X3), B, n, d, ld, stride, _vp(C3), k, _vp(labels),
                                       _vp(ws), ws.numel(), _st(X3)), "kmeans_assign")
    return labels if X.dim() == 3 else labels.view(n)


def _kmeans_assign_fake(X, C):
    _kmeans_shape(X, C)
    return X.new_empty(X.shape[:-1], dtype=torch.int32)


def _kmeans_step(X, C):
    B, n, d, k = _kmeans_shape(X, C)
    X3, ld, stride = _kmeans_layout(X.reshape(B, n, d) if X.dim() == 2 else X)
    C3 = C.reshape(B, k, d).contiguous()
    L = _lib.lib()
    labels = torch.empty((B, n), dtype=torch.int32, device=X.device)
    C_new = torch.empty_like(C3)
    counts = torch.empty((B, k), dtype=torch.int32, device=X.device)
    inertia = torch.empty((B,), dtype=torch.float32, device=X.device)
    ws = _kmeans_ws(L, B, n, d, k, X.device)
    _lib.check(L.specenh_kmeans_step(_vp(X3), B, n, d, ld, stride, _vp(C3), k, _vp(labels),
                                     _vp(C_new), _vp(counts), _vp(inertia), _vp(ws), ws.numel(),
                                     _st(X3)), "kmeans_step")
    if X.dim() == 3:
        return labels, C_new, counts, inertia
    return labels.view(n), C_new.view(k, d), counts.view(k), inertia.view(())


def _kmeans_step_fake(X, C):
    _kmeans_shape(X, C)
    lead = X.shape[:-2]
    return (X.new_empty(X.shape[:-1], dtype=torch.int32), C.new_empty(C.shape),
            X.new_empty(C.shape[:-1], dtype=torch.int32), X.new_empty(lead))


_op("kmeans_assign(Tensor X, Tensor C) -> Tensor", _kmeans_assign, _kmeans_assign_fake)
_op("kmeans_step(Tensor X, Tensor C) -> (Tensor, Tensor, Tensor, Tensor)", _kmeans_step,
    _kmeans_step_fake)


# ---------------------------------------------------------------- strip glue
def _pack_out(S, rows, width, n_strips, out):
    if S.dim() != 3 or S.dtype != torch.float32 or S.stride(2) != 1 or S.stride(1) != S.shape[2]:
        raise ValueError("S must be float32 [batch, F, T] with row-major spectrograms")
    B, F, T = S.shape
    if (out.numel() != B * n_strips * rows * width or not out.is_contiguous()
            or out.device != S.device or out.dtype not in (torch.float32, torch.bfloat16,
                                                          torch.float16)):
        raise ValueError(f"out must be a contiguous float32/bfloat16/float16 tensor of "
                         f"{B * n_strips} x {rows} x {width} elements on S's device")
    _lib.check(_lib.lib().specenh_strips_pack(
        _code(out), _vp(S), B, F, T, S.stride(0), rows, width, n_strips, _vp(out), _st(S)),
        "strips_pack")


def _pack(S, rows, width, n_strips, dtype):
    out = torch.empty((S.shape[0] * n_strips, rows, width, 1), dtype=dtype, device=S.device)
    _pack_out(S, rows, width, n_strips, out)
    return out


def _unpack_out(strips, rows, width, n_strips, out):
    _need(strips, "strips")
    if strips.shape[0] % n_strips or tuple(strips.shape[1:3]) != (rows, width):
        raise ValueError(f"strips must be [k*{n_strips}, {rows}, {width}(, 1)]")
    B = strips.shape[0] // n_strips
    if (out.numel() != B * rows * n_strips * width or not out.is_contiguous()
            or out.device != strips.device or out.dtype != torch.float32):
        raise ValueError(f"out must be a contiguous float32 tensor of {B} x {rows} x "
                         f"{n_strips * width} elements on the strips' device")
    _lib.check(_lib.lib().specenh_strips_unpack(_code(strips), _vp(strips), B, rows, width,
                                                n_strips, _vp(out), _st(strips)), "strips_unpack")


def _unpack(strips, rows, width, n_strips):
    out = torch.empty((strips.shape[0] // n_strips, rows, n_strips * width), dtype=torch.float32,
                      device=strips.device)
    _unpack_out(strips, rows, width, n_strips, out)
    return out


_op("strips_pack(Tensor S, int rows, int width, int n_strips, ScalarType dtype) -> Tensor", _pack,
    lambda S, rows, width, n_strips, dtype:
    S.new_empty((S.shape[0] * n_strips, rows, width, 1), dtype=dtype))
_op("strips_unpack(Tensor strips, int rows, int width, int n_strips) -> Tensor", _unpack,
    lambda strips, rows, width, n_strips:
    strips.new_empty((strips.shape[0] // n_strips, rows, n_strips * width), dtype=torch.float32))
_op("strips_pack_out(Tensor S, int rows, int width, int n_strips, Tensor(a!) out) -> ()",
    _pack_out, lambda *a: None)
_op("strips_unpack_out(Tensor strips, int rows, int width, int n_strips, Tensor(a!) out) -> ()",
    _unpack_out, lambda *a: None)

ops = torch.ops.specenh
