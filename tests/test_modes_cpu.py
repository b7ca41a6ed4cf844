"""Host-side checks of the mode-decomposition boundary (no GPU): the extension header, ctypes
table, exports, operators and constants in sync; the C-ABI argument errors, all raised before
the device is touched; the argument errors of the tensor and numpy layers; meta shapes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO

HEADER = os.path.join(REPO, "include", "specenh_modes.h")
LIB = os.path.join(REPO, "spectrogram-enhancement_amd", "specenh", "libspecenh.so")


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(specenh_[a-z0-9_]+)\s*\(", src)))


def test_header_ctypes_table_exports_and_operators_agree():
    from specenh import _lib, ops  # noqa: F401  (ops registers the operators)

    names = declared_functions()
    assert names == ["specenh_herm_eig"]
    assert sorted(_lib.SIGNATURES_MODES) == names
    tables = [_lib.SIGNATURES, _lib.SIGNATURES_STFT_COMPLEX, _lib.SIGNATURES_SPECTRAL,
              _lib.SIGNATURES_CSM, _lib.SIGNATURES_MODES]
    for i, a in enumerate(tables):  # the five tables are pairwise disjoint
        for b in tables[i + 1:]:
            assert not set(a) & set(b)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (specenh_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    L = _lib.lib()
    for n, (res, args) in _lib.SIGNATURES_MODES.items():
        assert getattr(L, n).restype is res and list(getattr(L, n).argtypes) == args
    schemas = {op: str(getattr(torch.ops.specenh, op).default._schema)
               for op in ("herm_eig", "herm_eig_out")}
    assert schemas["herm_eig"] == "specenh::herm_eig(Tensor a, int k) -> (Tensor, Tensor)"
    assert schemas["herm_eig_out"] == ("specenh::herm_eig_out(Tensor a, int k, Tensor(a!)? w, "
                                       "Tensor(b!)? v, Tensor(c!)? sweeps) -> ()")
    src = open(HEADER).read()
    assert '#include "specenh.h"' in src
    nmax = int(re.search(r"#define SPECENH_HERM_EIG_MAX_N (\d+)", src).group(1))
    smax = int(re.search(r"#define SPECENH_HERM_EIG_MAX_SWEEPS (\d+)", src).group(1))
    assert nmax == _lib.HERM_EIG_MAX_N == 64
    assert smax == _lib.HERM_EIG_MAX_SWEEPS and 1 <= smax <= 64


def test_c_abi_argument_errors():
    """specenh_herm_eig validates before the device is touched: the pointers are never
    followed."""
    from specenh import _lib

    lib = _lib.lib()
    p = ctypes.c_void_p(4096)  # a non-null pointer that is never followed
    E = _lib.SPECENH_EINVAL

    def call(a=p, count=3, n=5, stride=25, k=2, w=p, v=p, sweeps=None):
        rc = lib.specenh_herm_eig(a, count, n, stride, k, w, v, sweeps, None)
        return rc, _lib.last_error()

    assert call(a=None) == (E, "null a")
    assert call(count=-1) == (E, "count must be >= 0")
    for n in (1, 0, -3, 65):
        assert call(n=n, stride=65 * 65, k=0) == (E, "n must be in [2, 64]")
    for k in (-1, 6):
        assert call(k=k) == (E, "k must be in [0, n]")
    assert call(stride=24) == (E, "matrix_stride < n * n")
    assert call(v=None) == (E, "null v with k > 0")
    assert call(k=0, w=None, v=None) == (E, "no output requested")
    assert call(a=ctypes.c_void_p(4100)) == (E, "a must be 8-byte aligned")
    assert call(v=ctypes.c_void_p(4100)) == (E, "v must be 8-byte aligned")
    # nothing to do, nothing touched: OK with null outputs
    assert call(count=0, k=0, w=None, v=None)[0] == _lib.SPECENH_OK
    assert call(count=0, w=None, v=None)[0] == _lib.SPECENH_OK


def test_python_argument_errors():
    from specenh import signal, spectral

    S = torch.zeros(3, 5, 5, dtype=torch.complex64)
    with pytest.raises(TypeError, match="torch.Tensor"):
        spectral.hermitian_modes(np.zeros((5, 5), np.complex64))
    with pytest.raises(ValueError, match="complex"):
        spectral.hermitian_modes(torch.zeros(3, 5, 5))
    with pytest.raises(ValueError, match=r"\[\.\.\., n, n\]"):
        spectral.hermitian_modes(torch.zeros(3, 5, 4, dtype=torch.complex64))
    with pytest.raises(ValueError, match=r"\[\.\.\., n, n\]"):
        spectral.hermitian_modes(torch.zeros(5, dtype=torch.complex64))
    for n in (1, 65):
        with pytest.raises(ValueError, match="n must be in"):
            spectral.hermitian_modes(torch.zeros(2, n, n, dtype=torch.complex64))
    for k in (-1, 6):
        with pytest.raises(ValueError, match="k must be in"):
            spectral.hermitian_modes(S, k)

    x = torch.zeros(2, 5, 4096)
    with pytest.raises(ValueError, match="noverlap must be less than nperseg."):
        spectral.array_modes(x, nperseg=256, noverlap=256)
    with pytest.raises(NotImplementedError, match="power of two"):
        spectral.array_modes(x, nperseg=200)
    with pytest.raises(ValueError, match="shorter than nperseg"):
        spectral.array_modes(torch.zeros(2, 5, 100), nperseg=256)
    with pytest.raises(ValueError, match="navg"):
        spectral.array_modes(x, navg=32)  # T = 31
    with pytest.raises(ValueError, match="channels must be in"):
        spectral.array_modes(torch.zeros(2, 1, 4096))
    with pytest.raises(ValueError, match="channels must be in"):
        spectral.array_modes(torch.zeros(1, 65, 4096))
    with pytest.raises(ValueError, match="channels, length"):
        spectral.array_modes(torch.zeros(4096))
    for k in (0, 6):
        with pytest.raises(ValueError, match=r"k must be in \[1, 5\]"):
            spectral.array_modes(x, k=k)
    with pytest.raises(ValueError, match="Trend type"):
        spectral.array_modes(x, detrend="quadratic")
    with pytest.raises(ValueError, match="scaling"):
        spectral.array_modes(x, scaling="power")
    with pytest.raises(TypeError, match="torch.Tensor"):
        spectral.array_modes(np.zeros((5, 4096)))

    xn = np.zeros((5, 4096))
    with pytest.raises(ValueError, match="noverlap must be less than nperseg."):
        signal.array_modes(xn, nperseg=256, noverlap=300)
    with pytest.raises(NotImplementedError, match="power of two"):
        signal.array_modes(xn, nperseg=200)
    with pytest.raises(ValueError, match="shorter than nperseg"):
        signal.array_modes(np.zeros((5, 100)), nperseg=256)
    with pytest.raises(ValueError, match="channels must be in"):
        signal.array_modes(np.zeros((1, 4096)))
    with pytest.raises(ValueError, match="k must be in"):
        signal.array_modes(xn, k=6)
    with pytest.raises(ValueError, match="at least 2-D"):
        signal.array_modes(np.zeros(4096))
    with pytest.raises(NotImplementedError, match="median"):
        signal.array_modes(xn, average="median")
    with pytest.raises(NotImplementedError, match="nfft"):
        signal.array_modes(xn, nperseg=256, nfft=512)
    with pytest.raises(NotImplementedError, match="two-sided"):
        signal.array_modes(xn, return_onesided=False)
    with pytest.raises(NotImplementedError, match="axis"):
        signal.array_modes(np.zeros((4096, 5, 2)), axis=0)
    with pytest.raises(NotImplementedError, match="complex"):
        signal.array_modes(np.zeros((5, 4096), dtype=np.complex64))


def test_cpu_tensors_are_refused_after_validation():
    from specenh import spectral

    S = torch.zeros(3, 5, 5, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spectral.hermitian_modes(S)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spectral.hermitian_modes(S[0], 5, return_sweeps=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spectral.array_modes(torch.zeros(2, 5, 4096))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spectral.array_modes(torch.zeros(5, 4096), k=3, navg=4)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.herm_eig(S, 2)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.herm_eig_out(S, 2, torch.zeros(3, 5),
                                       torch.zeros(3, 2, 5, dtype=torch.complex64), None)


def test_meta_shapes():
    m = torch.device("meta")
    a = torch.empty(3, 129, 4, 5, 5, dtype=torch.complex64, device=m)
    w, v = torch.ops.specenh.herm_eig(a, 2)
    assert w.shape == (3, 129, 4, 5) and w.dtype == torch.float32
    assert v.shape == (3, 129, 4, 2, 5) and v.dtype == torch.complex64
    w, v = torch.ops.specenh.herm_eig(a, 0)
    assert w.shape == (3, 129, 4, 5) and v.numel() == 0 and v.dtype == torch.complex64
    w, v = torch.ops.specenh.herm_eig(torch.empty(5, 5, dtype=torch.complex64, device=m), 5)
    assert w.shape == (5,) and v.shape == (5, 5)
