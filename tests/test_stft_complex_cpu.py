"""Host-side checks of the complex STFT / inverse STFT boundary (no GPU): the frame-count and
output-length entry points and the f / t grids against scipy.signal.stft / istft, and the
argument errors, which are all raised before a device is touched."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.signal
import torch

from conftest import REPO

HEADER = os.path.join(REPO, "include", "specenh_stft_complex.h")
LIB = os.path.join(REPO, "spectrogram-enhancement_amd", "specenh", "libspecenh.so")

# (L, nperseg, noverlap, window): the cases of tests/test_stft_complex_gpu.py
CASES = [
    (16512, 256, 128, "hann"),
    (4000, 64, 48, "hamm"),
    (5000, 256, 100, "hann"),
    (9000, 1024, 768, "hamm"),
    (20000, 4096, 2048, "hann"),
    (333, 64, 32, "hann"),
    (300, 64, 63, "hamm"),
    (640, 64, 0, "hamm"),
    (9000, 128, 96, "hann"),
    (12300, 512, 200, "hamm"),
    (20000, 2048, 1536, "hann"),
    (9010, 64, 48, "hamm"),
]
MODES = [("zeros", True), (None, True), ("zeros", False), (None, False)]


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(specenh_[a-z0-9_]+)\s*\(", src)))


def test_header_ctypes_table_exports_and_operators_agree():
    """include/specenh_stft_complex.h (the extension of the C-ABI in specenh.h), the ctypes
    table, the exported symbols and the operators are held in sync the way tests/test_capi.py
    and tests/test_ops_registry.py hold specenh.h."""
    from specenh import _lib

    names = declared_functions()
    assert names == ["specenh_istft", "specenh_istft_length", "specenh_stft_complex",
                     "specenh_stft_complex_frames"]
    assert sorted(_lib.SIGNATURES_STFT_COMPLEX) == names
    assert not set(_lib.SIGNATURES_STFT_COMPLEX) & set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (specenh_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    L = _lib.lib()
    for n, (res, args) in _lib.SIGNATURES_STFT_COMPLEX.items():
        assert getattr(L, n).restype is res and list(getattr(L, n).argtypes) == args
    for op in ("stft_complex", "stft_complex_out", "istft", "istft_out"):
        assert getattr(torch.ops.specenh, op).default._schema.name == f"specenh::{op}"


@pytest.mark.filterwarnings("ignore:NOLA condition failed")  # boundary=False on hann: lengths only
@pytest.mark.parametrize("L,nperseg,noverlap,window", CASES)
def test_frames_lengths_and_grids_match_scipy(L, nperseg, noverlap, window):
    from specenh import _lib, stft

    lib = _lib.lib()
    x = np.zeros(L)
    for boundary, padded in MODES:
        f, t, Z = scipy.signal.stft(x, fs=5e5, window=window, nperseg=nperseg, noverlap=noverlap,
                                    boundary=boundary, padded=padded)
        T = lib.specenh_stft_complex_frames(L, nperseg, noverlap, 0 if boundary is None else 1,
                                            int(padded))
        assert T == Z.shape[1], (boundary, padded)
        assert stft.complex_frame_count(L, nperseg, noverlap, boundary, padded) == T
        assert np.array_equal(stft.frequencies(nperseg, 5e5), f)
        assert np.array_equal(stft.stft_times(L, nperseg, noverlap, 5e5, boundary, padded), t)
        for inv_boundary in (True, False):
            ti, xi = scipy.signal.istft(Z, fs=5e5, window=window, nperseg=nperseg,
                                        noverlap=noverlap, boundary=inv_boundary)
            n = lib.specenh_istft_length(T, nperseg, noverlap, int(inv_boundary))
            assert n == xi.shape[0] == stft.istft_length(T, nperseg, noverlap, inv_boundary)


@pytest.mark.parametrize("case,frames,spans", [
    ((9000, 128, 96, "hann"), (283, 279, 282), 3),
    ((12300, 512, 200, "hamm"), (41, 39, 40), 4),
    ((20000, 2048, 1536, "hann"), (41, 37, 40), 5),
    ((9010, 64, 48, "hamm"), (565, 561, 564), 3),
])
def test_odd_size_cases_have_the_frames_and_spans_they_are_chosen_for(case, frames, spans):
    """The frame counts (boundary='zeros' padded, boundary=None padded, boundary='zeros'
    unpadded) and the inverse's workgroup count (4096 output samples each) that the comments
    of tests/test_stft_complex_gpu.py state: an odd and an even T per size, more than one
    span."""
    from specenh import stft

    L, n, nov, w = case
    got = tuple(stft.complex_frame_count(L, n, nov, b, p) for b, p in MODES[:3])
    assert got == frames
    assert -(-stft.istft_length(frames[0], n, nov, True) // 4096) == spans


def test_frame_count_errors():
    from specenh import _lib

    lib = _lib.lib()
    assert lib.specenh_stft_complex_frames(4096, 256, 256, 1, 1) == _lib.SPECENH_EINVAL
    assert lib.specenh_stft_complex_frames(100, 256, 128, 1, 1) == _lib.SPECENH_EINVAL
    assert lib.specenh_stft_complex_frames(4096, 256, 128, 2, 1) == _lib.SPECENH_EUNSUPPORTED
    assert lib.specenh_istft_length(10, 256, 300, 1) == _lib.SPECENH_EINVAL
    assert lib.specenh_istft_length(0, 256, 128, 1) == _lib.SPECENH_EINVAL


def test_stft_argument_errors():
    from specenh import signal, stft

    x = torch.zeros(2, 4096)
    with pytest.raises(ValueError, match="noverlap must be less than nperseg."):
        stft.stft(x, nperseg=256, noverlap=256)
    with pytest.raises(NotImplementedError, match="power of two"):
        stft.stft(x, nperseg=200)
    with pytest.raises(NotImplementedError, match="boundary"):
        stft.stft(x, nperseg=256, boundary="even")
    with pytest.raises(ValueError, match="shorter than nperseg"):
        stft.stft(torch.zeros(2, 100), nperseg=256)
    # the numpy layer: the same errors, and scipy arguments the GPU path does not cover
    xn = np.zeros(4096)
    with pytest.raises(ValueError, match="noverlap must be less than nperseg."):
        signal.stft(xn, nperseg=256, noverlap=300)
    with pytest.raises(NotImplementedError, match="power of two"):
        signal.stft(xn, nperseg=200)
    with pytest.raises(NotImplementedError, match="boundary"):
        signal.stft(xn, boundary="odd")
    with pytest.raises(ValueError, match="shorter than nperseg"):
        signal.stft(np.zeros(100), nperseg=256)
    with pytest.raises(NotImplementedError, match="nfft"):
        signal.stft(xn, nperseg=256, nfft=512)
    with pytest.raises(NotImplementedError, match="two-sided"):
        signal.stft(xn, return_onesided=False)
    with pytest.raises(NotImplementedError, match="axis"):
        signal.stft(np.zeros((4096, 2)), axis=0)


def test_istft_argument_errors():
    from specenh import signal, stft

    Z = torch.zeros(3, 129, 20, dtype=torch.complex64)
    with pytest.raises(ValueError, match="noverlap must be less than nperseg."):
        stft.istft(Z, noverlap=256)
    with pytest.raises(ValueError, match="nperseg"):
        stft.istft(Z, nperseg=128)
    with pytest.raises(NotImplementedError, match="power of two"):
        stft.istft(torch.zeros(3, 101, 20, dtype=torch.complex64))
    for shape in ((3, 127, 20), (3, 129, 19), (2, 129, 20), (129, 20)):
        with pytest.raises(ValueError, match="gain must be"):
            stft.istft(Z, gain=torch.zeros(shape))
    Zn = np.zeros((3, 129, 20), dtype=np.complex128)
    with pytest.raises(ValueError, match="gain must be"):
        signal.istft(Zn, gain=np.zeros((3, 130, 20)))
    with pytest.raises(NotImplementedError, match="two-sided"):
        signal.istft(Zn, input_onesided=False)
    with pytest.raises(NotImplementedError, match="axis"):
        signal.istft(Zn, time_axis=0, freq_axis=1)
    with pytest.raises(NotImplementedError, match="nfft"):
        signal.istft(Zn, nfft=512)


def test_cpu_tensors_are_refused_after_validation():
    from specenh import stft

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stft.stft(torch.zeros(2, 4096))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stft.istft(torch.zeros(2, 129, 20, dtype=torch.complex64))
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.stft_complex(torch.zeros(2, 4096), 256, 128, "hann", 1.0, 1, 0, 1, True)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.istft(torch.zeros(2, 129, 20, dtype=torch.complex64), None, 256, 128,
                                "hann", 1.0, 1, True)


def test_meta_shapes():
    m = torch.device("meta")
    Z = torch.ops.specenh.stft_complex(torch.empty(3, 5000, device=m), 256, 100, "hann", 1.0, 1, 0,
                                       1, True)
    assert Z.shape == (3, 129, 34) and Z.dtype == torch.complex64
    x = torch.ops.specenh.istft(torch.empty(3, 129, 34, device=m, dtype=torch.complex64), None,
                                256, 100, "hann", 1.0, 1, True)
    assert x.shape == (3, 5148) and x.dtype == torch.float32
