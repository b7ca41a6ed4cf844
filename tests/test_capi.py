"""CPU-side checks of the C-ABI boundary: the library loads, exports exactly the
symbols include/specenh.h declares, and its pure-host entry points behave."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "specenh.h")
LIB = os.path.join(REPO, "spectrogram-enhancement_amd", "specenh", "libspecenh.so")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(specenh_[a-z0-9_]+)\s*\(", src)))


def test_header_declares_the_boundary():
    names = declared_functions()
    for required in ("specenh_stft_plan_create", "specenh_stft_psd", "specenh_last_error"):
        assert required in names


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "run spectrogram-enhancement_amd/build.py first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (specenh_[a-z0-9_]+)", out))
    missing = [n for n in declared_functions() if n not in exported]
    assert not missing, missing


def test_ctypes_signature_table_matches_header():
    from specenh import _lib

    assert sorted(_lib.SIGNATURES) == declared_functions()


def test_library_loads_and_host_entry_points():
    from specenh import _lib

    L = _lib.lib()
    assert b"gfx950" in L.specenh_version()
    # T = (L - N) // (N - noverlap) + 1   (scipy.signal.spectrogram, no padding)
    assert L.specenh_stft_frames(65536, 1024, 768) == 253
    assert L.specenh_stft_frames(16512, 256, 128) == 128
    assert L.specenh_stft_frames(1_000_000, 512, 256) == 3905
    assert L.specenh_stft_frames(512, 512, 256) == 1
    assert L.specenh_stft_frames(100, 512, 256) < 0
    with pytest.raises(ValueError, match="noverlap"):
        _lib.check(L.specenh_stft_frames(4096, 256, 256))


def test_plan_create_validates_before_touching_the_device():
    from specenh import _lib

    L = _lib.lib()
    h = ctypes.c_void_p()
    w = (ctypes.c_double * 100)(*([1.0] * 100))
    rc = L.specenh_stft_plan_create(ctypes.byref(h), 100, 50, w, 1.0, 0, 2, 1e-11)
    assert rc == _lib.SPECENH_EUNSUPPORTED
    with pytest.raises(NotImplementedError, match="power of two"):
        _lib.check(rc)
    w = (ctypes.c_double * 256)(*([1.0] * 256))
    assert L.specenh_stft_plan_create(ctypes.byref(h), 256, 300, w, 1.0, 0, 2, 1e-11) == \
        _lib.SPECENH_EINVAL
    assert L.specenh_stft_plan_create(ctypes.byref(h), 256, 128, w, 1.0, 7, 2, 1e-11) == \
        _lib.SPECENH_EINVAL
    assert L.specenh_stft_plan_create(ctypes.byref(h), 256, 128, w, 1.0, 0, 9, 1e-11) == \
        _lib.SPECENH_EINVAL


def test_host_frequency_and_time_grids_bit_exact():
    import numpy as np
    import scipy.signal

    from specenh import stft

    x = np.zeros(65536)
    f, t, _ = scipy.signal.spectrogram(x, fs=500000, nperseg=1024, noverlap=768)
    assert np.array_equal(stft.frequencies(1024, 500000), f)
    assert np.array_equal(stft.times(65536, 1024, 768, 500000), t)
    assert np.array_equal(stft.get_window("hamm", 512), scipy.signal.get_window("hamm", 512))


@pytest.mark.parametrize("batch,m,n,start,stop,path", [
    (4096, 513, 256, 0, 16, "subspace"),      # C3 rank-16
    (4096, 513, 256, 1, 256, "subspace"),     # C3 default range
    (4096, 128, 128, 1, 128, "top1"),         # C5 default range, whole batch
    (2048, 128, 128, 1, 128, "top1"),         # the bench's C5 slice
    (4096, 513, 256, 0, 200, "eigen"),        # wide kept range: every matrix on the eigen path
    (1 << 16, 256, 3905, 1, 256, "subspace"),  # many production-shape spectrograms
])
def test_svd_workspace_bounded(batch, m, n, start, stop, path):
    """The eigen-path part of the SVD workspace is capped at 1 GiB whatever the batch
    (an 8 GB cap made C3 calls reserve 6.5 GB); the rest is the subspace path's
    G / V / theta (batch x r x r fp32) and per-matrix flags."""
    from specenh import _lib

    L = _lib.lib()
    r = min(m, n)
    ws = L.specenh_svd_denoise_workspace_bytes(batch, m, n, start, stop)
    per_matrix = r * r * 8 + 3 * r * 8 + 4 * r * (r // 2 + 2) * 8 + 24
    eig = min(batch, max(1, (1 << 30) // per_matrix)) * per_matrix + 256
    assert eig <= (1 << 30) + 256
    if path == "eigen":
        assert ws == eig
    elif path == "top1":  # top1 flags + eigen fallback (r = 128: the subspace layout)
        assert eig < ws <= eig + batch * (r * r + 8 * r + 8) * 4 + 8 * batch + 1024
    else:
        K = 16 if start == 0 else 1
        sub = batch * (r * r + r * K + K) * 4
        assert sub + eig <= ws <= sub + eig + 8 * batch + 1024


def test_svd_workspace_bytes_unchanged():
    """Both SVD workspace queries return exactly what the library did before the layout
    arithmetic moved into one place (tests/golden/svd_workspace_bytes.json, recorded by
    make_golden_svd_workspace.py from a build of the commit it names), over a grid that
    reaches every layout branch: top-1 with either fallback layout, subspace (direct,
    complement, with and without the eigen fallback), eigen path, no workspace."""
    import json

    from specenh import _lib

    L = _lib.lib()
    gold = json.load(open(os.path.join(REPO, "tests", "golden", "svd_workspace_bytes.json")))
    assert re.fullmatch(r"[0-9a-f]{40}", gold["commit"])
    batches = (1, 3, 70000)
    shapes = ((4, 4), (16, 16), (40, 24), (24, 40), (128, 128), (513, 256), (300, 300))
    want = {(b, m, n, s, e)
            for b in batches for m, n in shapes
            for s, e in ((1, min(m, n)), (0, 4), (0, min(m, n) - 2), (3, 3), (0, min(m, n)),
                         (2, -1))}
    rows = gold["denoise_workspace_bytes"]
    assert {tuple(r[:5]) for r in rows} == want
    bad = [(r, got) for r in rows
           if (got := L.specenh_svd_denoise_workspace_bytes(*r[:5])) != r[5]]
    assert not bad, bad[:5]
    rows = gold["svd_workspace_bytes"]
    assert {tuple(r[:3]) for r in rows} == {(b, m, n) for b in batches for m, n in shapes}
    assert {r[3] for r in rows} >= {1, 4, 16, 40, 41, 256, 300}
    bad = [(r, got) for r in rows if (got := L.specenh_svd_workspace_bytes(*r[:4])) != r[4]]
    assert not bad, bad[:5]


def test_python_boundary_rejects_cpu_tensors():
    import torch

    from specenh import stft

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stft.stft_psd(torch.zeros(2, 4096), 256, 128)


def test_variant_switches_read_once_and_settable():
    """Kernel-variant switches: known names round-trip through the C-ABI, unknown names are
    refused, and the environment is not consulted per launch (runtime.hpp)."""
    from specenh import _lib

    old = _lib.get_variant("CONV_NO_S2")
    with _lib.variant("SPECENH_CONV_NO_S2", 1):
        assert _lib.get_variant("CONV_NO_S2") == 1
        os.environ["SPECENH_CONV_NO_S2"] = "0"  # too late: read once per process
        try:
            assert _lib.get_variant("CONV_NO_S2") == 1
        finally:
            del os.environ["SPECENH_CONV_NO_S2"]
    assert _lib.get_variant("CONV_NO_S2") == old
    assert _lib.get_variant("PATCH_WSPLIT") in (-1, 0, 1)
    with pytest.raises(ValueError, match="unknown variant"):
        _lib.set_variant("NO_SUCH_SWITCH", 1)
    assert _lib.last_kernel_name() == ""  # nothing launched on this thread
