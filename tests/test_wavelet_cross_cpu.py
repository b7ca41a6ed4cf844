"""Host-side checks of the cross-wavelet / wavelet-coherence boundary (no GPU): the new header,
ctypes table, exports and operators in sync, the two older headers untouched; the argument
errors of the C entry, all raised before a device is touched; meta shapes; the Python argument
errors and the broadcasting of the leading dimensions; smoothing_windows and the sliding boxcar
against hand values; the sign convention; the host rule for the filters per workgroup; and the
preconditions of the GPU comparison: a float32 run of the overlap-save formulation stays within
a quarter of every bound at every parity configuration, and on the inputs used the propagated
coherence bound stays small while the coherence spans its range."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import wavelet_cross_local as xl
import wavelet_local as wl
from conftest import REPO

HEADER = os.path.join(REPO, "include", "specenh_wavelet_cross.h")
LIB = os.path.join(REPO, "spectrogram-enhancement_amd", "specenh", "libspecenh.so")
OPS = ("filterbank_cross", "filterbank_cross_out")


def header_source(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def test_header_ctypes_table_exports_and_operators_agree():
    from specenh import _lib, ops

    src = header_source()
    names = sorted(set(re.findall(r"\b(specenh_[a-z0-9_]+)\s*\(", src)))
    assert names == ["specenh_filterbank_cross", "specenh_filterbank_cross_chunk"]
    assert sorted(_lib.SIGNATURES_WAVELET_CROSS) == names
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STFT_COMPLEX, _lib.SIGNATURES_SPECTRAL,
                  _lib.SIGNATURES_CSM, _lib.SIGNATURES_MODES, _lib.SIGNATURES_BISPECTRUM,
                  _lib.SIGNATURES_WAVENUMBER, _lib.SIGNATURES_CORRELATION,
                  _lib.SIGNATURES_BEAMFORM, _lib.SIGNATURES_WAVELET):
        assert not set(_lib.SIGNATURES_WAVELET_CROSS) & set(table)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (specenh_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    L = _lib.lib()
    for n, (res, args) in _lib.SIGNATURES_WAVELET_CROSS.items():
        assert getattr(L, n).restype is res and list(getattr(L, n).argtypes) == args
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1)
        assert len(decl.split(",")) == len(args), n
    for op in OPS:
        assert getattr(torch.ops.specenh, op).default._schema.name == f"specenh::{op}"
    assert callable(ops.filterbank_cross_chunk)
    consts = dict(re.findall(r"#define\s+(SPECENH_XWT_[A-Z_]+)\s+(\d+)", src))
    assert consts == {"SPECENH_XWT_POINT": str(_lib.XWT_POINT),
                      "SPECENH_XWT_MEAN": str(_lib.XWT_MEAN)}
    assert (_lib.XWT_POINT, _lib.XWT_MEAN) == (xl.POINT, xl.MEAN)
    assert not re.findall(r"SPECENH_FB_[A-Z_]+", src)


def test_the_older_headers_are_untouched():
    """Nothing of the feature is declared in specenh_wavelet.h or specenh.h."""
    for name in ("specenh_wavelet.h", "specenh.h"):
        src = header_source(os.path.join(REPO, "include", name))
        assert "cross" not in " ".join(re.findall(r"\b(specenh_filterbank[a-z0-9_]*)\s*\(", src))
        assert "XWT" not in src


def test_c_abi_argument_errors():
    """Validation happens before the device is touched: the pointers are never followed."""
    from specenh import _lib

    lib = _lib.lib()
    p, q, r = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(16384)

    def call(tables=p, S=12, nfft=1024, lmax=256, x=q, y=r, batch=2, length=5000, xs=5000,
             ys=5000, hop=4, mode=0, sxy=p, sxx=q, syy=r):
        rc = lib.specenh_filterbank_cross(tables, S, nfft, lmax, x, y, batch, length, xs, ys, hop,
                                          mode, sxy, sxx, syy, None)
        return rc, _lib.last_error()

    E = _lib.SPECENH_EINVAL
    assert call(tables=None) == (E, "null tables")
    assert call(x=None) == (E, "null x")
    assert call(y=None) == (E, "null y")
    assert call(sxy=None) == (E, "null sxy")
    assert call(tables=ctypes.c_void_p(4100)) == (E, "tables must be 8-byte aligned")
    assert call(S=0) == (E, "nscales must be >= 1")
    for nfft in (0, 128, 300, 1000, 8192):
        assert call(nfft=nfft, lmax=10) == (E, "nfft must be 256, 512, 1024, 2048 or 4096")
    for lmax in (-1, 1025):
        assert call(nfft=4096, lmax=lmax) == (E, "lmax must be in [0, 1024]")
    assert call(batch=-1) == (E, "batch must be >= 0")
    for hop in (0, -3):
        assert call(hop=hop) == (E, "hop must be >= 1")
    assert call(hop=513) == (E, "2 lmax + hop must not exceed nfft")
    assert call(nfft=256, lmax=128, hop=1) == (E, "2 lmax + hop must not exceed nfft")
    for mode in (-1, 2):
        rc, msg = call(mode=mode)
        assert rc == E and "mode" in msg
    assert call(length=0, xs=0, ys=0) == (E, "length must be >= 1")
    assert call(length=3, xs=3, ys=3, hop=4, mode=1) == (E, "signal shorter than hop")
    assert call(xs=4999) == (E, "x_stride < length")
    assert call(ys=4999) == (E, "y_stride < length")
    for sxx, syy in ((None, r), (q, None)):
        rc, msg = call(sxx=sxx, syy=syy)
        assert rc == E and "both" in msg
    # nothing to do, nothing launched: with and without the powers, x passed as y
    assert call(batch=0)[0] == _lib.SPECENH_OK
    assert call(batch=0, sxx=None, syy=None)[0] == _lib.SPECENH_OK
    assert call(batch=0, y=q)[0] == _lib.SPECENH_OK
    assert call(batch=0, hop=512, mode=1)[0] == _lib.SPECENH_OK
    assert call(batch=0, length=3, xs=3, ys=3, hop=4, mode=0)[0] == _lib.SPECENH_OK


def meta_bank(S, nfft):
    return torch.empty(S + 1, nfft, dtype=torch.complex64, device="meta")


def test_meta_shapes():
    m = torch.device("meta")
    op, op_out = torch.ops.specenh.filterbank_cross, torch.ops.specenh.filterbank_cross_out
    T = meta_bank(12, 1024)
    hop = 7
    for length in (1, hop, hop + 1, 5 * hop - 1, 4096):
        x, y = torch.empty(3, length, device=m), torch.empty(3, length, device=m)
        sxy, sxx, syy = op(x, y, T, 256, hop, xl.POINT)
        To = (length - 1) // hop + 1
        assert sxy.shape == sxx.shape == syy.shape == (3, 12, To)
        assert To == xl.n_out(length, hop, xl.POINT)
        assert sxy.dtype == torch.complex64 and sxx.dtype == syy.dtype == torch.float32
        assert op_out(x, y, T, 256, hop, xl.POINT, torch.empty_like(sxy), None, None) is None
        if length < hop:
            with pytest.raises(ValueError, match="shorter than hop"):
                op(x, y, T, 256, hop, xl.MEAN)
            continue
        sxy, sxx, syy = op(x, y, T, 256, hop, xl.MEAN)
        assert sxy.shape == sxx.shape == syy.shape == (3, 12, length // hop)
        assert sxy.dtype == torch.complex64 and sxx.dtype == syy.dtype == torch.float32
    x = torch.empty(2, 1041, device=m)
    assert [op(x, x, T, 256, 1, k)[0].shape[-1] for k in (0, 1)] == [1041, 1041]
    assert [op(x, x, T, 256, 3, k)[1].shape[-1] for k in (0, 1)] == [347, 347]
    assert [op(x, x, T, 256, 512, k)[2].shape[-1] for k in (0, 1)] == [3, 2]
    with pytest.raises(ValueError, match="exceed nfft"):
        op(x, x, T, 256, 513, 0)
    with pytest.raises(ValueError, match="hop must be"):
        op(x, x, T, 256, 0, 0)
    with pytest.raises(ValueError, match="kind"):
        op(x, x, T, 256, 1, 2)
    with pytest.raises(ValueError, match="lmax"):
        op(x, x, T, 1025, 1, 0)
    with pytest.raises(ValueError, match="nfft must be"):
        op(x, x, meta_bank(3, 300), 10, 1, 0)
    with pytest.raises(ValueError, match="y must be"):
        op(x, torch.empty(2, 1040, device=m), T, 10, 1, 0)
    with pytest.raises(ValueError, match="y must be"):
        op(x, x.double(), T, 10, 1, 0)
    with pytest.raises(ValueError, match="float32"):
        op(x.double(), x.double(), T, 10, 1, 0)


def test_cpu_tensors_are_refused():
    from specenh import signal
    from specenh import wavelet as wv

    x = torch.zeros(2, 4096)
    T = torch.zeros(4, 1024, dtype=torch.complex64)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.filterbank_cross(x, x, T, 10, 1, 0)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.filterbank_cross_out(
            x, x, T, 10, 1, 0, torch.zeros(2, 3, 4096, dtype=torch.complex64), None, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wv.cross_wavelet(x, x, [4.0, 8.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wv.wavelet_coherence(x, x, [4.0, 8.0], hop=16)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            signal.wavelet_coherence(np.zeros(4096), np.zeros(4096), fs=1.0, freqs=[0.1], hop=16)


def test_python_argument_errors_and_broadcasting():
    from specenh import wavelet as wv

    bank = wv.FilterBank(wv.morlet_filters([2.0, 4.0]), device="cpu")   # host tables only
    x = torch.zeros(2, 64)
    with pytest.raises(TypeError, match="torch.Tensor"):
        wv.cross_filter_bank(np.zeros(64), x, bank)
    with pytest.raises(TypeError, match="torch.Tensor"):
        wv.cross_filter_bank(x, np.zeros(64), bank)
    with pytest.raises(TypeError, match="FilterBank"):
        wv.cross_filter_bank(x, x, bank.tables)
    with pytest.raises(ValueError, match="same length"):
        wv.cross_filter_bank(x, torch.zeros(2, 65), bank)
    with pytest.raises(ValueError, match="hop"):
        wv.cross_filter_bank(x, x, bank, hop=0)
    with pytest.raises(ValueError, match="hop"):
        wv.cross_filter_bank(x, x, bank, hop=2.5)
    with pytest.raises(ValueError, match="exceed nfft"):
        wv.cross_filter_bank(x, x, bank, hop=993)
    with pytest.raises(ValueError, match="shorter than hop"):
        wv.cross_filter_bank(x, x, bank, hop=65)
    with pytest.raises(ValueError, match="do not broadcast"):
        wv.cross_filter_bank(torch.zeros(2, 64), torch.zeros(3, 64), bank)
    for smooth in (0, 2, 2.5, [1, 3, 5], [1, 4], "x"):
        with pytest.raises(ValueError, match="smooth must be"):
            wv.wavelet_coherence(x, x, [2.0, 4.0], hop=4, smooth=smooth)
    # the leading dimensions broadcast: the refusal of host tensors comes after every shape check
    for xs, ys in (((2, 64), (64,)), ((3, 1, 64), (2, 64)), ((64,), (4, 2, 64))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            wv.cross_filter_bank(torch.zeros(xs), torch.zeros(ys), bank, hop=4)
    # ... and on meta tensors the operator gives the broadcast batch
    m = torch.device("meta")
    xm = torch.empty(3, 1, 64, device=m).expand(3, 2, 64).reshape(-1, 64)
    ym = torch.empty(2, 64, device=m).expand(3, 2, 64).reshape(-1, 64)
    T = torch.empty(3, 1024, dtype=torch.complex64, device=m)
    assert torch.ops.specenh.filterbank_cross(xm, ym, T, 16, 4, xl.MEAN)[0].shape == (6, 2, 16)


def test_smoothing_windows_hand_values():
    """period = 4 pi s / (w0 + sqrt(2 + w0^2)) = 1.0330436 s for w0 = 6; n = 2 floor(3 period /
    (2 hop)) + 1."""
    from specenh import wavelet as wv

    n = wv.smoothing_windows([1.0, 10.0, 40.0, 160.0], hop=16)
    assert n.dtype == np.int64 and n.shape == (4,)
    # 3 period / 32 = 0.097, 0.968, 3.87, 15.5
    assert n.tolist() == [1, 1, 7, 31]
    assert wv.smoothing_windows([40.0], hop=1).tolist() == [2 * 61 + 1]      # 3 * 41.32 / 2 = 61.98
    assert wv.smoothing_windows([40.0], hop=16, cycles=1.0).tolist() == [3]  # 41.32 / 32 = 1.29
    assert wv.smoothing_windows([40.0], hop=16, cycles=0.0).tolist() == [1]
    w8 = wv.smoothing_windows([30.0], hop=4, w0=8.0)   # period = 4 pi 30 / (8 + sqrt 66) = 23.38
    assert w8.tolist() == [2 * 8 + 1]                  # 3 * 23.38 / 8 = 8.77
    assert (wv.smoothing_windows(np.geomspace(1, 256, 50), hop=7) % 2 == 1).all()
    with pytest.raises(ValueError, match="hop"):
        wv.smoothing_windows([4.0], hop=0)


def test_sliding_boxcar_seven_element_hand_case():
    """Widths 1, 3, 5 and 7 on [1, 2, 4, 8, 16, 32, 64]: the ends are truncated and divided by
    the count of values present."""
    from specenh import wavelet as wv

    v = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0])
    want = np.array([
        v,
        [3 / 2, 7 / 3, 14 / 3, 28 / 3, 56 / 3, 112 / 3, 96 / 2],
        [7 / 3, 15 / 4, 31 / 5, 62 / 5, 124 / 5, 120 / 4, 112 / 3],
        [15 / 4, 31 / 5, 63 / 6, 127 / 7, 126 / 6, 124 / 5, 120 / 4]])
    widths = [1, 3, 5, 7]
    rows = np.tile(v, (4, 1))
    tol = 7 * np.finfo(np.float64).eps * v.sum()   # seven roundings of a running sum <= 127
    got = wv._boxcar(torch.from_numpy(rows.astype(np.float32)), widths)
    assert got.dtype == torch.float64 and np.abs(got.numpy() - want).max() <= tol
    assert np.abs(xl.boxcar(rows, widths) - want).max() <= tol
    # complex values and leading dimensions
    z = torch.from_numpy((rows * (1 - 2j)).astype(np.complex64))[None].expand(2, 4, 7)
    gz = wv._boxcar(z, widths)
    assert gz.dtype == torch.complex128 and gz.shape == (2, 4, 7)
    assert np.abs(gz.numpy() - want * (1 - 2j)).max() <= tol * abs(1 - 2j)
    # a width past both ends is the mean of the row
    assert np.abs(wv._boxcar(torch.from_numpy(rows[:1]), [15]).numpy() - v.mean()).max() <= tol


def test_sign_convention():
    """x = cos(w n), y = cos(w (n - d)) through Morlet at the scale of w: away from the ends
    Wy = e^{-iwd} Wx up to the negative-frequency term, so angle(conj(Wx) Wy) = -w d: a y that
    lags x has a negative phase. The taps run out to 6 s: the truncation at the default 4 s
    leaves a negative-frequency response near exp(-8) of a tap (tests/test_wavelet_cpu.py), which
    beats against the positive one at 3.5e-5 of the phase; at 6 s it is exp(-18)."""
    from specenh import wavelet as wv

    N, s, d = 600, 10.0, 3
    w = 2 * np.pi * float(wv.scale_to_frequency([s])[0])
    n = np.arange(N, dtype=np.float64)
    taps = wv.morlet_filters([s], support=6.0)
    L = taps[0].size // 2
    Wx = wl.filter_bank_direct(np.cos(w * n), taps)
    Wy = wl.filter_bank_direct(np.cos(w * (n - d)), taps)
    for hop, mode in ((1, xl.POINT), (8, xl.MEAN)):
        sxy = xl.cross(Wx, Wy, hop, mode)[0][0, 0]
        inner = slice((L + d) // hop + 1, (N - L) // hop - 1)
        err = np.abs(np.angle(sxy[inner] * np.exp(1j * w * d))).max()
        print(f"\n[sign convention, hop {hop} mode {mode}] |angle(Sxy) + w d| max {err:.2e} "
              f"(allowed 1e-6), w d = {w * d:.4f}")
        assert err <= 1e-6
    assert -w * d < -0.5   # a phase far from zero: the sign is tested


def test_chunk_rule_at_256_compute_units():
    """specenh_filterbank_cross_chunk is host arithmetic for cus > 0: the rule of the filter
    bank (16 filters a workgroup, halved down to 4 while the launch has fewer than two
    workgroups a compute unit) for the chunk bank, and its errors."""
    from specenh import _lib, ops

    cfg = wl.CHUNK_CFG
    for hop, mode in xl.CHUNK_CASES:
        for nb in (1, 2, 34, 35, 36, 51, 52, 56, 57, 85, 86, 87, 500, 65535, 70000):
            got = ops.filterbank_cross_chunk(cfg["S"], cfg["nfft"], cfg["lmax"], nb,
                                             cfg["length"], hop, mode, cus=256)
            want = wl.filters_per_workgroup(cfg["nfft"], cfg["lmax"], hop, xl.fb_mode(mode),
                                            cfg["length"], cfg["S"], nb, 256)
            assert got == want, (hop, mode, nb)

    def sc(hop, mode, nb, cus=256):
        return ops.filterbank_cross_chunk(33, 256, 32, nb, 401, hop, mode, cus)

    assert [sc(1, xl.POINT, nb) for nb in (1, 34, 35, 56, 57)] == [4, 4, 8, 8, 16]
    assert [sc(37, xl.MEAN, nb) for nb in (2, 51, 52, 85, 86)] == [4, 4, 8, 8, 16]
    assert sc(1, xl.POINT, 8, cus=32) == 16
    # the benchmark shape: 128 scales, 65,536 samples, hop 128, one pair and 64
    assert ops.filterbank_cross_chunk(128, 4096, 1024, 1, 65536, 128, xl.MEAN, 256) == 8
    assert ops.filterbank_cross_chunk(128, 4096, 1024, 64, 65536, 128, xl.MEAN, 256) == 16
    with pytest.raises(ValueError, match="mode"):
        sc(1, 2, 1)
    with pytest.raises(ValueError, match="shorter than hop"):
        ops.filterbank_cross_chunk(33, 4096, 32, 1, 401, 500, xl.MEAN, 256)
    with pytest.raises(ValueError, match="cus"):
        sc(1, 0, 1, cus=-1)
    assert _lib.lib().specenh_filterbank_cross_chunk(0, 256, 32, 1, 401, 1, 0, 256) == \
        _lib.SPECENH_EINVAL


@pytest.mark.parametrize("name", list(wl.CONFIGS))
def test_float32_restatement_meets_a_quarter_of_each_bound(name):
    """The precondition of tests/test_wavelet_cross_gpu.py: the overlap-save formulation in
    float32 stays within a quarter of the bound on sxy, sxx and syy against the float64 direct
    sum, so the bounds ask nothing of the kernel that float32 arithmetic cannot give."""
    Wx, Wy = xl.reference(name)
    assert Wx.dtype == np.complex128 and Wx.shape[0] == xl.B
    worst = np.zeros(3)
    for hop, mode in xl.cases(name):
        ref = xl.cross(Wx, Wy, hop, mode)
        errs = xl.compare(xl.restatement32(name, hop, mode), ref)
        worst = np.maximum(worst, errs)
        assert max(errs) <= xl.BOUND / 4, (hop, mode, errs)
    print(f"\n[cross spectrum float32 restatement {name}] max row error: sxy / sqrt(max sxx "
          f"max syy) {worst[0]:.2e}, sxx {worst[1]:.2e}, syy {worst[2]:.2e} "
          f"(bound {xl.BOUND / 4:.1e})")


@pytest.mark.parametrize("nfft", wl.NFFTS)
def test_coherence_allowance_and_range_on_the_inputs_used(nfft):
    """hop{nfft} at hops 16, 17, 37 and V: no element's allowed coherence error exceeds 2e-3,
    the coherence spans below 0.2 and above 0.9, and the float32 restatement uses a small part
    of the allowance."""
    name = f"hop{nfft}"
    Wx, Wy = xl.reference(name)
    lo, hi, peak, used = 1.0, 0.0, 0.0, 0.0
    for hop in wl.hops_of(name)[1:]:
        ref = xl.coherence(*xl.cross(Wx, Wy, hop, xl.MEAN))
        allow = xl.coherence_allowance(ref[0], ref[3], ref[4])
        assert np.isfinite(allow).all()
        f32 = xl.coherence(*xl.restatement32(name, hop, xl.MEAN))
        lo, hi = min(lo, ref[0].min()), max(hi, ref[0].max())
        peak = max(peak, allow.max())
        used = max(used, (np.abs(f32[0] - ref[0]) / allow).max())
    print(f"\n[coherence {name}] range {lo:.3f} .. {hi:.3f}, allowed error at most {peak:.2e} "
          f"(limit {xl.COH_ALLOWED_MAX:.0e}), float32 restatement uses {used:.1%} of it")
    assert peak <= xl.COH_ALLOWED_MAX
    assert lo < 0.2 and hi > 0.9
    assert used <= 0.25
