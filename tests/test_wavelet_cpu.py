"""Host-side checks of the filter-bank / wavelet boundary (no GPU): the extension header,
ctypes table, exports and operators in sync; the host-built tables against np.fft.fft; the
argument errors, all raised before a device is touched; meta shapes; the host functions
(scales, frequencies, Morlet taps, cone of influence) against closed forms; the sign convention
of the restatement of tests/wavelet_local.py; and the precondition of the GPU comparison: a
float32 run of the overlap-save formulation stays within a quarter of the bound against the
float64 direct sum at every parity configuration."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import wavelet_local as wl
from conftest import REPO

HEADER = os.path.join(REPO, "include", "specenh_wavelet.h")
LIB = os.path.join(REPO, "spectrogram-enhancement_amd", "specenh", "libspecenh.so")
OPS = ("filterbank", "filterbank_out")


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_ctypes_table_exports_and_operators_agree():
    from specenh import _lib, ops

    src = header_source()
    names = sorted(set(re.findall(r"\b(specenh_[a-z0-9_]+)\s*\(", src)))
    assert names == ["specenh_filterbank", "specenh_filterbank_nfft", "specenh_filterbank_tables",
                     "specenh_filterbank_tables_bytes"]
    assert sorted(_lib.SIGNATURES_WAVELET) == names
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STFT_COMPLEX, _lib.SIGNATURES_SPECTRAL,
                  _lib.SIGNATURES_CSM, _lib.SIGNATURES_MODES, _lib.SIGNATURES_BISPECTRUM,
                  _lib.SIGNATURES_WAVENUMBER, _lib.SIGNATURES_CORRELATION,
                  _lib.SIGNATURES_BEAMFORM):
        assert not set(_lib.SIGNATURES_WAVELET) & set(table)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (specenh_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    L = _lib.lib()
    for n, (res, args) in _lib.SIGNATURES_WAVELET.items():
        assert getattr(L, n).restype is res and list(getattr(L, n).argtypes) == args
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1)
        assert len(decl.split(",")) == len(args), n
    for op in OPS:
        assert getattr(torch.ops.specenh, op).default._schema.name == f"specenh::{op}"
    assert callable(ops.filterbank_tables) and callable(ops.filterbank_nfft)
    consts = dict(re.findall(r"#define\s+(SPECENH_FB_[A-Z_]+)\s+(\d+)", src))
    assert consts == {"SPECENH_FB_COMPLEX": str(_lib.FB_COMPLEX),
                      "SPECENH_FB_POWER": str(_lib.FB_POWER),
                      "SPECENH_FB_POWER_MEAN": str(_lib.FB_POWER_MEAN),
                      "SPECENH_FB_MAX_HALF": str(_lib.FB_MAX_HALF)}
    assert (_lib.FB_COMPLEX, _lib.FB_POWER, _lib.FB_POWER_MEAN) == (wl.COMPLEX, wl.POWER, wl.MEAN)
    assert _lib.FB_NFFT == wl.NFFTS and _lib.FB_MAX_HALF == wl.MAX_HALF


def test_default_transform_length():
    from specenh import _lib, ops

    for lmax in (0, 1, 255, 256, 257, 512, 513, 1023, 1024):
        assert ops.filterbank_nfft(lmax) == ops.filterbank_nfft(lmax, 0) == wl.default_nfft(lmax)
    assert ops.filterbank_nfft(256) == 1024 and ops.filterbank_nfft(257) == 2048
    assert ops.filterbank_nfft(1024) == 4096
    assert ops.filterbank_nfft(100, 256) == 256 and ops.filterbank_nfft(127, 256) == 256
    with pytest.raises(ValueError, match="exceed nfft"):
        ops.filterbank_nfft(128, 256)
    with pytest.raises(ValueError, match="lmax"):
        ops.filterbank_nfft(1025)
    with pytest.raises(ValueError, match="nfft must be"):
        ops.filterbank_nfft(10, 300)
    assert _lib.lib().specenh_filterbank_tables_bytes(7, 512) == 8 * 8 * 512
    assert _lib.lib().specenh_filterbank_tables_bytes(7, 500) == 0
    assert "nfft must be" in _lib.last_error()
    assert _lib.lib().specenh_filterbank_tables_bytes(0, 512) == 0


@pytest.mark.parametrize("nfft", wl.NFFTS)
def test_tables_against_numpy_fft(nfft):
    """Random complex (non-Hermitian) taps: row s is np.fft.fft of the wrapped taps to the
    rounding to fp32 (half an ulp of each component, and what the fp64 transform itself
    loses, far below it); the last row is exp(-2 pi i n / nfft)."""
    from specenh import ops

    lm = min(wl.MAX_HALF, (nfft - 1) // 2)
    hl = [0, 1, lm // 3, lm]
    taps = wl.random_bank(hl, seed=nfft)
    T = ops.filterbank_tables(np.concatenate(taps), hl, nfft, device="cpu")
    assert T.shape == (len(hl) + 1, nfft) and T.dtype == torch.complex64
    got = T.numpy().astype(np.complex128)
    want = wl.tables64(taps, nfft)
    top = np.abs(want).max()
    for part in (np.real, np.imag):
        err = np.abs(part(got[:-1]) - part(want))
        assert (err <= 2.0 ** -24 * np.abs(part(want)) + 1e-14 * top).all()
    n = np.arange(nfft)
    tw = np.exp(-2j * np.pi * n / nfft)
    assert np.abs(got[-1] - tw).max() <= 2.0 ** -24
    assert got[-1, 0] == 1.0 and got[-1, nfft // 4].imag == -1.0 and got[-1, nfft // 2].real == -1.0
    # L = 0: the transform of a single tap is that tap at every bin
    assert (T[0] == complex(np.complex64(taps[0][0]))).all()


def test_table_argument_errors():
    from specenh import _lib, ops

    h3 = np.ones(3, dtype=np.complex128)
    with pytest.raises(ValueError, match="nfft must be"):
        ops.filterbank_tables(h3, [1], 300, device="cpu")
    with pytest.raises(ValueError, match="2 L_s \\+ 1"):
        ops.filterbank_tables(h3, [2], 256, device="cpu")
    with pytest.raises(ValueError, match="at least one"):
        ops.filterbank_tables(np.zeros(0), [], 256, device="cpu")
    with pytest.raises(ValueError, match="longer than nfft"):
        ops.filterbank_tables(np.ones(257, dtype=np.complex128), [128], 256, device="cpu")
    with pytest.raises(ValueError, match=r"\[0, 1024\]"):
        ops.filterbank_tables(np.ones(2051, dtype=np.complex128), [1025], 4096, device="cpu")
    L = _lib.lib()
    hl = (ctypes.c_int * 1)(1)
    tp = (ctypes.c_double * 6)()
    buf = ctypes.create_string_buffer(2 * 256 * 8)
    assert L.specenh_filterbank_tables(1, None, tp, 256, buf) == _lib.SPECENH_EINVAL
    assert _lib.last_error() == "null half_lengths"
    assert L.specenh_filterbank_tables(1, hl, None, 256, buf) == _lib.SPECENH_EINVAL
    assert _lib.last_error() == "null taps"
    assert L.specenh_filterbank_tables(1, hl, tp, 256, None) == _lib.SPECENH_EINVAL
    assert _lib.last_error() == "null tables"
    assert L.specenh_filterbank_tables(0, hl, tp, 256, buf) == _lib.SPECENH_EINVAL
    assert L.specenh_filterbank_tables(1, hl, tp, 256, buf) == _lib.SPECENH_OK


def test_c_abi_argument_errors():
    """Validation happens before the device is touched: the pointers are never followed."""
    from specenh import _lib

    lib = _lib.lib()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # non-null pointers, never followed

    def call(tables=p, S=12, nfft=1024, lmax=256, x=q, batch=2, length=5000, xs=5000, hop=4,
             mode=0, out=p):
        rc = lib.specenh_filterbank(tables, S, nfft, lmax, x, batch, length, xs, hop, mode, out,
                                    None)
        return rc, _lib.last_error()

    assert call(tables=None) == (_lib.SPECENH_EINVAL, "null tables")
    assert call(x=None) == (_lib.SPECENH_EINVAL, "null x")
    assert call(out=None) == (_lib.SPECENH_EINVAL, "null out")
    assert call(tables=ctypes.c_void_p(4100)) == (_lib.SPECENH_EINVAL,
                                                  "tables must be 8-byte aligned")
    assert call(S=0) == (_lib.SPECENH_EINVAL, "nscales must be >= 1")
    for nfft in (0, 128, 300, 1000, 8192):
        assert call(nfft=nfft, lmax=10) == (_lib.SPECENH_EINVAL,
                                            "nfft must be 256, 512, 1024, 2048 or 4096")
    for lmax in (-1, 1025):
        assert call(nfft=4096, lmax=lmax) == (_lib.SPECENH_EINVAL, "lmax must be in [0, 1024]")
    assert call(batch=-1) == (_lib.SPECENH_EINVAL, "batch must be >= 0")
    for hop in (0, -3):
        assert call(hop=hop) == (_lib.SPECENH_EINVAL, "hop must be >= 1")
    # 2 Lmax + hop > nfft: no whole hop fits a block
    assert call(hop=513) == (_lib.SPECENH_EINVAL, "2 lmax + hop must not exceed nfft")
    assert call(nfft=256, lmax=128, hop=1) == (_lib.SPECENH_EINVAL,
                                               "2 lmax + hop must not exceed nfft")
    assert call(nfft=4096, lmax=1024, hop=2049)[0] == _lib.SPECENH_EINVAL
    for mode in (-1, 3):
        rc, msg = call(mode=mode)
        assert rc == _lib.SPECENH_EINVAL and "mode" in msg
    assert call(length=0, xs=0) == (_lib.SPECENH_EINVAL, "length must be >= 1")
    assert call(length=3, xs=3, hop=4, mode=2) == (_lib.SPECENH_EINVAL,
                                                   "signal shorter than hop")
    assert call(xs=4999) == (_lib.SPECENH_EINVAL, "x_stride < length")
    # nothing to do, nothing launched; the largest legal hop passes the checks
    assert call(batch=0)[0] == _lib.SPECENH_OK
    assert call(batch=0, hop=512)[0] == _lib.SPECENH_OK
    assert call(batch=0, length=3, xs=3, hop=4, mode=0)[0] == _lib.SPECENH_OK


def meta_bank(S, nfft):
    return torch.empty(S + 1, nfft, dtype=torch.complex64, device="meta")


def test_meta_shapes():
    m = torch.device("meta")
    op, op_out = torch.ops.specenh.filterbank, torch.ops.specenh.filterbank_out
    T = meta_bank(12, 1024)
    hop = 7
    for length in (1, hop, hop + 1, 5 * hop - 1, 4096):
        x = torch.empty(3, length, device=m)
        W = op(x, T, 256, hop, wl.COMPLEX)
        P = op(x, T, 256, hop, wl.POWER)
        To = (length - 1) // hop + 1
        assert W.shape == P.shape == (3, 12, To) == (3, 12, wl.n_out(length, hop, wl.COMPLEX))
        assert W.dtype == torch.complex64 and P.dtype == torch.float32
        assert op_out(x, T, 256, hop, wl.COMPLEX, torch.empty_like(W)) is None
        assert op_out(x, T, 256, hop, wl.POWER, torch.empty_like(P)) is None
        if length < hop:
            with pytest.raises(ValueError, match="shorter than hop"):
                op(x, T, 256, hop, wl.MEAN)
            continue
        M = op(x, T, 256, hop, wl.MEAN)
        assert M.shape == (3, 12, length // hop) and M.dtype == torch.float32
        assert op_out(x, T, 256, hop, wl.MEAN, torch.empty_like(M)) is None
    x = torch.empty(2, 1041, device=m)
    assert [op(x, T, 256, 1, k).shape[-1] for k in (0, 1, 2)] == [1041] * 3
    assert [op(x, T, 256, 3, k).shape[-1] for k in (0, 1, 2)] == [347, 347, 347]
    assert [op(x, T, 256, 512, k).shape[-1] for k in (0, 1, 2)] == [3, 3, 2]
    with pytest.raises(ValueError, match="exceed nfft"):
        op(x, T, 256, 513, 0)
    with pytest.raises(ValueError, match="hop must be"):
        op(x, T, 256, 0, 0)
    with pytest.raises(ValueError, match="kind"):
        op(x, T, 256, 1, 3)
    with pytest.raises(ValueError, match="lmax"):
        op(x, T, 1025, 1, 0)
    with pytest.raises(ValueError, match="nfft must be"):
        op(x, meta_bank(3, 300), 10, 1, 0)
    with pytest.raises(ValueError, match="tables must be"):
        op(x, torch.empty(4, 1024, device=m), 10, 1, 0)
    with pytest.raises(ValueError, match="float32"):
        op(x.double(), T, 10, 1, 0)


def test_cpu_tensors_are_refused():
    from specenh import wavelet as wv

    x = torch.zeros(2, 4096)
    T = torch.zeros(4, 1024, dtype=torch.complex64)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.filterbank(x, T, 10, 1, 0)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.filterbank_out(x, T, 10, 1, 0, torch.zeros(2, 3, 4096,
                                                                     dtype=torch.complex64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wv.cwt(x, [4.0, 8.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        wv.scalogram(x, [4.0, 8.0], hop=16)


def test_python_argument_errors():
    from specenh import wavelet as wv

    bank = wv.FilterBank(wv.morlet_filters([2.0, 4.0]), device="cpu")   # host tables only
    assert (bank.nscales, bank.lmax, bank.nfft) == (2, 16, 1024)
    assert bank.tables.shape == (3, 1024) and bank.block() == 992 and bank.block(5) == 990
    assert wv.FilterBank(wv.morlet_filters([2.0]), nfft=256, device="cpu", lmax=100).block() == 56
    x = torch.zeros(2, 64)
    with pytest.raises(ValueError, match="mode must be"):
        wv.filter_bank(x, bank, mode="abs")
    with pytest.raises(ValueError, match="hop"):
        wv.filter_bank(x, bank, hop=0)
    with pytest.raises(ValueError, match="hop"):
        wv.filter_bank(x, bank, hop=2.5)
    with pytest.raises(ValueError, match="exceed nfft"):
        wv.filter_bank(x, bank, hop=993)
    with pytest.raises(ValueError, match="shorter than hop"):
        wv.filter_bank(x, bank, hop=65, mode="mean_power")
    with pytest.raises(TypeError, match="torch.Tensor"):
        wv.filter_bank(np.zeros(64), bank)
    with pytest.raises(TypeError, match="FilterBank"):
        wv.filter_bank(x, bank.tables)
    with pytest.raises(ValueError, match="odd number"):
        wv.FilterBank([np.ones(4)], device="cpu")
    with pytest.raises(ValueError, match="at least one"):
        wv.FilterBank([], device="cpu")
    with pytest.raises(ValueError, match="L <= 1024"):
        wv.FilterBank([np.ones(2051)], device="cpu")
    with pytest.raises(ValueError, match="nfft must be one of"):
        wv.FilterBank([np.ones(3)], nfft=300, device="cpu")
    with pytest.raises(ValueError, match="exceed nfft"):
        wv.FilterBank([np.ones(257)], nfft=256, device="cpu")
    with pytest.raises(ValueError, match="shorter than the longest"):
        wv.FilterBank([np.ones(9)], device="cpu", lmax=3)
    with pytest.raises(ValueError, match="positive"):
        wv.morlet_filters([1.0, -2.0])
    with pytest.raises(ValueError, match="fmin"):
        wv.morlet_scales(10.0, 5.0, 100.0)


def test_scale_to_frequency_is_the_table_1_factor():
    """Torrence & Compo Table 1: the Fourier period of the Morlet wavelet is
    4 pi s / (w0 + sqrt(2 + w0^2)) = 1.03 s for w0 = 6."""
    from specenh import wavelet as wv

    f = wv.scale_to_frequency([1.0, 10.0, 40.0], fs=1.0)
    assert f.dtype == np.float64
    np.testing.assert_allclose(1.0 / f, 1.0330436477 * np.array([1.0, 10.0, 40.0]), rtol=1e-9)
    assert abs(1.0 / f[0] - 1.03) < 0.005
    np.testing.assert_allclose(wv.scale_to_frequency([8.0], fs=5e5), 5e5 * f[:1] / 8.0, rtol=1e-15)
    np.testing.assert_allclose(wv.scale_to_frequency([3.0], 2.0, w0=8.0),
                               2.0 * (8 + math.sqrt(66.0)) / (4 * math.pi * 3.0), rtol=1e-15)
    np.testing.assert_allclose(wv.frequency_to_scale(f, 1.0), [1.0, 10.0, 40.0], rtol=1e-14)


def test_morlet_filters_energy_symmetry_and_form():
    from specenh import wavelet as wv

    scales = [1.5, 4.0, 16.0, 64.0, 256.0]
    taps = wv.morlet_filters(scales)
    ours = wl.morlet(scales)
    for s, h, g in zip(scales, taps, ours):
        L = h.size // 2
        assert h.dtype == np.complex128 and L == math.ceil(4.0 * s)
        np.testing.assert_allclose(h, g, rtol=0, atol=1e-14)
        assert np.array_equal(h[::-1], np.conj(h))          # h[-m] = conj(h[m])
        assert h[L].imag == 0 and abs(h[L].real - math.pi ** -0.25 / math.sqrt(s)) < 1e-15
        # sum |h|^2 = pi^-1/2 / s sum exp(-m^2 / s^2): the Riemann sum of a Gaussian of unit
        # integral, short of 1 by the tails past 4 s, erfc(4) = 1.5e-8 (s = 1.5: and by the
        # sum's own aliasing term 2 exp(-pi^2 s^2) = 4.5e-10)
        e = (np.abs(h) ** 2).sum()
        assert 1.0 - 2.5e-8 < e < 1.0 + 1e-9, (s, e)
    assert len(wv.morlet_filters(3.0)[0]) == 25
    assert wv.morlet_filters([2.0], support=3.0)[0].size == 13


def test_morlet_scales_are_geometric_and_span_the_band():
    from specenh import wavelet as wv

    fs, fmin, fmax = 5e5, 2e3, 1e5
    s = wv.morlet_scales(fmin, fmax, fs, voices_per_octave=16)
    f = wv.scale_to_frequency(s, fs)
    np.testing.assert_allclose(s[1:] / s[:-1], 2.0 ** (1 / 16), rtol=1e-13)
    assert abs(f[0] - fmax) < 1e-9 * fmax
    assert f[-1] <= fmin * (1 + 1e-12) and f[-2] > fmin    # the first scale at or past fmin
    assert s.size == math.ceil(16 * math.log2(fmax / fmin)) + 1
    o = wv.morlet_scales(1.0, 8.0, 100.0, voices_per_octave=1)
    np.testing.assert_allclose(wv.scale_to_frequency(o, 100.0), [8.0, 4.0, 2.0, 1.0], rtol=1e-13)
    assert wv.morlet_scales(5.0, 5.0, 100.0).size == 1


def test_cone_of_influence_small_case():
    """length 10, hop 3: outputs at samples 0, 3, 6, 9, at distances 0, 3, 3, 0 from the nearer
    end. s = 1: sqrt 2 = 1.41 covers distance 0 only; s = 2: 2.83 < 3 likewise; s = 2.2: 3.11
    covers all four."""
    from specenh import wavelet as wv

    coi = wv.cone_of_influence([1.0, 2.0, 2.2], 10, 3)
    assert coi.dtype == bool and coi.shape == (3, 4)
    assert coi.tolist() == [[True, False, False, True], [True, False, False, True],
                            [True, True, True, True]]
    c1 = wv.cone_of_influence([2.0], 9)        # distances 0 1 2 3 4 3 2 1 0 against 2.83
    assert c1[0].tolist() == [True, True, True, False, False, False, True, True, True]


def test_sign_convention_of_the_restatement():
    """x = cos(w n): away from the ends W = (H_s(w) e^{iwn} + H_s(-w) e^{-iwn}) / 2 with
    H_s(w) = sum_m h_s[m] e^{-iwm}; for Morlet the positive-frequency term dominates at the
    scale of w (the wavelet is analytic up to exp(-w0^2 / 2))."""
    from specenh import wavelet as wv

    N, s = 600, 10.0
    w = 2 * np.pi * float(wv.scale_to_frequency([s])[0])
    n = np.arange(N, dtype=np.float64)
    taps = wv.morlet_filters([s, 2 * s])
    W = wl.filter_bank_direct(np.cos(w * n), taps)
    assert W.shape == (1, 2, N) and W.dtype == np.complex128
    for i, h in enumerate(taps):
        L = h.size // 2
        m = np.arange(-L, L + 1)
        Hp, Hm = (h * np.exp(-1j * w * m)).sum(), (h * np.exp(1j * w * m)).sum()
        want = 0.5 * (Hp * np.exp(1j * w * n) + Hm * np.exp(-1j * w * n))
        inner = slice(L, N - L)
        assert np.abs(W[0, i, inner] - want[inner]).max() < 1e-12
        if i == 0:
            # the truncation at 4 s leaves |H(-w)| near exp(-8) of a tap, not exp(-72)
            assert abs(Hp) > 1e3 * abs(Hm) and abs(Hp) > 1.0
    # a non-Hermitian bank tells a reversed or conjugated filter apart
    h = wl.random_bank([5], seed=1)[0]
    x = np.random.default_rng(0).standard_normal(64)
    W = wl.filter_bank_direct(x, [h])[0, 0]
    assert abs(W[20] - sum(h[m + 5] * x[20 - m] for m in range(-5, 6))) < 1e-13
    assert np.abs(W - wl.filter_bank_direct(x, [h[::-1]])[0, 0]).max() > 0.1
    assert np.abs(W - wl.filter_bank_direct(x, [np.conj(h)])[0, 0]).max() > 0.1


def test_filters_per_workgroup_restates_the_host_rule():
    """wl.filters_per_workgroup against the text of plan() in csrc/filterbank_block.hpp, the one
    place both entries take the rule from (the single-signal kernel gives no way to observe
    SC), its values at the MI355X's 256 CUs, and every chunk size reachable with the bank of
    test_filters_per_workgroup_do_not_change_a_bit at any CU count a device may have."""
    csrc = os.path.join(REPO, "spectrogram-enhancement_amd", "csrc")
    src = " ".join(open(os.path.join(csrc, "filterbank_block.hpp")).read().split())
    for line in ("constexpr int MAX_SC = 16;", "constexpr int MIN_SC = 4;",
                 "p.Vh = (nfft - 2 * lmax) / (int)hop;",
                 "p.To = mean ? length / hop : (length - 1) / hop + 1;",
                 "const long long nblk = (p.To + p.Vh - 1) / p.Vh;",
                 "const long long want = 2LL * cus;",
                 "const long long nb0 = batch < 65535 ? batch : 65535;",
                 "p.SC = MAX_SC; while (p.SC > MIN_SC && nblk * ((nscales + p.SC - 1) / p.SC) "
                 "* nb0 < want) p.SC /= 2;"):
        assert line in src, line
    # neither entry keeps a copy; each plans for the device it runs on, with its own mean mode
    for name, call in (("filterbank.hip", "const bool mean = mode == SPECENH_FB_POWER_MEAN;"),
                       ("filterbank.hip", "hop, mean, device_cus());"),
                       ("filterbank_cross.hip", "hop, mode == SPECENH_XWT_MEAN, device_cus());")):
        hip = " ".join(open(os.path.join(csrc, name)).read().split())
        assert "SC /= 2" not in hip and "(length - 1) / hop + 1" not in hip, name
        assert call in hip, (name, call)
    cfg = wl.CHUNK_CFG
    assert (cfg["nfft"], cfg["lmax"], cfg["length"], cfg["S"]) == (256, 32, 401, 33)

    def sc(hop, mode, B, cus):
        return wl.filters_per_workgroup(256, 32, hop, mode, 401, 33, B, cus)

    # hop 1 at 256 CUs: 3 blocks x 3, 5 or 9 chunks x B against 512
    assert wl.chunk_batches(1, wl.COMPLEX, 256) == (57, 35, 2)
    assert [sc(1, wl.COMPLEX, B, 256) for B in (1, 2, 34, 35, 56, 57, 65535, 70000)] == \
        [4, 4, 4, 8, 8, 16, 16, 16]
    assert wl.chunk_batches(5, wl.POWER, 256) == (57, 35, 2)
    assert wl.chunk_batches(37, wl.MEAN, 256) == (86, 52, 2)  # To = 10: two blocks of 5
    for cus in (32, 64, 104, 110, 120, 228, 256, 304):
        for hop, mode in wl.CHUNK_CASES:
            B16, B8, B4 = wl.chunk_batches(hop, mode, cus)
            assert B4 < B8 < B16
            assert [sc(hop, mode, B, cus) for B in (B16, B16 - 1, B8, B8 - 1, B4)] == \
                [16, 8, 8, 4, 4]
            esize = 8 if mode == wl.COMPLEX else 4
            assert B16 * 33 * wl.n_out(401, hop, mode) * esize < 10e6  # the largest output
    # the largest launch of the benchmark shape (128 scales, one 65,536-sample shot, hop 128)
    assert wl.filters_per_workgroup(4096, 1024, 128, wl.MEAN, 65536, 128, 1, 256) == 8
    assert wl.filters_per_workgroup(4096, 1024, 128, wl.MEAN, 65536, 128, 64, 256) == 16


@pytest.mark.parametrize("hop,mode", wl.CHUNK_CASES)
def test_float32_restatement_of_the_chunk_bank_meets_a_quarter_of_the_bound(hop, mode):
    """The precondition of the comparison test_filters_per_workgroup_do_not_change_a_bit makes
    with the direct sum: rows 0, 1 and the last of the 256-CU batch."""
    B16 = wl.chunk_batches(hop, mode, 256)[0]
    x, taps = wl.chunk_signal(B16)[[0, 1, B16 - 1]], wl.chunk_taps()
    f32 = wl.filter_bank_fft32(x, taps, wl.CHUNK_CFG["nfft"], wl.CHUNK_CFG["lmax"], hop, mode)
    err = wl.compare(f32, wl.filter_bank_direct(x, taps, hop, mode), mode)
    print(f"\n[chunk bank float32 restatement, hop {hop} mode {mode}] {err:.2e} "
          f"(bound {wl.bound(mode) / 4:.1e})")
    assert err <= wl.bound(mode) / 4


def test_hop_configurations_cover_both_mean_paths_at_every_nfft():
    for nfft in wl.NFFTS:
        name = f"hop{nfft}"
        n, lmax, spec, length, B, kind = wl.CONFIGS[name]
        V1 = nfft - 2 * lmax
        assert (n, lmax, length, B, kind) == (nfft, nfft // 8, 2 * V1 + 17, 2, "white")
        assert len(wl.taps_of(name)) == 5 and max(h.size // 2 for h in wl.taps_of(name)) == lmax
        assert wl.hops_of(name) == (1, 16, 17, 37, V1)
        runs = [-(-h // 16) for h in wl.hops_of(name)]   # P of csrc/filterbank.hip
        assert runs == [1, 1, 2, 3, V1 // 16] and V1 % 16 == 0
        assert wl.block_len(nfft, lmax, 37) < V1 and 37 % 16   # V rounds down, a partial run
        assert len(wl.cases(name)) == 15
    assert wl.CONFIGS["hop4096"][3] == 6161


@pytest.mark.parametrize("name", list(wl.CONFIGS))
def test_float32_overlap_save_restatement_meets_a_quarter_of_the_bound(name):
    """The precondition of tests/test_wavelet_gpu.py: the overlap-save formulation in float32
    stays within TOL / 4 of the float64 direct sum (twice that for the power modes), so the
    bound asks nothing of the kernel that float32 arithmetic cannot give."""
    nfft, lmax = wl.CONFIGS[name][:2]
    x, taps, W = wl.signal_of(name), wl.taps_of(name), wl.reference(name)
    assert x.dtype == np.float32 and W.dtype == np.complex128
    worst = {}
    for hop, mode in wl.cases(name):
        f32 = wl.filter_bank_fft32(x, taps, nfft, lmax, hop, mode)
        ref = wl.decimate(W, hop, mode)
        assert f32.shape == ref.shape == (x.shape[0], len(taps), wl.n_out(x.shape[1], hop, mode))
        err = wl.compare(f32, ref, mode)
        worst[mode] = max(worst.get(mode, 0.0), err)
        assert err <= wl.bound(mode) / 4, (hop, mode, err)
    print(f"\n[filter bank float32 restatement {name}] max row error / row max: "
          + ", ".join(f"mode {m}: {e:.2e}" for m, e in worst.items())
          + f" (bounds {wl.TOL / 4:.1e}, {wl.TOL / 2:.1e})")
