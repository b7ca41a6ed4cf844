"""Host-side checks of the block-averaged cross-correlation boundary (no GPU): the extension
header, ctypes table, exports and operators in sync; the workspace arithmetic and the argument
errors, all raised before a device is touched; meta shapes; the host functions (lags, the
window's lag product, time_delay, correlation_time) against closed forms; the sign convention
of the restatement of tests/correlation_local.py; and the precondition of the GPU comparison:
a float32 run of the FFT formulation stays within the bound against the float64 direct sum at
every parity configuration."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.signal
import torch

import correlation_local as cl
from conftest import REPO

HEADER = os.path.join(REPO, "include", "specenh_correlation.h")
LIB = os.path.join(REPO, "spectrogram-enhancement_amd", "specenh", "libspecenh.so")
OP_ARGS = (256, 128, "boxcar", 1.0, 0, 1)  # nperseg, noverlap, window, fs, density, constant
OPS = ("correlation", "correlation_out")


def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_ctypes_table_exports_and_operators_agree():
    from specenh import _lib, ops

    src = header_source()
    names = sorted(set(re.findall(r"\b(specenh_[a-z0-9_]+)\s*\(", src)))
    assert names == ["specenh_correlation", "specenh_correlation_workspace_bytes"]
    assert sorted(_lib.SIGNATURES_CORRELATION) == names
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STFT_COMPLEX, _lib.SIGNATURES_SPECTRAL,
                  _lib.SIGNATURES_CSM, _lib.SIGNATURES_MODES, _lib.SIGNATURES_BISPECTRUM,
                  _lib.SIGNATURES_WAVENUMBER):
        assert not set(_lib.SIGNATURES_CORRELATION) & set(table)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (specenh_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    L = _lib.lib()
    for n, (res, args) in _lib.SIGNATURES_CORRELATION.items():
        assert getattr(L, n).restype is res and list(getattr(L, n).argtypes) == args
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1)
        assert len(decl.split(",")) == len(args), n
    for op in OPS:
        assert getattr(torch.ops.specenh, op).default._schema.name == f"specenh::{op}"
    assert callable(ops.correlation_workspace)
    modes = dict(re.findall(r"#define\s+(SPECENH_CORR_[A-Z]+)\s+(\d+)", src))
    assert modes == {"SPECENH_CORR_RAW": str(_lib.CORR_RAW),
                     "SPECENH_CORR_COEFF": str(_lib.CORR_COEFF)}
    assert (_lib.CORR_RAW, _lib.CORR_COEFF, _lib.CORR_MAX_NPERSEG) == (0, 1, 2048)


class PlanHead(ctypes.Structure):  # csrc/stft_plan.hpp: int nperseg, noverlap, hop; ...
    _fields_ = [("nperseg", ctypes.c_int), ("noverlap", ctypes.c_int), ("hop", ctypes.c_int),
                ("rest", ctypes.c_byte * 256)]


def plan_ptr(plan):
    return ctypes.cast(ctypes.pointer(plan), ctypes.c_void_p)


def test_workspace_bytes_and_c_abi_argument_errors():
    """Validation happens before the device is touched: the plan is a host-side stand-in (the
    fields the validation reads lead the struct), the pointers are never followed."""
    from specenh import _lib

    lib = _lib.lib()
    plan = PlanHead(256, 128, 128)
    pp = plan_ptr(plan)
    wsb = lib.specenh_correlation_workspace_bytes
    rec = (256 + 3) * 8
    # L = 16512: T = 128 frames = 4 chunks of 32
    assert wsb(pp, 2, 16512, 0, 255) == 2 * 4 * rec
    assert wsb(pp, 2, 16512, 0, 0) == 2 * 4 * rec        # the lag range does not enter
    assert wsb(pp, 5, 16512, 33, 10) == 5 * 3 * 2 * rec  # 128 // 33 = 3 groups of 2 chunks
    assert wsb(pp, 5, 16512, 32, 10) == 0                # a group is one chunk: no workspace
    assert wsb(pp, 5, 16512, 9, 10) == 0
    assert wsb(pp, 0, 16512, 0, 10) == 0
    for bad, msg in (((None, 2, 16512, 0, 10), "null plan"),
                     ((pp, -1, 16512, 0, 10), "batch must be >= 0"),
                     ((pp, 2, 255, 0, 10), "signal shorter than nperseg"),
                     ((pp, 2, 16512, 129, 10), "navg exceeds the number of frames"),
                     ((pp, 2, 16512, 0, 256), "maxlag must be in [0, nperseg - 1]"),
                     ((pp, 2, 16512, 0, -1), "maxlag must be in [0, nperseg - 1]")):
        assert wsb(*bad) == 0 and _lib.last_error() == msg
    odd = PlanHead(200, 100, 100)
    assert wsb(plan_ptr(odd), 2, 16512, 0, 10) == 0 and "power of two" in _lib.last_error()
    big = PlanHead(4096, 2048, 2048)
    assert wsb(plan_ptr(big), 2, 1 << 20, 0, 10) == 0
    assert "4096 is not supported" in _lib.last_error() and "[64, 2048]" in _lib.last_error()

    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)  # non-null pointers, never followed

    def call(plan=pp, x=p, y=q, batch=2, length=16512, xs=16512, ys=16512, navg=0, maxlag=40,
             mode=1, out=p, en=None, ws=p, wsbytes=1 << 40):
        rc = lib.specenh_correlation(plan, x, y, batch, length, xs, ys, navg, maxlag, mode, out,
                                     en, ws, wsbytes, None)
        return rc, _lib.last_error()

    assert call(plan=None) == (_lib.SPECENH_EINVAL, "null plan")
    assert call(x=None) == (_lib.SPECENH_EINVAL, "null x")
    assert call(y=None) == (_lib.SPECENH_EINVAL, "null y")
    assert call(batch=-1) == (_lib.SPECENH_EINVAL, "batch must be >= 0")
    assert call(xs=16511) == (_lib.SPECENH_EINVAL, "x_stride < length")
    assert call(ys=16511) == (_lib.SPECENH_EINVAL, "y_stride < length")
    assert call(length=255, xs=255, ys=255) == (_lib.SPECENH_EINVAL,
                                                "signal shorter than nperseg")
    assert call(navg=129) == (_lib.SPECENH_EINVAL, "navg exceeds the number of frames")
    for M in (256, 1000, -1):
        assert call(maxlag=M) == (_lib.SPECENH_EINVAL, "maxlag must be in [0, nperseg - 1]")
    for mode in (-1, 2):
        rc, msg = call(mode=mode)
        assert rc == _lib.SPECENH_EINVAL and "mode" in msg
    assert call(out=None) == (_lib.SPECENH_EINVAL, "null out")
    assert call(ws=None) == (_lib.SPECENH_EINVAL, "null workspace")
    assert call(ws=ctypes.c_void_p(4104)) == (_lib.SPECENH_EINVAL,
                                              "workspace must be 16-byte aligned")
    assert call(wsbytes=2 * 4 * rec - 1) == (_lib.SPECENH_EINVAL, "workspace too small")
    rc, msg = call(plan=plan_ptr(big), length=1 << 20, xs=1 << 20, ys=1 << 20)
    assert rc == _lib.SPECENH_EUNSUPPORTED and "4096 is not supported" in msg
    rc, msg = call(plan=plan_ptr(odd))
    assert rc == _lib.SPECENH_EUNSUPPORTED and "power of two" in msg
    assert call(batch=0, ws=None)[0] == _lib.SPECENH_OK  # nothing to do, nothing launched


def test_python_argument_errors():
    from specenh import correlation as co
    from specenh import signal

    x = torch.zeros(2, 4096)
    with pytest.raises(NotImplementedError, match="4096 is not supported"):
        co.correlate(torch.zeros(2, 16384), torch.zeros(2, 16384), nperseg=4096)
    with pytest.raises(NotImplementedError, match="power of two"):
        co.correlate(x, x, nperseg=200)
    for M in (256, 300, -1, 2.5):
        with pytest.raises(ValueError, match="maxlag"):
            co.correlate(x, x, nperseg=256, maxlag=M)
    with pytest.raises(ValueError, match="navg"):
        co.correlate(x, x, navg=32)  # T = 31
    with pytest.raises(ValueError, match="same shape"):
        co.correlate(x, torch.zeros(2, 4000))
    with pytest.raises(ValueError, match="same shape and device"):
        co.correlate(x, torch.zeros(2, 4096, device="meta"))
    with pytest.raises(ValueError, match="shorter than nperseg"):
        co.correlate(torch.zeros(2, 100), torch.zeros(2, 100))
    with pytest.raises(ValueError, match="noverlap must be less than nperseg."):
        co.correlate(x, x, nperseg=256, noverlap=256)
    with pytest.raises(ValueError, match="Trend type"):
        co.correlate(x, x, detrend="quadratic")
    with pytest.raises(ValueError, match="normalize"):
        co.correlate(x, x, normalize="biased")
    with pytest.raises(TypeError, match="torch.Tensor"):
        co.correlate(x, np.zeros((2, 4096)))
    with pytest.raises(ValueError, match=r"\[2 M \+ 1\]"):
        co.time_delay(torch.zeros(3, 9), np.zeros(7))
    with pytest.raises(ValueError, match=r"\[2 M \+ 1\]"):
        co.correlation_time(torch.zeros(3, 8), np.zeros(8))
    with pytest.raises(ValueError, match="maxlag"):
        co.correlation_lags(-1)
    xn = np.zeros(4096)
    with pytest.raises(NotImplementedError, match="4096 is not supported"):
        signal.correlate(np.zeros(16384), np.zeros(16384), nperseg=4096)
    with pytest.raises(ValueError, match="same shape"):
        signal.correlate(xn, np.zeros(4000))
    with pytest.raises(ValueError, match="maxlag"):
        signal.correlate(xn, xn, maxlag=256)


def test_cpu_tensors_are_refused_after_validation():
    from specenh import correlation as co

    x = torch.zeros(2, 4096)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        co.correlate(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        co.correlate(x[0], x[1], navg=3, maxlag=8, normalize="raw", unbiased=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        co.autocorrelate(x, window="hann")
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.correlation(x, x, *OP_ARGS, 0, 40, 1)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.correlation_out(x, x, *OP_ARGS, 0, 40, 1, torch.zeros(2, 1, 81), None,
                                          None)


def test_meta_shapes():
    m = torch.device("meta")
    x = torch.empty(3, 16512, device=m)  # T = 128
    R, E = torch.ops.specenh.correlation(x, x, *OP_ARGS, 0, 255, 1)
    assert R.shape == (3, 1, 511) and E.shape == (3, 1, 2)
    assert R.dtype == E.dtype == torch.float32
    R, E = torch.ops.specenh.correlation(x, torch.empty_like(x), *OP_ARGS, 9, 0, 0)
    assert R.shape == (3, 14, 1) and E.shape == (3, 14, 2)
    with pytest.raises(ValueError, match="maxlag"):
        torch.ops.specenh.correlation(x, x, *OP_ARGS, 0, 256, 1)
    with pytest.raises(ValueError, match="mode"):
        torch.ops.specenh.correlation(x, x, *OP_ARGS, 0, 10, 2)
    with pytest.raises(NotImplementedError, match="4096 is not supported"):
        torch.ops.specenh.correlation(x, x, 4096, 2048, "boxcar", 1.0, 0, 1, 0, 10, 1)
    assert torch.ops.specenh.correlation_out(
        x, x, *OP_ARGS, 0, 40, 1, torch.empty(3, 1, 81, device=m),
        torch.empty(3, 1, 2, device=m), None) is None


def test_lags_and_the_window_lag_product():
    from specenh import correlation as co

    lags = co.correlation_lags(5, 2.0)
    assert lags.dtype == np.float64 and np.array_equal(lags, np.arange(-5, 6) / 2.0)
    full = scipy.signal.correlation_lags(64, 64)
    assert np.array_equal(co.correlation_lags(63), full)
    assert np.array_equal(co.correlation_lags(10), full[np.abs(full) <= 10])
    assert np.array_equal(co.correlation_lags(0, 7.0), [0.0])
    c = co.window_lag_product("boxcar", 64)
    assert c.dtype == np.float64 and np.array_equal(c, 64.0 - np.abs(np.arange(-63, 64)))
    assert np.array_equal(co.window_lag_product("boxcar", 64, 5), 64.0 - np.abs(np.arange(-5, 6)))
    # periodic hann, w[n] = (1 - cos(h n)) / 2 with h = 2 pi / N: with K = N - m terms and
    # D = sum_{j < m} cos(h j) = sin(h m / 2) cos(h (m - 1) / 2) / sin(h / 2),
    # c[m] = (K (1 + cos(h m) / 2) + 2 D - 1 + cos(h m) - sin(h m) / (2 tan h)) / 4; c[0] = 3 N / 8
    N = 128
    m = np.arange(N)
    h = 2 * np.pi / N
    D = np.sin(h * m / 2) * np.cos(h * (m - 1) / 2) / np.sin(h / 2)
    want = ((N - m) * (1 + np.cos(h * m) / 2) + 2 * D - 1 + np.cos(h * m)
            - np.sin(h * m) / (2 * np.tan(h))) / 4
    assert abs(want[0] - 3 * N / 8) < 1e-12
    got = co.window_lag_product("hann", N)
    np.testing.assert_allclose(got[N - 1:], want, rtol=0, atol=1e-11)
    assert np.array_equal(got, got[::-1])
    w = scipy.signal.get_window("hamm", 64)
    np.testing.assert_allclose(co.window_lag_product("hamm", 64),
                               scipy.signal.correlate(w, w, "full"), rtol=1e-13)


def test_time_delay_closed_forms():
    from specenh import correlation as co

    lags = co.correlation_lags(8, 4.0)  # a quarter of a second apart
    m = np.arange(-8, 9, dtype=np.float64)
    # a parabola is recovered exactly: peak 3 at m0 = 2.3 samples
    R = torch.tensor(np.stack([3.0 - 0.5 * (m - 2.3) ** 2, 1.0 - 0.1 * (m + 5.75) ** 2]))
    tau, peak = co.time_delay(R.reshape(1, 2, -1), lags)
    assert tau.shape == peak.shape == (1, 2) and tau.dtype == peak.dtype == torch.float64
    np.testing.assert_allclose(tau[0].numpy(), [2.3 / 4, -5.75 / 4], rtol=0, atol=1e-12)
    np.testing.assert_allclose(peak[0].numpy(), [3.0, 1.0], rtol=0, atol=1e-12)
    # a peak on the first or last lag is returned unrefined; float32 in, float64 out
    edge = torch.tensor(np.stack([m, -m]), dtype=torch.float32)
    tau, peak = co.time_delay(edge, lags)
    assert tau.dtype == torch.float64 and tau.tolist() == [2.0, -2.0] and peak.tolist() == [8.0, 8.0]
    # an isolated spike: the parabola through (0, 1, 0) keeps the lag
    spike = torch.zeros(17)
    spike[11] = 1.0
    tau, peak = co.time_delay(spike, lags)
    assert tau.shape == () and float(tau) == 3 / 4 and float(peak) == 1.0
    # a flat top of two equal lags and a single lag do not divide by zero
    tau, _ = co.time_delay(torch.ones(17), lags)
    assert float(tau) == -2.0
    tau, peak = co.time_delay(torch.tensor([[0.5]]), [0.0])
    assert tau.tolist() == [0.0] and peak.tolist() == [0.5]


def test_correlation_time_closed_forms():
    from specenh import correlation as co

    lags = co.correlation_lags(10, 2.0)
    m = np.abs(np.arange(-10, 11, dtype=np.float64))
    tri = 1.0 - m / 8.0            # crosses 1/e at 8 (1 - 1/e) samples, linear: exact
    slow = 1.0 - m / 40.0          # never below 1/e within 10 lags
    step = np.where(m < 3, 1.0, 0.0)  # from 1 at lag 2 to 0 at lag 3
    raw = 5.0 * tri                # an unnormalised auto-correlation: divided by its lag 0
    tc = co.correlation_time(torch.tensor(np.stack([tri, slow, step, raw])), lags)
    assert tc.shape == (4,) and tc.dtype == torch.float64
    want = 8 * (1 - 1 / math.e) / 2.0
    np.testing.assert_allclose(tc[[0, 3]].numpy(), [want, want], rtol=1e-12)
    assert torch.isnan(tc[1])
    np.testing.assert_allclose(float(tc[2]), (2 + (1 - 1 / math.e)) / 2.0, rtol=1e-12)
    assert torch.isnan(co.correlation_time(torch.zeros(2, 21), lags)).all()   # R[0] == 0
    assert torch.isnan(co.correlation_time(torch.ones(1, 1), [0.0])).all()    # no positive lag
    e = np.exp(-m / 4.0)           # 1/e at lag 4, to rounding
    tc = float(co.correlation_time(torch.tensor(e), lags))
    assert abs(tc - 4 / 2.0) < 1e-9


def test_sign_convention_y_delayed_peaks_at_positive_lag():
    """y = roll(x, d) (y[n] = x[n - d]) peaks at m = +d, in the restatement and in scipy's own
    lag axis."""
    from specenh import correlation as co

    rng = np.random.default_rng(3)
    x = rng.standard_normal(1024)
    kw = dict(window="boxcar", nperseg=128, noverlap=64, detrend="constant", maxlag=20)
    for d in (4, -7, 0):
        y = np.roll(x, d)
        ref = cl.correlation(x, y, **kw)
        assert ref["R"].shape == (1, 1, 41)
        assert int(ref["R"][0, 0].argmax()) - 20 == d
        rho = cl.coefficient(ref)
        assert np.abs(rho).max() <= 1.0 and rho[0, 0, 20 + d] > 0.8
        tau, _ = co.time_delay(torch.tensor(rho), co.correlation_lags(20))
        assert abs(float(tau[0, 0]) - d) < 0.5
        full = scipy.signal.correlate(y[:128], x[:128], "full")
        lags = scipy.signal.correlation_lags(128, 128)
        assert lags[np.argmax(full)] == d
    # the zero-energy rule
    zero = cl.correlation(np.ones(1024), x, **kw)
    assert not zero["Ex"].any() and not cl.coefficient(zero).any()


@pytest.mark.parametrize("cfg", cl.PARITY, ids=[cl.cfg_id(c) for c in cl.PARITY])
def test_float32_fft_restatement_meets_the_bound(cfg):
    """The precondition of tests/test_correlation_gpu.py: the FFT formulation in float32 meets
    the bound against the float64 direct sum, so the bound asks nothing of the kernel that
    float32 arithmetic cannot give."""
    ref = cl.reference(cfg)
    x, y = cl.signals(cfg[4], cfg[2])
    f32 = cl.correlation_fft32(x, y, **cl.ref_kw(cfg))
    assert f32.dtype == np.float32 and ref["R"].dtype == np.float64
    assert f32.shape == ref["R"].shape == cl.shape_of(cfg)
    assert (ref["Ex"] > 0).all() and (ref["Ey"] > 0).all()
    err = cl.compare(f32, ref["R"], np.sqrt(ref["Ex"] * ref["Ey"]))
    print(f"\n[correlation float32 restatement {cl.cfg_id(cfg)}] max |R - R_ref| / "
          f"sqrt(Ex Ey) = {err:.2e} (bound {cl.TOL:.0e}); max |rho| = "
          f"{np.abs(cl.coefficient(ref)).max():.3f}")
    assert err <= cl.TOL
