"""Host-side checks of the label-filter C ABI (csrc/filters.hip, no GPU): every argument
error of specenh_filter / specenh_quantfilt / specenh_gaussblr / specenh_morph is returned
before a HIP call is made (the pointers are never followed), batch 0 is a no-op, and the two
workspace-size functions follow the formulas the kernels' buffer layout implies."""
import ctypes

import pytest

F32, F64 = 0, 3  # SPECENH_DTYPE_F32, SPECENH_DTYPE_F64
P = ctypes.c_void_p(4096)  # a non-null pointer that is never followed
# quantfilt keeps 16 columns of `rows` elements in at most 160 KiB - 512 of LDS
QF_MAX_ROWS = {F64: (160 * 1024 - 512) // (16 * 8), F32: (160 * 1024 - 512) // (16 * 4)}


def _entry_points():
    """name -> call(dtype, S, batch, rows, cols, stride, out, ws) with valid other arguments."""
    from specenh import _lib

    L = _lib.lib()
    eps = {}
    for op, name in ((_lib.FILTER_NORM, "norm"), (_lib.FILTER_RESCALE, "rescale"),
                     (_lib.FILTER_MEANSUB, "meansub")):
        eps[name] = (lambda op: lambda dt, S, B, r, c, st, out, ws:
                     L.specenh_filter(op, dt, S, B, r, c, st, out, ws, None))(op)
    eps["quantfilt"] = lambda dt, S, B, r, c, st, out, ws: L.specenh_quantfilt(
        dt, S, B, r, c, st, 0.9, out, None)
    eps["gaussblr"] = lambda dt, S, B, r, c, st, out, ws: L.specenh_gaussblr(
        dt, S, B, r, c, st, 31, 3, 0.0, out, ws, None)
    eps["morph"] = lambda dt, S, B, r, c, st, out, ws: L.specenh_morph(
        dt, S, B, r, c, st, out, ws, None)
    return eps


NAMES = ["norm", "rescale", "meansub", "quantfilt", "gaussblr", "morph"]


@pytest.mark.parametrize("name", NAMES)
def test_common_argument_errors(name):
    from specenh import _lib

    f = _entry_points()[name]
    E = _lib.SPECENH_EINVAL

    def call(dt=F64, S=P, B=2, r=8, c=6, st=48, out=P, ws=P):
        return f(dt, S, B, r, c, st, out, ws), _lib.last_error()

    for dt in (1, 2, 4, -1):  # bf16, f16 and unknown codes
        assert call(dt=dt) == (E, "filters take float32 or float64 spectrograms"), dt
    for r, c in ((0, 6), (-1, 6), (8, 0), (8, -3)):
        assert call(r=r, c=c, st=1 << 20) == (E, "bad shape"), (r, c)
    assert call(B=-1) == (E, "bad shape")
    assert call(st=47) == (E, "stride < rows*cols")
    assert call(st=0) == (E, "stride < rows*cols")
    assert call(st=-48) == (E, "stride < rows*cols")
    assert call(S=None) == (E, "null pointer")
    assert call(out=None) == (E, "null pointer")
    if name != "quantfilt":  # quantfilt takes no workspace
        assert call(ws=None) == (E, "null workspace")
    for dt in (F32, F64):  # nothing to do: nothing is touched, null pointers are fine
        assert f(dt, None, 0, 8, 6, 48, None, None) == _lib.SPECENH_OK
        assert f(dt, None, 0, 8, 6, 55, None, None) == _lib.SPECENH_OK
    assert f(F64, None, 0, 0, 6, 48, None, None) == E  # the shape is still checked


def test_filter_unknown_op():
    from specenh import _lib

    L = _lib.lib()
    for op in (-1, 3, 99):
        assert L.specenh_filter(op, F64, P, 2, 8, 6, 48, P, P, None) == _lib.SPECENH_EINVAL
        assert _lib.last_error() == "unknown filter op"
        assert L.specenh_filter(op, F64, None, 0, 8, 6, 48, None, None, None) == _lib.SPECENH_EINVAL


def test_quantfilt_threshold_range():
    from specenh import _lib

    L = _lib.lib()
    for thr in (-1e-9, 1.0000001, -1.0, 2.0, float("nan"), float("inf"), float("-inf")):
        for B, p in ((2, P), (0, None)):
            rc = L.specenh_quantfilt(F64, p, B, 8, 6, 48, thr, p, None)
            assert rc == _lib.SPECENH_EINVAL, (thr, B)
            assert _lib.last_error() == "Quantiles must be in the range [0, 1]"
    for thr in (0.0, 1.0, 0.5):
        assert L.specenh_quantfilt(F32, None, 0, 8, 6, 48, thr, None, None) == _lib.SPECENH_OK


@pytest.mark.parametrize("dtype,name", [(F64, "float64"), (F32, "float32")])
def test_quantfilt_lds_row_limit(dtype, name):
    """The largest height is what 16 columns of the dtype fit in 160 KiB - 512 of LDS; the
    message names that dtype's limit."""
    from specenh import _lib

    L = _lib.lib()
    top = QF_MAX_ROWS[dtype]
    assert top == {F64: 1276, F32: 2552}[dtype]
    # batch 0 passes the argument checks and returns before any launch
    rc = L.specenh_quantfilt(dtype, None, 0, top, 17, top * 17, 0.9, None, None)
    assert rc == _lib.SPECENH_OK
    for rows in (top + 1, 2 * top, 1 << 20):
        for B, p in ((0, None), (3, P)):
            rc = L.specenh_quantfilt(dtype, p, B, rows, 17, rows * 17, 0.9, p, None)
            assert rc == _lib.SPECENH_EUNSUPPORTED, (rows, B)
            msg = _lib.last_error()
            assert f"rows <= {top}" in msg and name in msg, msg
            with pytest.raises(NotImplementedError, match=f"rows <= {top}"):
                _lib.check(rc, "quantfilt")


def test_gaussblr_kernel_sizes():
    from specenh import _lib

    L = _lib.lib()
    msg = "Gaussian kernel size must be odd, positive and <= 127"

    def call(kw, kh, B=2, p=P, sigma=0.0):
        return L.specenh_gaussblr(F32, p, B, 8, 6, 48, kw, kh, sigma, p, p, None)

    for bad in (0, 2, 4, 30, 126, 128, 129, 131, -1, -3):
        for kw, kh in ((bad, 3), (3, bad), (bad, bad)):
            for B, p in ((2, P), (0, None)):
                assert call(kw, kh, B, p) == _lib.SPECENH_EINVAL, (kw, kh, B)
                assert _lib.last_error() == msg
    for kw, kh in ((1, 1), (127, 127), (1, 127), (31, 3), (3, 31)):
        for sigma in (0.0, -1.0, 0.3, 7.5):
            assert call(kw, kh, 0, None, sigma) == _lib.SPECENH_OK, (kw, kh, sigma)


def _round256(n):
    return (n + 255) // 256 * 256


def test_workspace_formulas():
    """specenh_filter: {a, b} statistics per spectrogram and one mean per row, in fp64.
    u8 filters: the statistics (16 B a spectrogram), one uint16 plane and two uint8 planes,
    each rounded up to 256 B."""
    from specenh import _lib

    L = _lib.lib()
    fw, uw = L.specenh_filter_workspace_bytes, L.specenh_u8filter_workspace_bytes
    for B, rows in ((1, 1), (3, 37), (6, 128), (90000, 3), (2051, 128), (4096, 128), (1, 2552)):
        assert fw(B, rows) == B * (2 + rows) * 8, (B, rows)
    for B, rows in ((0, 8), (-1, 8), (4, 0), (4, -2)):
        assert fw(B, rows) == 16, (B, rows)
    for B, rows, cols in ((1, 1, 1), (3, 37, 29), (4, 128, 128), (226, 250, 300), (17, 1, 15),
                          (16, 4, 4), (1, 256, 3905)):
        n = B * rows * cols
        assert uw(B, rows, cols) == _round256(16 * B) + _round256(2 * n) + 2 * _round256(n), \
            (B, rows, cols)
    for B, rows, cols in ((0, 8, 8), (-2, 8, 8), (4, 0, 8), (4, 8, 0), (4, 8, -1)):
        assert uw(B, rows, cols) == 16, (B, rows, cols)
