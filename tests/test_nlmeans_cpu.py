"""Host-side checks of non-local means (no GPU): the numpy restatement of tests/nlmeans_local.py
against a literal four-loop version and against properties of the formula; the extension
header, ctypes table and export in sync; every argument error of the C entry, returned before
a device is touched (the pointers are never followed); the operator's schema, meta shapes and
the refusal of CPU tensors; specenh.restoration."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import nlmeans_local as nl
from conftest import REPO

HEADER = os.path.join(REPO, "include", "specenh_nlmeans.h")
LIB = os.path.join(REPO, "spectrogram-enhancement_amd", "specenh", "libspecenh.so")
F32, F64 = 0, 3  # SPECENH_DTYPE_F32, SPECENH_DTYPE_F64
PTR = ctypes.c_void_p(4096)  # a non-null pointer that is never followed


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("params", [(3, 2, 0.1, 0.0), (5, 3, 0.3, 0.2), (1, 1, 0.5, 0.0)],
                         ids=lambda p: f"P{p[0]}-D{p[1]}")
@pytest.mark.parametrize("shape", [(5, 4), (1, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_quotient64_against_the_four_loops(shape, params):
    """Images smaller than the halo: np.pad's iterated reflection against the index loop."""
    u = nl.noise_image(*shape, seed=11)
    q = nl.quotient64(u, *params)
    b = nl.brute(u, *params)
    err = float(np.abs(q - b).max())
    print(f"\n[nlmeans restatement {shape} {params}] max |quotient64 - brute| = {err:.3e}")
    assert q.shape == shape and q.dtype == np.float64
    assert err <= 1e-13


def test_a_stack_of_images_equals_the_single_images():
    u = np.stack([nl.noise_image(6, 9, 1), nl.smooth_image(6, 9, 2), nl.ridge_image(6, 9, 3)])
    q, B = nl.quotient64_and_bound(u, 3, 2, 0.1, 0.05)
    for i in range(3):
        qi, Bi = nl.quotient64_and_bound(u[i], 3, 2, 0.1, 0.05)
        assert np.array_equal(q[i], qi) and np.array_equal(B[i], Bi)


def test_distance_zero_is_the_identity():
    for maker in (nl.noise_image, nl.smooth_image, nl.ridge_image):
        u = maker(7, 10, seed=2)
        for P, h, sigma in ((7, 0.1, 0.0), (1, 0.5, 0.3), (9, 0.02, 0.0)):
            assert np.array_equal(nl.quotient64(u, P, 0, h, sigma), u.astype(np.float64))


def test_single_pixel_patch_and_large_h_is_the_box_mean_of_the_reflected_window():
    u = nl.noise_image(9, 12, seed=4)
    D = 2
    up = np.pad(u.astype(np.float64), D, mode="reflect")
    box = np.zeros(u.shape)
    for i in range(2 * D + 1):
        for j in range(2 * D + 1):
            box += up[i:i + 9, j:j + 12]
    box /= (2 * D + 1) ** 2
    assert np.abs(nl.quotient64(u, 1, D, 1e8, 0.0) - box).max() <= 1e-15


def test_output_lies_within_the_window_and_bounds_are_finite_and_positive():
    for maker in (nl.noise_image, nl.smooth_image, nl.ridge_image):
        u = maker(12, 17, seed=6)
        for P, D, h, sigma in ((7, 11, 0.1, 0.0), (5, 6, 0.08, 0.05), (3, 2, 0.02, 0.0),
                               (9, 15, 0.3, 0.2), (1, 1, 0.5, 0.0)):
            a, v = nl.terms(u, P, D, h, sigma)
            q, B = nl.quotient64_and_bound(u, P, D, h, sigma)
            assert (a >= 0).all() and a[a.shape[0] // 2].max() == 0.0   # the centre shift
            assert np.array_equal(v[a.shape[0] // 2], u.astype(np.float64))
            assert (q >= v.min(axis=0) - 1e-15).all() and (q <= v.max(axis=0) + 1e-15).all()
            assert np.isfinite(B).all() and (B > 0).all()
            assert B.max() < 1e-2                      # a bound, not a licence


def test_the_bound_constants_depend_on_the_patch_alone():
    assert [nl.c_d(P) for P in (1, 3, 5, 7, 9)] == [9, 17, 33, 57, 89] and nl.C_E == 4
    assert nl.EPS == 2.0 ** -24


def test_image_makers():
    for maker in (nl.noise_image, nl.smooth_image, nl.ridge_image):
        for shape in ((1, 1), (9, 1), (16, 24)):
            u = maker(*shape, seed=3)
            assert u.dtype == np.float32 and u.shape == shape
            assert u.min() >= 0.0 and u.max() <= 1.0
            assert np.array_equal(u, maker(*shape, seed=3))


# ---------------------------------------------------------------- library boundary
def header_source():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _ctype_of(param):
    param = " ".join(param.split())
    if "*" in param:
        return ctypes.c_void_p
    if param.startswith("long long"):
        return ctypes.c_longlong
    if param.startswith("double"):
        return ctypes.c_double
    if param.startswith("int"):
        return ctypes.c_int
    raise AssertionError(param)


def test_header_ctypes_table_and_exports_agree():
    from specenh import _lib

    src = header_source()
    assert sorted(set(re.findall(r"\b(specenh_[a-z0-9_]+)\s*\(", src))) == ["specenh_nlmeans"]
    assert sorted(_lib.SIGNATURES_NLMEANS) == ["specenh_nlmeans"]
    assert not set(_lib.SIGNATURES_NLMEANS) & set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    assert "specenh_nlmeans" in set(re.findall(r"\bT (specenh_[a-z0-9_]+)", out))
    fn = _lib.lib().specenh_nlmeans
    res, args = _lib.SIGNATURES_NLMEANS["specenh_nlmeans"]
    assert fn.restype is res is ctypes.c_int and list(fn.argtypes) == args
    m = re.search(r"int\s+specenh_nlmeans\s*\(([^)]*)\)", src)
    assert [_ctype_of(p) for p in m.group(1).split(",")] == args
    consts = dict(re.findall(r"#define\s+(SPECENH_NLMEANS_[A-Z_]+)\s+(\d+)", src))
    assert consts == {"SPECENH_NLMEANS_MAX_PATCH": str(_lib.NLMEANS_MAX_PATCH),
                      "SPECENH_NLMEANS_MAX_DISTANCE": str(_lib.NLMEANS_MAX_DISTANCE),
                      "SPECENH_NLMEANS_TILE_ROWS": str(_lib.NLMEANS_TILE_ROWS),
                      "SPECENH_NLMEANS_TILE_COLS": str(_lib.NLMEANS_TILE_COLS)}
    assert (_lib.NLMEANS_MAX_PATCH, _lib.NLMEANS_MAX_DISTANCE) == (9, 15)
    assert _lib.NLMEANS_TILE_ROWS * _lib.NLMEANS_TILE_COLS % 256 == 0   # 256 threads a tile


def test_argument_errors():
    from specenh import _lib

    L = _lib.lib()
    E, U = _lib.SPECENH_EINVAL, _lib.SPECENH_EUNSUPPORTED

    def call(dt=F32, S=PTR, B=2, r=8, c=6, st=48, P=7, D=11, h=0.1, sigma=0.0, out=PTR):
        return L.specenh_nlmeans(dt, S, B, r, c, st, P, D, h, sigma, out, None), _lib.last_error()

    for dt in (1, 2, 4, -1):  # bf16, f16 and unknown codes
        assert call(dt=dt) == (E, "filters take float32 or float64 spectrograms"), dt
    for r, c in ((0, 6), (-1, 6), (8, 0), (8, -3)):
        assert call(r=r, c=c, st=1 << 20) == (E, "bad shape"), (r, c)
    assert call(B=-1) == (E, "bad shape")
    for st in (47, 0, -48):
        assert call(st=st) == (E, "stride < rows*cols")
    assert call(S=None) == (E, "null pointer")
    assert call(out=None) == (E, "null pointer")
    nan, inf = float("nan"), float("inf")
    # with and without work to do: the parameters are checked before an empty batch returns
    for B, p in ((2, PTR), (0, None)):
        for P in (4, 0, -3, 2, 10):
            rc, msg = call(S=p, out=p, B=B, P=P)
            assert rc == E and "patch_size must be odd and positive" in msg, P
        for D in (-1, -16):
            rc, msg = call(S=p, out=p, B=B, D=D)
            assert rc == E and "patch_distance must not be negative" in msg, D
        for h in (0.0, -0.1, nan, inf, -inf):
            rc, msg = call(S=p, out=p, B=B, h=h)
            assert rc == E and "h must be finite and positive" in msg, h
        for sigma in (-1.0, -1e-300, nan, inf, -inf):
            rc, msg = call(S=p, out=p, B=B, sigma=sigma)
            assert rc == E and "sigma must be finite and not negative" in msg, sigma
        for P in (11, 13, 2 ** 31 - 1):
            rc, msg = call(S=p, out=p, B=B, P=P)
            assert rc == U and f"patch_size {P}" in msg and "limit of 9" in msg, P
            with pytest.raises(NotImplementedError, match="limit of 9"):
                _lib.check(rc, "nl_means")
        for D in (16, 1000):
            rc, msg = call(S=p, out=p, B=B, D=D)
            assert rc == U and f"patch_distance {D}" in msg and "limit of 15" in msg, D
    # a dimension whose tile, halo and reflection arithmetic would leave an int
    for r, c in ((1, 2 ** 30), (2 ** 30, 1), (1, 2 ** 31 - 1), (2 ** 31 - 1, 1)):
        for B, p in ((1, PTR), (0, None)):
            rc, msg = call(S=p, out=p, B=B, r=r, c=c, st=2 ** 31)
            assert rc == U and "below 2^30" in msg, (r, c)
    assert call(S=None, out=None, B=0, r=1, c=2 ** 30 - 1, st=2 ** 30)[0] == _lib.SPECENH_OK
    with pytest.raises(ValueError, match="h must be finite"):
        _lib.check(call(h=0.0)[0], "nl_means")
    # nothing to do: nothing is touched, null pointers are fine; the shape is still checked
    for dt in (F32, F64):
        for P, D, h, sigma in ((7, 11, 0.1, 0.0), (9, 15, 0.3, 0.2), (1, 0, 1e-30, 0.0)):
            assert call(dt=dt, S=None, out=None, B=0, P=P, D=D, h=h, sigma=sigma)[0] == 0
    assert call(S=None, out=None, B=0, st=55)[0] == _lib.SPECENH_OK
    assert call(S=None, out=None, B=0, r=0)[0] == E
    assert call(S=None, out=None, B=0, st=47)[0] == E


# ---------------------------------------------------------------- Python layer
def test_operator_and_schema():
    import specenh  # noqa: F401

    s = torch.ops.specenh.nl_means.default._schema
    assert str(s) == ("specenh::nl_means(Tensor S, int patch_size, int patch_distance, float h, "
                      "float sigma) -> Tensor")


def test_meta_shapes():
    import specenh  # noqa: F401

    m = torch.device("meta")
    for dt in (torch.float32, torch.float64):
        for shape in ((3, 40, 70), (40, 70), (0, 8, 8)):
            y = torch.ops.specenh.nl_means(torch.empty(shape, device=m, dtype=dt), 7, 11, 0.1, 0.0)
            assert y.shape == shape and y.dtype == dt and y.is_contiguous()
    padded = torch.empty(3, 40 * 70 + 13, device=m)[:, :2800].view(3, 40, 70)
    y = torch.ops.specenh.nl_means(padded, 5, 6, 0.08, 0.05)
    assert y.shape == (3, 40, 70) and y.is_contiguous()
    for bad in ((8,), (2, 3, 8, 8), (3, 0, 8)):
        with pytest.raises(ValueError):
            torch.ops.specenh.nl_means(torch.empty(bad, device=m), 7, 11, 0.1, 0.0)


def test_cpu_tensors_are_refused():
    from specenh import filters, restoration

    with pytest.raises(NotImplementedError):
        torch.ops.specenh.nl_means(torch.zeros(1, 8, 8), 7, 11, 0.1, 0.0)
    for f in (filters.nl_means, restoration.denoise_nl_means):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(torch.zeros(8, 8))
        with pytest.raises(ValueError, match="nl_means takes one 2-D image"):
            f(np.zeros((2, 8, 8)))
        for kw in ({"patch_size": 7.5}, {"patch_distance": 11.0}):   # not truncated
            with pytest.raises(TypeError):
                f(np.zeros((8, 8)), **kw)
            with pytest.raises(TypeError):
                f(torch.zeros(8, 8), **kw)
    if not torch.cuda.is_available():   # numpy input is uploaded: without a GPU there is nowhere
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            restoration.denoise_nl_means(np.zeros((8, 8), np.float32), h=0.2)


def test_restoration_module():
    import inspect

    import specenh
    from specenh import restoration

    assert specenh.restoration is restoration and "specenh.restoration" in specenh.__doc__
    sig = inspect.signature(restoration.denoise_nl_means)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [
        ("patch_size", 7), ("patch_distance", 11), ("h", 0.1), ("fast_mode", True), ("sigma", 0.0)]
    with pytest.raises(NotImplementedError, match="fast_mode=True"):
        restoration.denoise_nl_means(np.zeros((8, 8)), fast_mode=False)
    with pytest.raises(NotImplementedError, match="fast_mode=True"):
        restoration.denoise_nl_means(torch.zeros(8, 8), 7, 11, 0.1, False)
