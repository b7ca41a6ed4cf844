"""The label filters (csrc/filters.hip) at their grid, tile, LDS and batch edges.

The reference of every check is numpy on the same dtype: oracle/filters.py (np.quantile,
np.where, ...) for quantfilt / norm / rescale / meansub, its integer restatement for gaussblr /
morph; never the library's own output. Tolerances are those of tests/test_filters_gpu.py:
quantfilt, rescale, gaussblr and morph bit-exact (float32 rescale: atol 2e-7); norm / meansub
in fp64 1e-12 of the output range; float32 meansub atol 1e-6. That file states nothing for
float32 norm: the bound used here is derived in _f32_norm_bound and comes to about 1e-5
(never above 2e-5) on values within +-4. The float32 label chain gets no tolerance of its
own: its stages are held to the figures above, with the uint8 requantisation inside morph
bracketed from the oracle (_label_chain_oracle). quantfilt's fp64 lerp is fused by the
compiler (csrc/filters.hip); no input here has order statistics a few ulps apart in fp64,
where that could show.

The kernels are called through the C ABI wherever the test owns the buffers: the output is
filled with NaN (or a sentinel) before the launch and the workspace is exactly what the size
function returns, filled with 0xFF (NaN doubles) and followed by a 256-byte guard that must
come back unchanged, so no result depends on what the allocator hands back."""
import ctypes
import warnings

import numpy as np
import pytest

from oracle import filters as ref

pytestmark = pytest.mark.gpu

GUARD = 256
DTYPES = [np.float64, np.float32]
U32 = 2.0 ** -24  # float32 unit roundoff


def _quiet(fn, *a, **k):
    """numpy's own warnings on NaN / inf / constant inputs (0/0, inf - inf) are expected."""
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **k)


class Capi:
    """specenh_filter / _quantfilt / _gaussblr / _morph on a flat device buffer holding
    `batch` images `stride` elements apart."""

    def __init__(self, dev):
        import torch

        from specenh import _lib

        self.torch, self._lib, self.L, self.dev = torch, _lib, _lib.lib(), dev
        self.ops = {"norm": _lib.FILTER_NORM, "rescale": _lib.FILTER_RESCALE,
                    "meansub": _lib.FILTER_MEANSUB}
        self.codes = {torch.float32: 0, torch.float64: 3}

    def workspace(self, nbytes):
        t = self.torch
        buf = t.empty(nbytes + GUARD, dtype=t.uint8, device=self.dev)
        buf[:nbytes] = 0xFF
        buf[nbytes:] = 0xA5
        return buf

    def run(self, kind, flat, batch, rows, cols, stride=None, arg=None, sentinel=float("nan")):
        t, L = self.torch, self.L
        stride = rows * cols if stride is None else stride
        assert flat.dim() == 1 and flat.numel() == batch * stride and flat.is_contiguous()
        out = t.full_like(flat, sentinel)
        vp = lambda x: ctypes.c_void_p(x.data_ptr())
        st = ctypes.c_void_p(t.cuda.current_stream(self.dev).cuda_stream)
        dt = self.codes[flat.dtype]
        ws, nws = None, 0
        if kind in self.ops:
            nws = int(L.specenh_filter_workspace_bytes(batch, rows))
            ws = self.workspace(nws)
            rc = L.specenh_filter(self.ops[kind], dt, vp(flat), batch, rows, cols, stride, vp(out),
                                  vp(ws), st)
        elif kind == "quantfilt":
            rc = L.specenh_quantfilt(dt, vp(flat), batch, rows, cols, stride, float(arg), vp(out),
                                     st)
        else:
            nws = int(L.specenh_u8filter_workspace_bytes(batch, rows, cols))
            ws = self.workspace(nws)
            if kind == "gaussblr":
                kw, kh, sigma = arg
                rc = L.specenh_gaussblr(dt, vp(flat), batch, rows, cols, stride, int(kw), int(kh),
                                        float(sigma), vp(out), vp(ws), st)
            else:
                assert kind == "morph"
                rc = L.specenh_morph(dt, vp(flat), batch, rows, cols, stride, vp(out), vp(ws), st)
        self._lib.check(rc, kind)
        t.cuda.synchronize(self.dev)
        if ws is not None:
            assert bool((ws[nws:] == 0xA5).all()), f"{kind}: wrote past its {nws}-byte workspace"
        return out

    def images(self, kind, S, arg=None):
        """numpy [B, rows, cols] in -> numpy out, contiguous call."""
        B, rows, cols = S.shape
        flat = self.torch.as_tensor(np.ascontiguousarray(S).reshape(-1), device=self.dev)
        return self.run(kind, flat, B, rows, cols, arg=arg).cpu().numpy().reshape(S.shape)


@pytest.fixture(scope="module")
def capi(gpu_device):
    return Capi(gpu_device)


def _shot_errors(got, exp, exact):
    """Per-shot error of [B, rows, cols] arrays: exact -> number of elements whose bits differ
    (NaN == NaN); otherwise max |got - exp| in fp64, inf where only one side is NaN."""
    if exact:
        same = (got == exp) | (np.isnan(got) & np.isnan(exp))
        return (~same).sum(axis=(1, 2)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    d[(got == exp) | (np.isnan(got) & np.isnan(exp))] = 0.0  # equal infinities too
    d[np.isnan(d)] = np.inf  # NaN on one side only, or infinities of opposite sign
    return d.max(axis=(1, 2))


def _assert_shots(what, got, exp, tol, named):
    """Every spectrogram within tol (0: bit-exact; a scalar or one bound per shot)."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.dtype, exp.dtype)
    err = _shot_errors(got, exp, exact=np.all(np.asarray(tol) == 0))
    bad = np.flatnonzero(err > tol)
    print(f"[{what}] max shot error {err.max():.3e}, bound {np.max(tol):.3e}")
    assert bad.size == 0, (
        f"{what}: {bad.size} of {len(err)} shots wrong, first {bad[:6].tolist()}, "
        f"last {bad[-1]}; errors at the named shots "
        + ", ".join(f"{b}: {err[b]:.3e}" for b in named))


# ---------------------------------------------------------------- large batches
def _batch_refs(S, kind, arg=None):
    """numpy, vectorised over the batch, in S's dtype."""
    if kind == "meansub":
        d = np.abs(S - S.mean(2, keepdims=True))
        mn, mx = d.min((1, 2), keepdims=True), d.max((1, 2), keepdims=True)
        return (d - mn) / (mx - mn)
    if kind == "norm":
        return (S - S.mean((1, 2), keepdims=True)) / S.std((1, 2), keepdims=True)
    if kind == "rescale":
        mn, mx = S.min((1, 2), keepdims=True), S.max((1, 2), keepdims=True)
        return (S - mn) / (mx - mn)
    return np.where(S < np.quantile(S, arg, axis=1, keepdims=True), 0, S)


def _f32_norm_bound(S):
    """float32 norm, y = (x - m) / s over n elements of [0, 1]. numpy's float32 sum of n terms
    carries at most c roundings on any path: c = n for a short sum in any order, and for its
    pairwise sum 18 inside a 128-element block (8 accumulators of 16 terms, 3 levels to join
    them) plus one per level of the tree above the blocks. Its mean is then off by at most
    c u (u = 2^-24) and its std by at most 2 c u relative; the kernel takes both from fp64
    sums and rounds three times (4 u |y|). So per shot
    |dy| <= ((c + 1) / s + (2 c + 6) max|y|) u: about 1e-5 for the shapes used here
    (15 elements: c = 15; 37 x 29: c = 23), asserted to stay under 2e-5."""
    n = S.shape[1] * S.shape[2]
    c = min(n, 19 + int(np.ceil(np.log2(max(1.0, n / 128)))))
    S64 = S.astype(np.float64)
    s = S64.std((1, 2))
    ymax = np.abs((S64 - S64.mean((1, 2), keepdims=True)) / s[:, None, None]).max((1, 2))
    bound = ((c + 1) / s + (2 * c + 6) * ymax) * U32
    assert bound.max() <= 2e-5, bound.max()
    return bound


@pytest.mark.parametrize("dtype", DTYPES)
def test_many_small_spectrograms(capi, dtype):
    """[90000, 3, 5]: 270,000 rows (the row-mean grid is capped at 65,536 workgroups of 4
    rows) and 90,000 shots (quantfilt is launched in slices of 65,535). Every image holds a
    0 and a 1 so that its std and the range of |x - row mean| are at least 0.18 and ~0.5:
    the absolute float32 tolerances then hold whatever the other 13 values are."""
    import torch

    B, rows, cols = 90000, 3, 5
    S = np.random.default_rng(20).random((B, rows, cols)).astype(dtype)
    S[:, 0, 0], S[:, 0, 1] = 0, 1
    # 87381 holds row 262,144 itself, 87382 is the first shot wholly past it
    named = [65534, 65535, 65536, 262144 // rows, -(-262144 // rows)]
    f32 = dtype == np.float32
    t = torch.as_tensor(S, device=capi.dev)
    flat = t.reshape(-1)
    tols = {"meansub": 1e-6 if f32 else 1e-12, "rescale": 2e-7 if f32 else 0.0}
    for kind in ("meansub", "norm", "rescale"):
        exp = _batch_refs(S, kind)
        tol = tols.get(kind)
        if kind == "norm":
            tol = _f32_norm_bound(S) if f32 else 1e-12 * np.ptp(exp, axis=(1, 2))
        out = capi.run(kind, flat, B, rows, cols)
        _assert_shots(f"{kind} {S.dtype}", out.cpu().numpy().reshape(S.shape), exp, tol, named)
        op = torch.ops.specenh.label_filter(t, capi.ops[kind])
        assert torch.equal(op.reshape(-1), out), f"{kind}: the torch op differs from the C call"
    for thr in (0.9, 0.37):
        got = capi.run("quantfilt", flat, B, rows, cols, arg=thr).cpu().numpy().reshape(S.shape)
        _assert_shots(f"quantfilt {thr} {S.dtype}", got, _batch_refs(S, "quantfilt", thr), 0.0,
                      named)


@pytest.mark.parametrize("dtype", DTYPES)
def test_few_shots_many_rows_meansub(capi, dtype):
    """[2051, 128, 4]: 262,528 rows in 128-row images; shot 2048 is the first past row 262,144."""
    import torch

    B, rows, cols = 2051, 128, 4
    S = np.random.default_rng(21).random((B, rows, cols)).astype(dtype)
    t = torch.as_tensor(S, device=capi.dev)
    out = capi.run("meansub", t.reshape(-1), B, rows, cols)
    tol = 1e-6 if dtype == np.float32 else 1e-12
    _assert_shots(f"meansub {S.dtype}", out.cpu().numpy().reshape(S.shape),
                  _batch_refs(S, "meansub"), tol, [0, 2047, 2048, 2050])
    op = torch.ops.specenh.label_filter(t, capi.ops["meansub"])
    assert torch.equal(op.reshape(-1), out), "the torch op differs from the C call"


# ---------------------------------------------------------------- more than 2^24 elements
def _below(a):
    return np.nextafter(a, np.float32(-np.inf))


def _label_chain_oracle(x):
    """The float32 label chain of one image in numpy, stage by stage, and the interval in which
    its last three stages can land when the first meansub is only known to 1e-6.

    quantfilt and gaussblr are exact, so q and g (float32) are what the library must return,
    and m1 = meansub(g) in float32 is what its first meansub must match within 1e-6. morph
    requantises m1 to uint8; where 255 m1 sits within 255e-6 of an integer the level may be
    the one below or above. Every later step is monotone in its inputs, so two level images
    (from m1 - 1e-6 and m1 + 1e-6, rounded outwards, through the same float32 expression)
    bracket the library's levels, max / min filters keep the bracket, and
    v = (w - mn) / (mx - mn) rises with w and falls with mn and mx. The last meansub gets
    intervals for the row means, for d = |v - mean| and for min d and max d in the same way.
    Away from the ambiguous pixels the two ends coincide or lie about 1e-5 apart."""
    q = ref.quantfilt(x, 0.9)
    g = ref.gaussblr(q, (31, 3)).astype(np.float32)
    m1 = ref.meansub(g)
    assert q.dtype == g.dtype == m1.dtype == np.float32
    tol = np.float32(1e-6)
    lo, hi = np.clip(_below(m1 - tol), 0, 1), np.clip(-_below(-(m1 + tol)), 0, 1)
    # A rescaled image holds an exact 1 at its maximum: one of the pixels that can reach 1 is
    # 1 in the library too. One bracket per such pixel, then their union.
    top = np.argwhere(hi >= 1)
    assert 1 <= len(top) <= 8, len(top)
    parts = []
    for r, c in top:
        lo_k = lo.copy()
        lo_k[r, c] = 1
        parts.append(_chain_tail(lo_k, hi))
    v_lo, v_hi, o_lo, o_hi = (f([p[i] for p in parts], axis=0)
                              for i, f in enumerate((np.min, np.max, np.min, np.max)))
    return {"q": q, "g": g, "m1": m1, "v": (v_lo, v_hi), "out": (o_lo, o_hi)}


def _chain_tail(m_lo, m_hi):
    """morph then meansub on a bracket [m_lo, m_hi] of the first meansub's float32 output."""
    # (rescale(m) * 255).astype(uint8) with min m = 0 and max m = 1, as both sides have it
    w_lo, w_hi = (ref.morph_u8((m * np.float32(255)).astype(np.uint8)).astype(np.float64)
                  for m in (m_lo, m_hi))
    assert (w_lo <= w_hi).all()
    mn_lo, mn_hi, mx_lo, mx_hi = w_lo.min(), w_hi.min(), w_lo.max(), w_hi.max()
    assert mx_lo - mn_hi > 8, (mn_lo, mn_hi, mx_lo, mx_hi)
    v_lo = np.clip((w_lo - mn_hi) / (mx_hi - mn_hi), 0, 1).astype(np.float32)
    v_hi = np.clip((w_hi - mn_lo) / (mx_lo - mn_lo), 0, 1).astype(np.float32)
    a, b = v_lo.astype(np.float64), v_hi.astype(np.float64)
    e_lo = a - b.mean(axis=1)[:, None]
    e_hi = b - a.mean(axis=1)[:, None]
    d_hi = np.maximum(np.abs(e_lo), np.abs(e_hi))
    d_lo = np.where((e_lo <= 0) & (e_hi >= 0), 0.0, np.minimum(np.abs(e_lo), np.abs(e_hi)))
    o_lo = np.clip((d_lo - d_hi.min()) / (d_hi.max() - d_hi.min()), 0, 1)
    o_hi = np.clip((d_hi - d_lo.min()) / (d_lo.max() - d_lo.min()), 0, 1)
    return v_lo, v_hi, o_lo, o_hi


def _assert_inside(what, got, lo, hi, slack):
    """lo - slack <= got <= hi + slack everywhere; the bracket must be narrow to mean much."""
    width = hi.astype(np.float64) - lo
    out = np.maximum(lo - got.astype(np.float64), got.astype(np.float64) - hi)
    out[np.isnan(out)] = np.inf
    print(f"[{what}] worst excursion {out.max():.3e} (allowed {slack:.1e}); bracket width: "
          f"median {np.median(width):.2e}, 99.9% {np.quantile(width, 0.999):.2e}, "
          f"max {width.max():.2e}, equal ends {np.mean(width == 0):.4f}")
    assert (width >= 0).all() and np.quantile(width, 0.999) <= 1e-3, what
    assert np.mean(width == 0) >= 0.9, what
    bad = np.argwhere(out > slack)
    assert len(bad) == 0, f"{what}: {len(bad)} pixels outside, first {bad[:5].tolist()}"


def test_more_than_2_pow_24_elements(capi):
    """[226, 250, 300] float32, 16.95 M elements: the element-wise kernels' grid (capped at
    65,536 workgroups of 256) wraps inside image 223, which straddles element 2^24."""
    import torch

    from specenh import filters

    B, rows, cols = 226, 250, 300
    assert 223 * rows * cols < 2 ** 24 < 224 * rows * cols < B * rows * cols
    S = np.random.default_rng(22).random((B, rows, cols), dtype=np.float32) ** 2
    t = torch.as_tensor(S, device=capi.dev)
    flat = t.reshape(-1)
    check = [0, 223, 224, 225]
    cases = [("rescale", None, ref.rescale, 2e-7), ("meansub", None, ref.meansub, 1e-6),
             ("gaussblr", (31, 3, 0.0), lambda x: ref.gaussblr(x).astype(np.float32), 0.0),
             ("morph", None, lambda x: ref.morph(x).astype(np.float32), 0.0)]
    for kind, arg, oracle, tol in cases:
        out = capi.run(kind, flat, B, rows, cols, arg=arg).reshape(B, rows, cols)
        nan = torch.isnan(out).any(2).any(1).cpu().numpy()
        assert not nan.any(), f"{kind}: NaN in images {np.flatnonzero(nan)[:8].tolist()}"
        got = out[check].cpu().numpy()
        exp = np.stack([oracle(S[b]) for b in check])
        _assert_shots(f"{kind} >2^24", got, exp, tol, [0, 1, 2, 3])
        del out
    # the composed chain, stage by stage on the whole batch, then label_pipeline itself
    stages = {}
    stages["q"] = filters.quantfilt(t, 0.9)
    stages["g"] = filters.gaussblr(stages["q"], (31, 3))
    stages["m1"] = filters.meansub(stages["g"])
    stages["v"] = filters.morph(stages["m1"])
    stages["out"] = filters.meansub(stages["v"])
    out = filters.label_pipeline(t)
    assert out.shape == t.shape and out.dtype == torch.float32
    assert torch.equal(out, stages["out"]), "label_pipeline is not the chain of its stages"
    nan = torch.isnan(out).any(2).any(1).cpu().numpy()
    assert not nan.any(), f"label_pipeline: NaN in images {np.flatnonzero(nan)[:8].tolist()}"
    got = {k: v[check].cpu().numpy() for k, v in stages.items()}
    for i, b in enumerate(check):
        o = _label_chain_oracle(S[b])
        np.testing.assert_array_equal(got["q"][i], o["q"], err_msg=f"quantfilt, image {b}")
        np.testing.assert_array_equal(got["g"][i], o["g"], err_msg=f"gaussblr, image {b}")
        _assert_shots(f"chain meansub, image {b}", got["m1"][i][None], o["m1"][None], 1e-6, [0])
        _assert_inside(f"chain morph, image {b}", got["v"][i], *o["v"], 0.0)
        _assert_inside(f"label_pipeline, image {b}", got["out"][i], *o["out"], 1e-6)


# ---------------------------------------------------------------- strided batches
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_batch_through_c_abi(capi, dtype):
    """stride = rows * cols + 7: the gaps of S hold a huge value (read one and the statistics
    go wrong), the gaps of out must keep their sentinel, and the images must carry the bits of
    the contiguous call and match numpy."""
    import torch

    B, rows, cols = 3, 37, 29
    n, stride = rows * cols, rows * cols + 7
    S = (np.random.default_rng(23).random((B, rows, cols)) ** 2).astype(dtype)
    padded = np.full((B, stride), 1e30, dtype=dtype)
    padded[:, :n] = S.reshape(B, n)
    flat = torch.as_tensor(padded.reshape(-1), device=capi.dev)
    f32 = dtype == np.float32
    as_t = (lambda a: a.astype(np.float32)) if f32 else (lambda a: a)
    cases = [("norm", None, ref.norm, None),
             ("rescale", None, ref.rescale, 2e-7 if f32 else 0.0),
             ("meansub", None, ref.meansub, 1e-6 if f32 else 1e-12),
             ("quantfilt", 0.9, lambda x: ref.quantfilt(x, 0.9), 0.0),
             ("quantfilt", 0.37, lambda x: ref.quantfilt(x, 0.37), 0.0),
             ("gaussblr", (31, 3, 0.0), lambda x: as_t(ref.gaussblr(x)), 0.0),
             ("gaussblr", (5, 9, 1.5), lambda x: as_t(ref.gaussblr(x, (5, 9), 1.5)), 0.0),
             ("morph", None, lambda x: as_t(ref.morph(x)), 0.0)]
    for kind, arg, oracle, tol in cases:
        out = capi.run(kind, flat, B, rows, cols, stride=stride, arg=arg, sentinel=-7.0)
        out = out.cpu().numpy().reshape(B, stride)
        assert (out[:, n:] == -7.0).all(), f"{kind}: wrote into the gap between two images"
        got = out[:, :n].reshape(S.shape)
        np.testing.assert_array_equal(got, capi.images(kind, S, arg), err_msg=kind)
        exp = np.stack([oracle(S[b]) for b in range(B)])
        if tol is None:  # norm
            tol = _f32_norm_bound(S) if f32 else 1e-12 * np.ptp(exp, axis=(1, 2))
        _assert_shots(f"{kind} strided {S.dtype}", got, exp, tol, [0, 1, 2])


# ---------------------------------------------------------------- quantfilt edges
QF_THR = (0.0, 1.0, 0.5, 0.9, 0.37)


def _qf_images(rng, rows, cols, dtype):
    """random; columns of all-equal values; columns holding +inf, -inf or both."""
    a = rng.random((3, rows, cols)).astype(dtype)
    a[1, :, ::2] = a[1, 0, ::2]
    a[1, :, 0] = 0.0
    r = rng.integers(0, rows, 3 * cols)
    for c in range(cols):
        a[2, r[3 * c], c] = (np.inf, -np.inf, np.inf)[c % 3]
        if c % 3 == 2:
            a[2, r[3 * c + 1], c] = -np.inf
        if c % 5 == 4:
            a[2, :, c] = np.inf
    return a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 2, 3, 11, 21, 255, 256, 257])
def test_quantfilt_tiles_and_ranks(capi, rows, dtype):
    """rows around the 256-thread block, cols around the 16-column tile, thr at both ends,
    between two ranks, and on an integer virtual index: exactly (rows 11, thr 0.5:
    (n - 1) q = 5) and after rounding (rows 21, thr 0.9: 20 q rounds to 18.0 in fp64, where
    n q + (1 - q) - 1 gives 18.000000000000004 and a weight that lifts the quantile one ulp
    above the 18th order statistic, which is then zeroed)."""
    rng = np.random.default_rng(100 + rows)
    for cols in (1, 15, 16, 17, 33):
        S = _qf_images(rng, rows, cols, dtype)
        for thr in QF_THR:
            got = capi.images("quantfilt", S, thr)
            exp = np.stack([_quiet(ref.quantfilt, S[b], thr) for b in range(len(S))])
            assert got.dtype == exp.dtype == S.dtype
            np.testing.assert_array_equal(got, exp, err_msg=f"rows {rows} cols {cols} thr {thr}")


@pytest.mark.parametrize("dtype,top", [(np.float64, 1276), (np.float32, 2552)])
def test_quantfilt_largest_height(capi, dtype, top):
    """16 columns of `top` rows fill the 160 KiB - 512 of LDS the kernel may ask for; one row
    more is refused with that dtype's limit in the message."""
    import torch

    S = np.random.default_rng(top).random((2, top, 17)).astype(dtype)
    S[1] = np.round(S[1] * 64) / 64  # many ties
    for thr in (0.9, 0.37):
        got = capi.images("quantfilt", S, thr)
        exp = np.stack([ref.quantfilt(S[b], thr) for b in range(2)])
        np.testing.assert_array_equal(got, exp, err_msg=f"thr {thr}")
    over = np.zeros((1, top + 1, 17), dtype)
    name = np.dtype(dtype).name
    with pytest.raises(NotImplementedError, match=rf"rows <= {top} for {name}"):
        torch.ops.specenh.quantfilt(torch.as_tensor(over, device=capi.dev), 0.9)
    with pytest.raises(NotImplementedError, match=rf"rows <= {top} for {name}"):
        capi.images("quantfilt", over, 0.9)


@pytest.mark.parametrize("dtype", DTYPES)
def test_quantfilt_nan_columns(capi, dtype):
    """A column that holds a NaN has the quantile NaN: it passes through unchanged while its
    neighbours are filtered; an all-NaN image comes back all NaN. Run twice with another
    launch in between, so the answer cannot lean on what an earlier launch left in LDS."""
    rng = np.random.default_rng(24)
    rows, cols = 37, 40
    S = rng.random((4, rows, cols)).astype(dtype)
    for c in range(0, cols, 3):  # image 0: one NaN in every third column, any row
        S[0, rng.integers(0, rows), c] = np.nan
    S[1] = np.nan
    S[2, 0, :] = np.nan  # the NaN first in every column
    S[2, -1, ::2] = np.nan  # ... and last
    other = (rng.random((4, rows, cols)) * 1e6 - 5e5).astype(dtype)
    for thr in (0.9, 0.37, 0.0, 1.0):
        exp = np.stack([_quiet(ref.quantfilt, S[b], thr) for b in range(4)])
        assert np.isnan(exp[1]).all() and not np.isnan(exp[3]).any()
        assert np.array_equal(exp[0][:, ::3], S[0][:, ::3], equal_nan=True)
        for attempt in (1, 2):
            got = capi.images("quantfilt", S, thr)
            wrong = int(_shot_errors(got, exp, exact=True).sum())
            assert np.array_equal(got, exp, equal_nan=True), (
                f"thr {thr} attempt {attempt}: {wrong} elements differ")
            capi.images("quantfilt", other, 1.0 - thr)


def _adjacent_stats(rng, rows, cols, thr):
    """float32 columns whose two order statistics around the virtual index (n - 1) thr are one
    ulp apart, rows permuted; returns the image and the float32 weight gamma."""
    vi = np.float32(rows - 1) * np.float32(thr)
    lo = int(np.floor(vi))
    s = np.sort(rng.random((rows, cols)).astype(np.float32) + np.float32(0.5), axis=0)
    s[lo + 1] = np.nextafter(s[lo], np.float32(np.inf))
    assert (s[lo + 1] <= s[lo + 2]).all()
    return rng.permuted(s, axis=0), float(vi - np.floor(vi))


def _fp64_lerp_quantfilt(S, thr):
    """What a kernel that lerps and compares in fp64 returns for a float32 image."""
    rows = S.shape[0]
    vi = rows * thr + (1.0 + thr * (1.0 - 1.0 - 1.0)) - 1.0
    lo = int(np.floor(vi))
    g = vi - lo
    s = np.sort(S.astype(np.float64), axis=0)
    a, b = s[lo], s[lo + 1]
    q = b - (b - a) * (1.0 - g) if g >= 0.5 else a + (b - a) * g
    return np.where(S.astype(np.float64) < q, 0, S).astype(np.float32)


@pytest.mark.parametrize("rows", [23, 128])
def test_quantfilt_float32_adjacent_order_statistics(capi, rows):
    """numpy lerps and compares a float32 array in float32: with the two statistics one ulp
    apart and gamma < 0.5 the quantile rounds to the lower one, which is then kept; an fp64
    lerp lands strictly between the two and zeroes it. The construction is checked on the CPU
    first: numpy and the fp64 emulation differ in every column exactly when gamma < 0.5."""
    rng = np.random.default_rng(rows)
    cols = 33
    imgs, exps = [], []
    for thr in (0.37, 0.61, 0.9, 0.12):
        S, gamma = _adjacent_stats(rng, rows, cols, thr)
        exp = ref.quantfilt(S, thr)
        assert exp.dtype == np.float32
        differs = (exp != _fp64_lerp_quantfilt(S, thr)).any(axis=0)
        assert differs.all() if gamma < 0.5 else not differs.any(), (thr, gamma, differs)
        imgs.append((thr, S))
        exps.append(exp)
    for (thr, S), exp in zip(imgs, exps):
        got = capi.images("quantfilt", S[None], thr)[0]
        bad = np.flatnonzero((got != exp).any(axis=0))
        assert bad.size == 0, f"rows {rows} thr {thr}: columns {bad.tolist()} differ from numpy"


# ---------------------------------------------------------------- blur sizes, tiny images
KSIZES = [(1, 1), (1, 31), (31, 1), (3, 31), (7, 7), (9, 9), (127, 127), (127, 1), (1, 127)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(40, 50), (129, 97), (5, 3), (2, 2), (1, 40)])
def test_gaussblr_sizes(capi, shape, dtype):
    """kw != kh in both orders, size 1 and the largest size, on images larger and smaller than
    the kernel (the reflect loop then runs more than once)."""
    s = (np.random.default_rng(sum(shape)).random((2,) + shape) ** 3).astype(dtype)
    for kw, kh in KSIZES:
        got = capi.images("gaussblr", s, (kw, kh, 0.0))
        exp = np.stack([_quiet(ref.gaussblr, s[b], (kw, kh)) for b in range(2)]).astype(dtype)
        np.testing.assert_array_equal(got, exp, err_msg=f"ksize {(kw, kh)}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_gaussblr_sigma_and_bad_sizes(capi, dtype):
    import torch

    s = (np.random.default_rng(25).random((2, 40, 50)) ** 3).astype(dtype)
    t = torch.as_tensor(s, device=capi.dev)
    for sigma in (0.3, 1.0, 7.5):
        for kw, kh in ((7, 7), (31, 3), (1, 31), (127, 9)):
            got = torch.ops.specenh.gaussblr(t, kw, kh, sigma).cpu().numpy()
            exp = np.stack([ref.gaussblr(s[b], (kw, kh), sigma) for b in range(2)]).astype(dtype)
            np.testing.assert_array_equal(got, exp, err_msg=f"sigma {sigma} ksize {(kw, kh)}")
    for kw, kh in ((4, 3), (3, 4), (2, 2), (129, 3), (3, 129), (0, 3), (3, 0), (0, 0)):
        with pytest.raises(ValueError, match="odd, positive and <= 127"):
            torch.ops.specenh.gaussblr(t, kw, kh, 0.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_morph_tiny_images(capi, dtype):
    """Images no larger than the 4 x 4 closing rect; 1 x 1 is 0 / 0 = NaN, as in numpy."""
    rng = np.random.default_rng(26)
    for shape in ((2, 2), (1, 1), (4, 4), (3, 5)):
        s = (rng.random((3,) + shape) ** 2).astype(dtype)
        got = capi.images("morph", s)
        exp = np.stack([_quiet(ref.morph, s[b]) for b in range(3)]).astype(dtype)
        np.testing.assert_array_equal(got, exp, err_msg=str(shape))
        if shape == (1, 1):
            assert np.isnan(got).all()
