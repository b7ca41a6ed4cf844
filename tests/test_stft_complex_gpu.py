"""Complex STFT / inverse STFT on the GPU (csrc/stft_complex.hip) against scipy.signal.stft /
istft called in fp64 on the fp32 samples widened.

Bounds: 1e-5 normwise (max|got - ref| / max|ref| per spectrogram or signal), the project's
contract for fp32 spectra, and the same 1e-5 per frame pair and per output
sample on shots whose level changes by four decades. Every output buffer is NaN-filled before the
launch, so an element the kernel does not write fails the comparison. Each test prints its
measured maximum (pytest -s); DESIGN.md records them.
"""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

import stft_local as sl

pytestmark = pytest.mark.gpu

FS = 5e5
TOL = 1e-5
# (L, nperseg, noverlap, window)
BASE = [
    (16512, 256, 128, "hann"),    # config 1; T = 130, inverse length 16512
    (4000, 64, 48, "hamm"),       # smallest nperseg, 4x overlap, T = 251
    (5000, 256, 100, "hann"),     # hop 156 does not divide nperseg; padding adds samples
    (9000, 1024, 768, "hamm"),    # the C2 parameters; T = 37
    (20000, 4096, 2048, "hann"),  # largest nperseg; T = 11
    (333, 64, 32, "hann"),        # T = 12: shorter than one tile, tail mostly zero-extension
    (300, 64, 63, "hamm"),        # hop 1: 64 frames under every sample
    (640, 64, 0, "hamm"),         # hop = nperseg: no overlap at all
    # odd log2(nperseg): the radix-2 pass, then radix-4 from Ns = 2, forward and inverse
    (9000, 128, 96, "hann"),      # T = 283 (odd): 17 tiles of 16 + 11; inverse in 3 spans
    (12300, 512, 200, "hamm"),    # T = 41 (odd): 5 tiles of 8 + 1; hop 312; 4 spans
    (20000, 2048, 1536, "hann"),  # T = 41 (odd): 10 tiles of 4 + 1; 5 spans
    (9010, 64, 48, "hamm"),       # T = 565 (odd): nperseg 64 across span edges, 3 spans
]
ODD = BASE[8:11]  # nperseg 128, 512, 2048
# (case, boundary, padded, detrend, scaling)
CONFIGS = [(c, "zeros", True, False, "spectrum") for c in BASE]
CONFIGS += [(c, None, True, False, "spectrum") for c in BASE[:3]]
CONFIGS += [(c, "zeros", False, False, "spectrum") for c in BASE[:3]]
CONFIGS += [(BASE[1], "zeros", True, "constant", "spectrum"),
            (BASE[1], "zeros", True, "linear", "spectrum"),
            (BASE[0], "zeros", True, False, "psd")]
CONFIGS += [(c, None, True, False, "spectrum") for c in ODD[:2]]     # T = 279, 39
CONFIGS += [(c, "zeros", False, False, "spectrum") for c in ODD[:2]]  # T = 282, 40: even
CONFIGS += [(ODD[2], "zeros", True, "linear", "spectrum"),
            (ODD[2], "zeros", True, False, "psd")]


def _id(cfg):
    (L, n, nov, w), boundary, padded, detrend, scaling = cfg
    return f"{L}-{n}-{nov}-{w}-{boundary}-{'pad' if padded else 'nopad'}-{detrend}-{scaling}"


IDS = [_id(c) for c in CONFIGS]
BASE_IDS = [f"{L}-{n}-{nov}-{w}" for L, n, nov, w in BASE]


@functools.lru_cache(maxsize=None)
def signal(L, batch=3):
    from specenh.synthetic import plasma_chirps

    x = np.ascontiguousarray(plasma_chirps(batch, L, seed0=7), dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(cfg):
    """scipy fp64 on the widened fp32 samples: Z_ref, its complex64 rounding, and the fp64
    inverse of that rounded Z (boundary trimmed exactly when the forward extended)."""
    (L, n, nov, w), boundary, padded, detrend, scaling = cfg
    x = signal(L).astype(np.float64)
    f, t, Z = scipy.signal.stft(x, fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend,
                                boundary=boundary, padded=padded, scaling=scaling)
    Z32 = np.ascontiguousarray(Z, dtype=np.complex64)  # scipy returns a transposed view
    Z32.setflags(write=False)
    ti, xi = scipy.signal.istft(Z32.astype(np.complex128), fs=FS, window=w, nperseg=n,
                                noverlap=nov, boundary=boundary is not None, scaling=scaling)
    return f, t, Z, Z32, ti, xi


SCALING = {"spectrum": 1, "psd": 0}  # SPECENH_SCALING_SPECTRUM / SPECENH_SCALING_DENSITY


def to_dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)  # a writable copy of the cached array


def nan_c64(shape, dev):
    return torch.full(shape, complex(float("nan"), float("nan")), dtype=torch.complex64,
                      device=dev)


def forward(x, cfg):
    """torch.ops.specenh.stft_complex_out into a NaN-filled buffer."""
    from specenh import _lib, ops, stft

    (L, n, nov, w), boundary, padded, detrend, scaling = cfg
    T = stft.complex_frame_count(x.shape[1], n, nov, boundary, padded)
    out = nan_c64((x.shape[0], n // 2 + 1, T), x.device)
    torch.ops.specenh.stft_complex_out(
        x, n, nov, ops.window_key(w, n), FS, SCALING[scaling], _lib.DETREND[detrend],
        0 if boundary is None else 1, padded, out)
    return out


def inverse(Z, cfg, gain=None):
    """torch.ops.specenh.istft_out into a NaN-filled buffer."""
    from specenh import _lib, ops, stft

    (L, n, nov, w), boundary, padded, detrend, scaling = cfg
    nout = stft.istft_length(Z.shape[2], n, nov, boundary is not None)
    out = torch.full((Z.shape[0], nout), float("nan"), dtype=torch.float32, device=Z.device)
    torch.ops.specenh.istft_out(Z, gain, n, nov, ops.window_key(w, n), FS, SCALING[scaling],
                                boundary is not None, out)
    return out


def normwise(got, ref):
    """max over the batch of max|got - ref| / max|ref| (NaN if anything is NaN)."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    ax = tuple(range(1, ref.ndim))
    return float(np.max(np.abs(got - ref).max(axis=ax) / np.abs(ref).max(axis=ax)))


def check(name, got, ref):
    err = normwise(got, ref)
    print(f"[stft_complex] {name}: normwise err {err:.3e}")
    assert err <= TOL, f"{name}: {err:.3e} > {TOL}"  # also fails on NaN


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_forward_matches_scipy(gpu_device, cfg):
    f, t, Z, Z32, ti, xi = reference(cfg)
    x = to_dev(signal(cfg[0][0]), gpu_device)
    got = forward(x, cfg)
    assert got.dtype == torch.complex64 and tuple(got.shape) == Z.shape
    assert got.shape[0] == 3 and got.shape[1] == cfg[0][1] // 2 + 1
    check("forward " + _id(cfg), got.cpu().numpy().astype(np.complex128), Z)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_inverse_matches_scipy(gpu_device, cfg):
    f, t, Z, Z32, ti, xi = reference(cfg)
    got = inverse(to_dev(Z32, gpu_device), cfg)
    assert got.dtype == torch.float32 and got.shape[1] == xi.shape[-1]
    check("inverse " + _id(cfg), got.cpu().numpy().astype(np.float64), xi)


# Localised error. normwise() divides by the loudest value of a whole shot, so on a shot whose
# level changes it lets any error through at the quiet end. The shots of tests/stft_local.py
# fall (or, reversed, rise) by four decades, and the error is measured where the algorithm
# bounds it: per frame against the louder frame of its pair (2q, 2q + 1), per output sample
# against the loudest sample within nperseg + hop. tests/test_stft_complex_local_cpu.py shows a
# plain emulation of the algorithm below 3e-7 under both metrics on the same inputs.
@pytest.mark.parametrize("reverse", [False, True], ids=["falling", "rising"])
@pytest.mark.parametrize("case", sl.LOCAL, ids=sl.LOCAL_IDS)
def test_forward_error_per_frame_pair(gpu_device, case, reverse):
    Z, Z32, xi = sl.reference(case, reverse)
    cfg = (case, "zeros", True, False, "spectrum")
    got = forward(to_dev(sl.shots(case, reverse), gpu_device), cfg)
    assert got.dtype == torch.complex64 and tuple(got.shape) == Z.shape
    e = sl.frame_error(got.cpu().numpy(), Z)
    b, t = np.unravel_index(np.nanargmax(e) if not np.isnan(e).all() else 0, e.shape)
    print(f"[stft_complex] forward per pair {_id(cfg)} {'rising' if reverse else 'falling'}: "
          f"max err {e.max():.3e} (shot {b}, frame {t} of {e.shape[1]}); normwise "
          f"{normwise(got.cpu().numpy().astype(np.complex128), Z):.3e}")
    assert not np.isnan(e).any() and e.max() <= TOL, f"{e.max():.3e} > {TOL} at frame {t}"


@pytest.mark.parametrize("reverse", [False, True], ids=["falling", "rising"])
@pytest.mark.parametrize("case", sl.LOCAL, ids=sl.LOCAL_IDS)
def test_inverse_error_per_sample(gpu_device, case, reverse):
    Z, Z32, xi = sl.reference(case, reverse)
    cfg = (case, "zeros", True, False, "spectrum")
    got = inverse(to_dev(Z32, gpu_device), cfg)
    assert got.dtype == torch.float32 and tuple(got.shape) == xi.shape
    e = sl.sample_error(got.cpu().numpy(), xi, case)
    b, n = np.unravel_index(np.nanargmax(e) if not np.isnan(e).all() else 0, e.shape)
    print(f"[stft_complex] inverse per sample {_id(cfg)} {'rising' if reverse else 'falling'}: "
          f"max err {e.max():.3e} (shot {b}, sample {n} of {e.shape[1]}); normwise "
          f"{normwise(got.cpu().numpy().astype(np.float64), xi):.3e}")
    assert not np.isnan(e).any() and e.max() <= TOL, f"{e.max():.3e} > {TOL} at sample {n}"


# Round trip: the boundary='zeros' configurations. The two detrended ones are left out: a
# per-frame detrend removes what no inverse can put back, so istft(stft(x)) != x there by
# construction (scipy's own round trip differs from x by the trend as well).
ROUND = [c for c in CONFIGS if c[1] == "zeros" and not c[3]]


@pytest.mark.parametrize("cfg", ROUND, ids=[_id(c) for c in ROUND])
def test_round_trip_on_the_gpu(gpu_device, cfg):
    from specenh import stft

    (L, n, nov, w), boundary, padded, detrend, scaling = cfg
    x = to_dev(signal(L), gpu_device)
    f, t, Z = stft.stft(x, fs=FS, window=w, nperseg=n, noverlap=nov, boundary=boundary,
                        padded=padded, scaling=scaling)
    ti, y = stft.istft(Z, fs=FS, window=w, nperseg=n, noverlap=nov, boundary=True,
                       scaling=scaling)
    assert ti.shape[0] == y.shape[1]
    # padded=True covers the whole signal; without padding scipy drops the last partial hop,
    # (extended length L + nperseg), so the inverse is L % hop samples short and only that
    # prefix can be compared
    m = min(L, y.shape[1])
    assert m == (L if padded else L - L % (n - nov))
    check("round trip " + _id(cfg), y[:, :m].cpu().numpy().astype(np.float64),
          signal(L)[:, :m].astype(np.float64))


@pytest.mark.parametrize("case", BASE, ids=BASE_IDS)
def test_gain_is_fused_into_the_bin_load(gpu_device, case):
    cfg = (case, "zeros", True, False, "spectrum")
    L, n, nov, w = case
    f, t, Z, Z32, ti, xi = reference(cfg)
    B, F, T = Z32.shape
    g = np.random.default_rng(11).uniform(0.0, 1.0, size=(B, F, T)).astype(np.float32)
    Zd = to_dev(Z32, gpu_device)
    keep = Zd.clone()
    kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, boundary=True)
    _, ref_full = scipy.signal.istft(Z32.astype(np.complex128) * g.astype(np.float64), **kw)
    got = inverse(Zd, cfg, to_dev(g, gpu_device))
    check(f"gain [F] {BASE_IDS[BASE.index(case)]}", got.cpu().numpy().astype(np.float64), ref_full)
    g0 = g.astype(np.float64).copy()
    g0[:, F - 1] = 0.0
    _, ref_drop = scipy.signal.istft(Z32.astype(np.complex128) * g0, **kw)
    got = inverse(Zd, cfg, to_dev(np.ascontiguousarray(g[:, :F - 1]), gpu_device))
    check(f"gain [F-1] {BASE_IDS[BASE.index(case)]}", got.cpu().numpy().astype(np.float64),
          ref_drop)
    assert torch.equal(torch.view_as_real(Zd), torch.view_as_real(keep)), "Z was overwritten"


def bits(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", BASE, ids=BASE_IDS)
def test_deterministic_and_batch_independent(gpu_device, case):
    cfg = (case, "zeros", True, False, "spectrum")
    L = case[0]
    x5 = to_dev(signal(L, 5), gpu_device)
    Z5 = forward(x5, cfg)
    assert torch.equal(bits(Z5), bits(forward(x5, cfg))), "forward: two runs differ"
    for b in range(5):
        Zb = forward(x5[b:b + 1].contiguous(), cfg)
        assert torch.equal(bits(Zb[0]), bits(Z5[b])), f"forward: batch of 1 differs (shot {b})"
    y5 = inverse(Z5, cfg)
    assert not torch.isnan(y5).any()
    assert torch.equal(bits(y5), bits(inverse(Z5, cfg))), "inverse: two runs differ"
    for b in range(5):
        yb = inverse(Z5[b:b + 1].contiguous(), cfg)
        assert torch.equal(bits(yb[0]), bits(y5[b])), f"inverse: batch of 1 differs (shot {b})"


@pytest.mark.parametrize("case", BASE[:3], ids=BASE_IDS[:3])
def test_strided_input_same_bits(gpu_device, case):
    cfg = (case, "zeros", True, False, "spectrum")
    L = case[0]
    x = to_dev(signal(L), gpu_device)
    wide = torch.full((3, L + 37), float("nan"), dtype=torch.float32, device=gpu_device)
    wide[:, :L] = x
    xs = wide[:, :L]
    assert xs.stride(0) == L + 37 and xs.stride(1) == 1
    assert torch.equal(bits(forward(xs, cfg)), bits(forward(x, cfg)))


def test_opcheck(gpu_device):
    ops = torch.ops.specenh
    x = to_dev(signal(4000), gpu_device)
    Z = ops.stft_complex(x, 64, 48, "hamm", FS, 1, 0, 1, True)
    g = torch.rand(Z.shape[0], Z.shape[1] - 1, Z.shape[2], device=gpu_device)
    n = (Z.shape[2] - 1) * 16
    cases = [
        (ops.stft_complex, (x, 64, 48, "hamm", FS, 1, 0, 1, True)),
        (ops.stft_complex, (x, 64, 48, "hamm", FS, 0, 2, 0, False)),
        (ops.stft_complex_out, (x, 64, 48, "hamm", FS, 1, 0, 1, True, torch.empty_like(Z))),
        (ops.istft, (Z, None, 64, 48, "hamm", FS, 1, True)),
        (ops.istft, (Z, g, 64, 48, "hamm", FS, 0, False)),
        (ops.istft_out, (Z, g, 64, 48, "hamm", FS, 1, True,
                         torch.empty(Z.shape[0], n, device=gpu_device))),
    ]
    for op, args in cases:
        torch.library.opcheck(op, args)


def test_numpy_layer_shapes_and_dtypes(gpu_device):
    from specenh import signal as sig

    cfg = CONFIGS[0]
    (L, n, nov, w), *_ = cfg
    f, t, Z, Z32, ti, xi = reference(cfg)
    fg, tg, Zg = sig.stft(signal(L), fs=FS, window=w, nperseg=n, noverlap=nov)
    assert Zg.dtype == np.complex128 and Zg.shape == Z.shape
    assert np.array_equal(fg, f) and np.array_equal(tg, t)
    check("numpy stft", Zg, Z)
    t2, x2 = sig.istft(Z32, fs=FS, window=w, nperseg=n, noverlap=nov)
    assert x2.dtype == np.float64 and x2.shape == xi.shape
    # one time per output sample (scipy 1.15 sizes t by the leading axis of a batched input)
    assert np.array_equal(t2, np.arange(xi.shape[-1]) / FS)
    check("numpy istft", x2, xi)
    f1, t1, Z1 = sig.stft(signal(L)[0], fs=FS, window=w, nperseg=n, noverlap=nov)
    assert Z1.shape == Z.shape[1:]
    t3, x3 = sig.istft(Z32[0], fs=FS, window=w, nperseg=n, noverlap=nov)
    ts, xs = scipy.signal.istft(Z32[0].astype(np.complex128), fs=FS, window=w, nperseg=n,
                                noverlap=nov)
    assert x3.shape == xs.shape and np.array_equal(t3, ts)
