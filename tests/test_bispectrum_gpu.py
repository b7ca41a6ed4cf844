"""Bispectrum and squared bicoherence on the GPU (csrc/bispectrum.hip) against the numpy
reference of tests/bispectrum_local.py run in fp64 on the fp32 samples widened.

Bounds, both those of tests/test_spectral_gpu.py. Bispectrum: 1e-5 normwise per shot and group
(max|got - ref| / max|ref| over the plane), the project's contract for fp32 spectra. b2: max
abs error against fp64, allowed min(max(4 x the reference's own float32 error on the same
inputs, 2e-6), 5e-5) (4x because the GPU transform and summation order differ from
pocketfft's). Integer spectra through bispectrum_from_spectra leave no rounding at all: there
the bispectrum must equal numpy bit for bit and b2 to 1 ulp, so an indexing mistake cannot hide
under a tolerance. Every output buffer is NaN-filled before the launch. The tests print their
measured and allowed values (pytest -s); DESIGN.md 5.10 records them.

At nperseg >= 1024 the whole plane is computed and checked for NaN and for the zeros outside
the domain on the device; against the reference go the rows and columns SEL of it (the first
48 bins, 48 around N/4 and the last 48 up to N/2: the tile edges, the diagonal and both ends
of the domain's edge k + l = N/2), so the reference needs only a 144 x 144 plane.
"""
import functools

import numpy as np
import pytest
import torch

import bispectrum_local as bl

pytestmark = pytest.mark.gpu

FS = 5e5
TOL_BISPEC = 1e-5
SCALING = {"density": 0, "spectrum": 1}
DETREND = {False: 0, "constant": 1, "linear": 2}
BOTH = 3

# (nperseg, noverlap, window, detrend, navg, scaling, B); L = 9 nperseg + 37
PARITY = [
    (64, 48, "hann", "linear", 0, "density", 3),        # T = 35: chunks 32 + 3; K = 33 < a tile
    (128, 64, "hamm", "linear", 3, "density", 3),       # T = 17: G = 5, two frames dropped
    (256, 128, "hann", "constant", 0, "density", 3),
    (256, 128, "hann", "linear", 2, "spectrum", 3),
    (512, 256, "hamm", "linear", 4, "density", 3),
    (1024, 768, "hamm", "linear", 1, "density", 3),     # one frame a group: b2 = 1
    (2048, 1536, "hann", "linear", 0, "density", 3),    # T = 33: chunks 32 + 1
    (4096, 3072, "hann", False, 3, "density", 1),
]


def _id(c):
    return "-".join(str(v) for v in c)


def sel_for(n):
    """None (the whole plane) below 1024, else the bins compared with the reference."""
    if n < 1024:
        return None
    return np.concatenate([np.arange(48), np.arange(n // 4 - 24, n // 4 + 24),
                           np.arange(n // 2 - 47, n // 2 + 1)])


@functools.lru_cache(maxsize=None)
def signals(B, L):
    """The partly coherent x, y of tests/test_spectral_gpu.py and z = x y + 0.3 x, fp32."""
    from test_spectral_gpu import signals as xy

    x, y = xy(B, L)
    z = (x.astype(np.float64) * y + 0.3 * x).astype(np.float32)
    z.setflags(write=False)
    return x, y, z


def ref_kw(cfg):
    n, nov, w, detrend, navg, scaling = cfg[:6]
    return dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, scaling=scaling,
                navg=navg)


def allowed_from(ref_b2, f32_b2):
    err32 = float(np.nanmax(np.abs(f32_b2.astype(np.float64) - ref_b2)))
    return err32, min(max(4.0 * err32, 2e-6), 5e-5)


@functools.lru_cache(maxsize=None)
def reference(cfg, cross):
    """The fp64 truth on sel_for(nperseg), and the b2 error allowed: from the reference's own
    float32 run."""
    B, L = cfg[6], 9 * cfg[0] + 37
    sig = signals(B, L) if cross else (signals(B, L)[0], None, None)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = bl.bispectrum(*sig, sel=sel_for(cfg[0]), dtype=np.float64, **ref_kw(cfg))
        f32 = bl.bispectrum(*sig, sel=sel_for(cfg[0]), dtype=np.float32, **ref_kw(cfg))
    assert f32[0].dtype == np.complex64 and f32[1].dtype == np.float32
    assert not np.isnan(f32[1]).any() and not np.isnan(ref[1]).any()
    err32, allowed = allowed_from(ref[1], f32[1])
    for a in ref:
        a.setflags(write=False)
    return ref, err32, allowed


def upload(dev, *arrs):
    return [None if a is None else torch.from_numpy(np.array(a)).to(dev) for a in arrs]


def op_args(cfg):
    n, nov, w, detrend, navg, scaling = cfg[:6]
    return (n, nov, w, FS, SCALING[scaling], DETREND[detrend], navg)


def nan_outputs(dev, shape, mask=BOTH):
    nan = float("nan")
    return [None if not mask >> i & 1 else
            torch.full(shape, complex(nan, nan) if i == 0 else nan,
                       dtype=torch.complex64 if i == 0 else torch.float32, device=dev)
            for i in range(2)]


def launch(dev, x, y, z, cfg, nbins=0, mask=BOTH, ws=None):
    """torch.ops.specenh.bispectrum_out into NaN-filled buffers: (bispec, bicoh), None where
    not asked for."""
    n, nov = cfg[0], cfg[1]
    B, L = x.shape
    T = (L - n) // (n - nov) + 1
    K = nbins if nbins > 0 else n // 2 + 1
    outs = nan_outputs(dev, (B, 1 if cfg[4] <= 0 else T // cfg[4], K, K), mask)
    torch.ops.specenh.bispectrum_out(x, y, z, *op_args(cfg), nbins, *outs, ws)
    return outs


def outside(K, F, dev):
    k = torch.arange(K, device=dev)
    return k[:, None] + k[None, :] > F - 1


def normwise(got, ref):
    """max over (shot, group) of max|got - ref| / max|ref| over the plane."""
    num = np.abs(got - ref).max(axis=(2, 3))
    den = np.abs(ref).max(axis=(2, 3))
    return float((num / den).max())


@pytest.mark.parametrize("cross", [False, True], ids=["auto", "cross"])
@pytest.mark.parametrize("cfg", PARITY, ids=[_id(c) for c in PARITY])
def test_parity_with_the_fp64_reference(gpu_device, cfg, cross):
    dev = gpu_device
    n, B = cfg[0], cfg[6]
    F = n // 2 + 1
    (rB, rc), err32, allowed = reference(cfg, cross)
    x, y, z = upload(dev, *signals(B, 9 * n + 37))
    bis, coh = launch(dev, x, y if cross else None, z if cross else None, cfg)
    assert bis.shape == coh.shape == (B, rB.shape[1], F, F)
    assert not torch.isnan(torch.view_as_real(bis)).any() and not torch.isnan(coh).any()
    out = outside(F, F, dev)
    assert not torch.view_as_real(bis)[:, :, out].any() and not coh[:, :, out].any()
    sel = sel_for(n)
    if sel is not None:
        s = torch.from_numpy(sel).to(dev)
        bis, coh = bis[:, :, s][:, :, :, s], coh[:, :, s][:, :, :, s]
    gB, gc = bis.cpu().numpy(), coh.cpu().numpy()
    assert gB.dtype == np.complex64 and gc.dtype == np.float32
    berr = normwise(gB.astype(np.complex128), rB)
    cerr = float(np.abs(gc.astype(np.float64) - rc).max())
    print(f"\n[bispectrum {_id(cfg)} {'cross' if cross else 'auto'}] bispec {berr:.2e} (bound "
          f"{TOL_BISPEC:.0e}); b2 {cerr:.2e} allowed {allowed:.2e} (reference float32 "
          f"{err32:.2e}); b2 range {rc[rc > 0].min():.1e}..{rc.max():.3f}")
    assert berr <= TOL_BISPEC
    assert cerr <= allowed
    if cfg[4] == 1:  # one frame a group: b2 is 1 wherever it is defined
        k = np.arange(F) if sel is None else sel
        inside = k[:, None] + k[None, :] <= F - 1
        assert float(np.abs(gc[:, :, inside] - 1.0).max()) <= allowed


def integer_spectra(B, T, F, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, (B, T, F)) + 1j * rng.integers(-3, 4, (B, T, F))).astype(
        np.complex64)


@pytest.mark.parametrize("navg", [0, 7])
@pytest.mark.parametrize("cross", [False, True], ids=["auto", "cross"])
def test_exact_arithmetic_from_spectra(gpu_device, navg, cross):
    """Integer components in [-3, 3], F = 33, T = 40 (a chunk and a quarter): every fp32 sum
    is exact, so nothing but the final rounding separates the kernel from numpy."""
    from specenh import bispectrum as bs

    dev = gpu_device
    B, T, F = 2, 40, 33
    S = [integer_spectra(B, T, F, s) for s in (1, 2, 3)] if cross else \
        [integer_spectra(B, T, F, 1)] * 3
    glen = navg or T
    k = np.arange(F)
    rB, rc = [], []
    for g in range(T // glen):
        X, Y, Z = (s[:, g * glen:(g + 1) * glen].transpose(0, 2, 1).astype(np.complex128)
                   for s in S)
        Bg, cg = bl.accumulate(X, Y, Z, k, k)
        rB.append(Bg.astype(np.complex64))  # exact sum / frames, rounded once to fp64, once to fp32
        rc.append(cg)
    rB, rc = np.stack(rB, axis=1), np.stack(rc, axis=1)
    assert np.isfinite(rc).all() and (rc > 0).sum() > 500
    Xd, Yd, Zd = upload(dev, *S)
    outs = nan_outputs(dev, rB.shape)
    torch.ops.specenh.bispectrum_spectra_out(Xd, Yd if cross else None, Zd if cross else None,
                                             navg, 0, *outs)
    gB, gc = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert torch.equal(outs[0].cpu(), torch.from_numpy(rB))  # bit for bit, the zeros included
    r32 = rc.astype(np.float32)
    assert (np.abs(gc - r32) <= np.spacing(r32)).all()
    assert not gc[:, :, k[:, None] + k[None, :] > F - 1].any()
    est = bs.bispectrum_from_spectra(Xd, Yd if cross else None, Zd if cross else None, navg=navg)
    assert torch.equal(est["bispec"], outs[0]) and torch.equal(est["bicoh"], outs[1])
    one = bs.bispectrum_from_spectra(Xd[1], None if not cross else Yd[1],
                                     None if not cross else Zd[1], navg=navg, nbins=20,
                                     want=("bicoh",))
    assert list(one) == ["bicoh"] and torch.equal(one["bicoh"], outs[1][1, :, :20, :20])
    assert gB.dtype == np.complex64


MID = (256, 128, "hann", "linear", 2, "density")  # L = 2341: T = 17, G = 8, one frame dropped


@pytest.mark.parametrize("cross", [False, True], ids=["auto", "cross"])
def test_nbins_is_the_corner_of_the_full_plane(gpu_device, cross):
    dev = gpu_device
    x, y, z = upload(dev, *signals(3, 9 * 256 + 37))
    y, z = (y, z) if cross else (None, None)
    full = launch(dev, x, y, z, MID)
    for K in (1, 7, 33, 45):
        part = launch(dev, x, y, z, MID, nbins=K)
        for p, f in zip(part, full):
            assert p.shape == (3, 8, K, K) and torch.equal(p, f[:, :, :K, :K])


DET = (64, 48, "hamm", "linear")  # L = 1184: T = 71, three chunks at navg = 0


@pytest.mark.parametrize("navg", [0, 5])
def test_batch_stride_and_subset_independence(gpu_device, navg, monkeypatch):
    from specenh import bispectrum as bs

    dev = gpu_device
    cfg = DET + (navg, "density")
    x, y, z = upload(dev, *signals(5, 1184))
    for sig in ((x, None, None), (x, y, z), (x, None, y)):
        full = launch(dev, *sig, cfg)
        for o in full:
            assert not torch.isnan(torch.view_as_real(o) if o.is_complex() else o).any()
        for b in range(5):  # a batch of 5 = five batches of 1, bitwise
            one = launch(dev, *(None if s is None else s[b:b + 1] for s in sig), cfg)
            for o, f in zip(one, full):
                assert torch.equal(o[0], f[b])
        wide = [None if s is None else torch.zeros(5, 1250 + 25 * i, device=dev)
                for i, s in enumerate(sig)]
        for w, s in zip(wide, sig):
            if s is not None:
                w[:, :1184] = s
        strided = launch(dev, *(None if w is None else w[:, :1184] for w in wide), cfg)
        for o, f in zip(strided, full):  # a stride beyond the length
            assert torch.equal(o, f)
        for bit in range(2):  # each output asked for alone = the same values
            sub = launch(dev, *sig, cfg, mask=1 << bit)
            assert [o is None for o in sub] == [i != bit for i in range(2)]
            assert torch.equal(sub[bit], full[bit])
        # the tensor layer, unsplit and split into launches of two shots by a small cap
        kw = dict(fs=FS, window="hamm", nperseg=64, noverlap=48, detrend="linear", navg=navg)
        f, t, est = bs.bispectrum(*sig, **kw)
        assert torch.equal(est["bispec"], full[0]) and torch.equal(est["bicoh"], full[1])
        nsig = 1 + sum(s is not None for s in sig[1:])
        T = 71
        with monkeypatch.context() as mp:
            mp.setattr(bs, "CSM_WORKSPACE_CAP", 2 * 8 * nsig * (T // (navg or T)) * (navg or T) * 33)
            _, _, split = bs.bispectrum(*sig, **kw)
        for name in ("bispec", "bicoh"):
            assert torch.equal(split[name], est[name])


def test_auto_symmetry_and_aliases(gpu_device):
    from specenh import bispectrum as bs

    dev = gpu_device
    x, y, _ = upload(dev, *signals(3, 9 * 256 + 37))
    bis, coh = launch(dev, x, None, None, MID)
    assert torch.equal(coh, coh.transpose(-1, -2)) and torch.equal(bis, bis.transpose(-1, -2))
    for sig in ((x, x, None), (x, None, x), (x, x, x)):  # the same tensor is no second signal
        again = launch(dev, *sig, MID)
        assert torch.equal(again[0], bis) and torch.equal(again[1], coh)
    kw = dict(fs=FS, window="hann", nperseg=256, noverlap=128, detrend="linear", navg=2)
    _, _, a = bs.bispectrum(x, **kw)
    _, _, b = bs.bispectrum(x, x, x, **kw)
    assert torch.equal(a["bicoh"], coh) and torch.equal(b["bicoh"], coh)
    assert torch.equal(a["bispec"], bis) and torch.equal(b["bispec"], bis)
    # z = y twice: two signals' worth of workspace, the values of three tensors
    two = launch(dev, x, y, y, MID)
    three = launch(dev, x, y, y.clone(), MID)
    assert torch.equal(two[0], three[0]) and torch.equal(two[1], three[1])


def test_workspace_is_fully_written(gpu_device):
    from specenh import ops

    dev = gpu_device
    cfg = DET + (5, "density")  # T = 71: 14 groups of 5, one frame dropped
    x, y, z = upload(dev, *signals(5, 1184))
    for sig, nsig in (((x, None, None), 1), ((x, y, None), 2), ((x, y, z), 3)):
        need = ops.bispectrum_workspace(*sig, *op_args(cfg)).numel()
        assert need == 5 * nsig * 70 * 33 * 8
        ws = torch.full((need // 4,), float("nan"), device=dev)
        outs = launch(dev, *sig, cfg, ws=ws)
        assert not torch.isnan(ws).any()
        ref = launch(dev, *sig, cfg)
        for o, r in zip(outs, ref):
            assert torch.equal(o, r)
        with pytest.raises(ValueError, match="workspace"):
            launch(dev, *sig, cfg, ws=ws.view(torch.uint8)[:-1])


def test_all_zero_input(gpu_device):
    dev = gpu_device
    zero = torch.zeros(2, 1184, device=dev)
    out = outside(33, 33, dev)
    for navg in (0, 5):
        for sig in ((zero, None, None), (zero, torch.zeros_like(zero), torch.zeros_like(zero))):
            bis, coh = launch(dev, *sig, DET + (navg, "density"))
            assert torch.equal(torch.view_as_real(bis), torch.zeros_like(torch.view_as_real(bis)))
            assert torch.isnan(coh[:, :, ~out]).all()
            assert torch.equal(coh[:, :, out], torch.zeros_like(coh[:, :, out]))


def test_coupling_detection(gpu_device):
    """The recipe of tests/test_bispectrum_cpu.py on the GPU: b2[20, 12] of the coupled and of
    the uncoupled signal within the b2 bound of the reference."""
    from specenh import bispectrum as bs

    for coupled in (True, False):
        s = bl.coupling_signal(coupled)
        ref = bl.bispectrum(s, dtype=np.float64, **bl.COUPLING)[1]
        f32 = bl.bispectrum(s, dtype=np.float32, **bl.COUPLING)[1]
        err32, allowed = allowed_from(ref, f32)
        kw = {k: v for k, v in bl.COUPLING.items() if k != "scaling"}
        f, b2 = bs.bicoherence(torch.from_numpy(s).to(gpu_device), **kw)
        assert b2.shape == (65, 65) and f.shape == (65,)
        got = float(b2[20, 12])
        print(f"\n[bispectrum coupling coupled={coupled}] b2[20,12] {got:.6f} reference "
              f"{ref[0, 0, 20, 12]:.6f} allowed {allowed:.2e} (reference float32 {err32:.2e})")
        assert abs(got - ref[0, 0, 20, 12]) <= allowed
        assert float(np.abs(b2.cpu().numpy().astype(np.float64) - ref[0, 0]).max()) <= allowed
        assert (got >= 0.9) if coupled else (got <= 0.25)
        summed = bs.summed_bicoherence(b2)
        assert summed.shape == (65,) and summed.device == b2.device
        if coupled:
            assert int(summed[1:].argmax()) + 1 == 32


def test_tensor_and_numpy_layers(gpu_device):
    from specenh import bispectrum as bs
    from specenh import signal, stft

    dev = gpu_device
    x, y, z = signals(3, 9 * 256 + 37)
    xd, yd, zd = upload(dev, x, y, z)
    kw = dict(fs=FS, window="hann", nperseg=256, noverlap=128, detrend="linear")
    f, t, est = bs.bispectrum(xd, yd, zd, navg=2, nbins=40, **kw)
    assert np.array_equal(f, stft.frequencies(256, FS)[:40]) and t.shape == (8,)
    assert sorted(est) == ["bicoh", "bispec"]
    assert est["bispec"].shape == est["bicoh"].shape == (3, 8, 40, 40)
    assert (est["bispec"].dtype, est["bicoh"].dtype) == (torch.complex64, torch.float32)
    f, t, one = bs.bispectrum(xd[1], yd[1], zd[1], navg=2, nbins=40, want=("bicoh",), **kw)
    assert list(one) == ["bicoh"] and torch.equal(one["bicoh"], est["bicoh"][1])
    f, b2 = bs.bicoherence(xd, yd, zd, nbins=40, **kw)
    assert b2.shape == (3, 40, 40) and b2.dtype == torch.float32
    # float64 and strided input are converted, the values those of the fp32 copy
    f, b2d = bs.bicoherence(xd.double(), yd.double(), zd.double(), nbins=40, **kw)
    assert torch.equal(b2d, b2)
    # numpy layer: leading axes flattened into the batch and restored, fp64 out
    f, n2 = signal.bicoherence(x.reshape(3, 1, -1), y.reshape(3, 1, -1), z.reshape(3, 1, -1),
                               nbins=40, **kw)
    assert n2.shape == (3, 1, 40, 40) and n2.dtype == np.float64 and f.shape == (40,)
    assert np.array_equal(n2[:, 0], b2.cpu().numpy().astype(np.float64))
    f, n1 = signal.bicoherence(x[0].astype(np.float64), **kw)  # 1-D in, [K, K] out
    assert n1.shape == (129, 129) and f.shape == (129,)
    assert np.array_equal(n1, n1.T)


def test_opcheck(gpu_device):
    from specenh import ops

    dev = gpu_device
    x, y, z = upload(dev, *signals(3, 9 * 256 + 37))
    args = op_args(MID)[:-1]
    op = torch.ops.specenh.bispectrum.default
    torch.library.opcheck(op, (x, None, None, *args, 2, 0, BOTH))
    torch.library.opcheck(op, (x, y, z, *args, 0, 33, 1))
    torch.library.opcheck(op, (x, None, z, *args, 0, 7, 2))
    shape = (3, 8, 45, 45)
    ws = ops.bispectrum_workspace(x, y, z, *args, 2)
    torch.library.opcheck(torch.ops.specenh.bispectrum_out.default,
                          (x, y, z, *args, 2, 45,
                           torch.empty(shape, dtype=torch.complex64, device=dev),
                           torch.empty(shape, device=dev), ws))
    torch.library.opcheck(torch.ops.specenh.bispectrum_out.default,
                          (x, None, None, *args, 2, 45, None, torch.empty(shape, device=dev),
                           None))
    X, Y = upload(dev, integer_spectra(2, 40, 33, 1), integer_spectra(2, 40, 33, 2))
    op = torch.ops.specenh.bispectrum_spectra.default
    torch.library.opcheck(op, (X, None, None, 0, 0, BOTH))
    torch.library.opcheck(op, (X, Y, X, 7, 9, 2))
    torch.library.opcheck(torch.ops.specenh.bispectrum_spectra_out.default,
                          (X, Y, None, 7, 9, torch.empty(2, 5, 9, 9, dtype=torch.complex64,
                                                          device=dev),
                           torch.empty(2, 5, 9, 9, device=dev)))


def test_graph_capture(gpu_device):
    """Both entry points launch without allocating, so a captured graph replays them: the
    replay on new samples equals the eager call."""
    from specenh import ops

    dev = gpu_device
    x, y, z = upload(dev, *signals(3, 9 * 256 + 37))
    args = op_args(MID)
    ws = ops.bispectrum_workspace(x, y, z, *args)
    eager = launch(dev, x, y, z, MID, nbins=45, ws=ws)
    X = upload(dev, integer_spectra(2, 40, 33, 1))[0]
    eager_s = nan_outputs(dev, (2, 5, 33, 33))
    torch.ops.specenh.bispectrum_spectra_out(X, None, None, 7, 0, *eager_s)
    xs, ys, zs, Xs = (torch.zeros_like(v) for v in (x, y, z, X))
    outs = nan_outputs(dev, (3, 8, 45, 45))
    outs_s = nan_outputs(dev, (2, 5, 33, 33))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        torch.ops.specenh.bispectrum_out(xs, ys, zs, *args, 45, *outs, ws)
        torch.ops.specenh.bispectrum_spectra_out(Xs, None, None, 7, 0, *outs_s)
    xs.copy_(x), ys.copy_(y), zs.copy_(z), Xs.copy_(X)
    g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs + outs_s, eager + eager_s):
        assert torch.equal(o, e)
