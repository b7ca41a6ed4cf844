"""Time-averaged spectra on the GPU (csrc/spectral_mean.hip) against scipy.signal.welch /
csd / coherence called in fp64 on the fp32 samples widened. Group g of a block-averaged call
is scipy on the slice x[g navg hop : g navg hop + (navg - 1) hop + nperseg].

Bounds. pxx, pyy, pxy: 1e-5 normwise per shot and group (max|got - ref| / max|ref|), the
project's contract for fp32 spectra. Coherence: max abs error against fp64, allowed
max(4 x scipy's own float32 error on the same inputs, 2e-6), capped at 5e-5 (4x because the
GPU transform and accumulation order differ from pocketfft's). Every output buffer is
NaN-filled before the launch, so an element the kernel does not write fails the comparison.
Each test prints its measured and allowed values (pytest -s); DESIGN.md 5.7 records them.
"""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

pytestmark = pytest.mark.gpu

FS = 5e5
TOL_PSD = 1e-5
SCALING = {"density": 0, "spectrum": 1}
DETREND = {False: 0, "constant": 1, "linear": 2}
ALL = 15

# (nperseg, noverlap, window, detrend, navg, scaling); L = 9 nperseg + 37, B = 3
PARITY = [
    (64, 48, "hann", "linear", 0, "density"),        # T = 35: two chunks, the workspace path
    (256, 128, "hann", "constant", 0, "density"),    # T = 17: one odd group
    (256, 128, "hann", "linear", 2, "density"),      # G = 8, one frame dropped
    (256, 128, "hann", "linear", 2, "spectrum"),
    (512, 256, "hamm", "linear", 4, "density"),      # T = 17: G = 4, one frame dropped
    (1024, 768, "hamm", "linear", 1, "density"),     # T = 33 groups of one frame
    (4096, 3072, "hann", False, 3, "density"),       # T = 33: G = 11
    (128, 96, "hamm", "linear", 0, "density"),       # T = 34: chunks of 32 + 2, the workspace path
    (128, 64, "hann", "constant", 3, "spectrum"),    # T = 17: G = 5, two frames dropped
    (2048, 1536, "hann", "linear", 0, "density"),    # T = 33: chunks 32 + 1; the 2048 kernels
    (2048, 1024, "hamm", False, 2, "density"),       # T = 17: G = 8, one frame dropped
]
LONG = [(64, 48, "hann", "linear", 0, "density"),    # T = 4101: 129 chunks
        (64, 48, "hann", "linear", 7, "density")]    # G = 585, 6 frames dropped
L_LONG = 65664


def _id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def signals(B, L, seed=11):
    """x and a partly coherent y (fp64 recipe, cast to fp32): coherence 2e-4 .. 1."""
    from specenh.synthetic import plasma_chirps

    x = plasma_chirps(B, L, seed0=seed, dtype=np.float64)
    y = 0.7 * np.roll(x, 3, axis=1) + 0.5 * plasma_chirps(B, L, seed0=seed + 100,
                                                          dtype=np.float64)
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def scipy_groups(x, y, cfg, dtype):
    """pxx, pyy, pxy, coh [B, F, G] from scipy on each group's slice, computed in `dtype`."""
    n, nov, w, detrend, navg, scaling = cfg
    hop = n - nov
    x, y = x.astype(dtype), y.astype(dtype)
    T = (x.shape[1] - n) // hop + 1
    glen = navg if navg >= 1 else T
    kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, scaling=scaling)
    out = [[], [], [], []]
    for g in range(T // glen):
        sl = slice(g * glen * hop, g * glen * hop + (glen - 1) * hop + n)
        _, pxx = scipy.signal.welch(x[:, sl], **kw)
        _, pyy = scipy.signal.welch(y[:, sl], **kw)
        _, pxy = scipy.signal.csd(x[:, sl], y[:, sl], **kw)
        coh = np.abs(pxy) ** 2 / pxx / pyy  # scipy.signal.coherence, from the same parts
        for o, v in zip(out, (pxx, pyy, pxy, coh)):
            o.append(v)
    return [np.stack(o, axis=-1) for o in out]


@functools.lru_cache(maxsize=None)
def reference(B, L, cfg):
    """The fp64 truth, and the coherence error allowed: from scipy's own float32 run."""
    x, y = signals(B, L)
    with np.errstate(invalid="ignore", divide="ignore"):
        ref = scipy_groups(x, y, cfg, np.float64)
        f32 = scipy_groups(x, y, cfg, np.float32)
    assert f32[2].dtype == np.complex64  # scipy really ran in float32
    err32 = float(np.abs(f32[3].astype(np.float64) - ref[3]).max())
    allowed = min(max(4.0 * err32, 2e-6), 5e-5)
    for a in ref:
        a.setflags(write=False)
    return ref, err32, allowed


def launch(dev, x, y, cfg, mask=ALL, ws=None):
    """torch.ops.specenh.spectral_mean_out into NaN-filled buffers; returns the four outputs
    (None where not asked for) and the workspace."""
    from specenh import ops

    n, nov, w, detrend, navg, scaling = cfg
    args = (n, nov, w, FS, SCALING[scaling], DETREND[detrend], navg)
    B, L = x.shape
    T = (L - n) // (n - nov) + 1
    shape = (B, n // 2 + 1, 1 if navg <= 0 else T // navg)
    nan = float("nan")
    outs = [None if not mask >> i & 1 else
            torch.full(shape, complex(nan, nan) if i == 2 else nan,
                       dtype=torch.complex64 if i == 2 else torch.float32, device=dev)
            for i in range(4)]
    if ws is None:
        ws = ops.spectral_workspace(x, *args)
    ops.ops.spectral_mean_out(x, y, *args, *outs, ws)
    return outs, ws


def normwise(got, ref):
    """max over (shot, group) of max_f |got - ref| / max_f |ref|."""
    num = np.abs(got - ref).max(axis=1)
    den = np.abs(ref).max(axis=1)
    return float((num / den).max())


def check_case(dev, B, L, cfg, label):
    ref, err32, allowed = reference(B, L, cfg)
    x, y = signals(B, L)
    xd, yd = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(y)).to(dev)
    outs, _ = launch(dev, xd, yd, cfg)
    got = [o.cpu().numpy() for o in outs]
    assert got[2].dtype == np.complex64
    errs = [normwise(got[i].astype(ref[i].dtype), ref[i]) for i in range(3)]
    cerr = float(np.abs(got[3].astype(np.float64) - ref[3]).max())
    w_only = launch(dev, xd, None, cfg, mask=1)[0][0]
    werr = normwise(w_only.cpu().numpy().astype(np.float64), ref[0])
    print(f"\n[spectral {label}] pxx {errs[0]:.2e} pyy {errs[1]:.2e} pxy {errs[2]:.2e} "
          f"welch(x alone) {werr:.2e} (bound {TOL_PSD:.0e}); coherence {cerr:.2e} allowed "
          f"{allowed:.2e} (scipy float32 {err32:.2e}); coherence range "
          f"{ref[3].min():.1e}..{ref[3].max():.3f}")
    for e in errs + [werr]:
        assert e <= TOL_PSD
    assert cerr <= allowed
    return got


@pytest.mark.parametrize("cfg", PARITY, ids=[_id(c) for c in PARITY])
def test_parity_with_scipy(gpu_device, cfg):
    L = 9 * cfg[0] + 37
    got = check_case(gpu_device, 3, L, cfg, _id(cfg))
    T = (L - cfg[0]) // (cfg[0] - cfg[1]) + 1
    assert got[0].shape == (3, cfg[0] // 2 + 1, 1 if cfg[4] <= 0 else T // cfg[4])


@pytest.mark.parametrize("cfg", LONG, ids=[_id(c) for c in LONG])
def test_long_reduction_and_chunk_split(gpu_device, cfg):
    from specenh import ops, spectral

    T = (L_LONG - 64) // 16 + 1
    assert T == 4101 and T > spectral.CHUNK_FRAMES
    check_case(gpu_device, 2, L_LONG, cfg, "long " + _id(cfg))
    if cfg[4] <= 0:  # the workspace path really ran: 129 chunks of partials
        x = torch.zeros(2, L_LONG, device=gpu_device)
        ws = ops.spectral_workspace(x, 64, 48, "hann", FS, 0, 2, 0)
        assert ws.numel() == 2 * -(-T // spectral.CHUNK_FRAMES) * 33 * 16


EDGE = (256, 128, "hann", "constant")


@pytest.mark.parametrize("L,navg", [(256, 0), (256, 1), (384, 0), (384, 2), (384, 1),
                                    (9 * 256 + 37, 17), (9 * 256 + 37, 1)])
def test_edge_shapes(gpu_device, L, navg):
    cfg = EDGE + (navg, "density")
    got = check_case(gpu_device, 3, L, cfg, f"edge L={L} navg={navg}")
    if navg == 1:
        from specenh import stft

        _, _, allowed = reference(3, L, cfg)
        assert float(np.abs(got[3] - 1.0).max()) <= allowed
        x, _ = signals(3, L)
        S = stft.stft_psd(torch.from_numpy(np.array(x)).to(gpu_device), 256, 128, window="hann",
                          fs=FS, scaling="density", detrend="constant").cpu().numpy()
        assert S.shape == got[0].shape
        assert normwise(got[0].astype(np.float64), S.astype(np.float64)) <= TOL_PSD


DET = (64, 48, "hamm", "linear")  # L = 1184: T = 71, three chunks at navg = 0


@pytest.mark.parametrize("navg", [0, 5])
def test_batch_stride_and_subset_independence(gpu_device, navg):
    dev = gpu_device
    cfg = DET + (navg, "density")
    x, y = signals(5, 1184)
    xd, yd = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(y)).to(dev)
    full, _ = launch(dev, xd, yd, cfg)
    for o in full:
        assert not torch.isnan(torch.view_as_real(o) if o.is_complex() else o).any()
    for b in range(5):  # batch of 5 = five batches of 1, bitwise
        one, _ = launch(dev, xd[b:b + 1], yd[b:b + 1], cfg)
        for o, f in zip(one, full):
            assert torch.equal(o[0], f[b])
    wide_x = torch.zeros(5, 1300, device=dev)
    wide_y = torch.zeros(5, 1250, device=dev)
    wide_x[:, :1184], wide_y[:, :1184] = xd, yd
    strided, _ = launch(dev, wide_x[:, :1184], wide_y[:, :1184], cfg)  # x_stride > length
    for o, f in zip(strided, full):
        assert torch.equal(o, f)
    for bit in range(4):  # a subset of the outputs = the same values
        sub, _ = launch(dev, xd, yd, cfg, mask=1 << bit)
        assert [o is None for o in sub] == [i != bit for i in range(4)]
        assert torch.equal(sub[bit], full[bit])


def test_workspace_is_fully_written(gpu_device):
    from specenh import ops

    dev = gpu_device
    cfg = DET + (0, "density")
    x, y = signals(5, 1184)
    xd, yd = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(y)).to(dev)
    need = ops.spectral_workspace(xd, 64, 48, "hamm", FS, 0, 2, 0).numel()
    assert need == 5 * 3 * 33 * 16
    ws = torch.full((need // 4,), float("nan"), device=dev)
    outs, _ = launch(dev, xd, yd, cfg, ws=ws)
    assert not torch.isnan(ws).any()
    ref, _ = launch(dev, xd, yd, cfg)
    for o, r in zip(outs, ref):
        assert torch.equal(o, r)
    with pytest.raises(ValueError, match="workspace"):
        launch(dev, xd, yd, cfg, ws=ws[:-4])


def test_all_zero_input(gpu_device):
    dev = gpu_device
    z = torch.zeros(2, 1184, device=dev)
    for navg in (0, 5):
        (pxx, pyy, pxy, coh), _ = launch(dev, z, z, DET + (navg, "density"))
        assert torch.equal(pxx, torch.zeros_like(pxx)) and torch.equal(pyy, torch.zeros_like(pyy))
        assert torch.equal(pxy, torch.zeros_like(pxy))
        assert torch.isnan(coh).all()


def test_numpy_layer_matches_scipy(gpu_device):
    from specenh import signal

    x, y = signals(3, 9 * 256 + 37)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    kw = dict(fs=FS, window="hann", nperseg=256, noverlap=128, detrend="linear")
    cfg = (256, 128, "hann", "linear", 0, "density")
    _, _, allowed = reference(3, 9 * 256 + 37, cfg)
    for name, args in (("welch", (x,)), ("csd", (x, y)), ("coherence", (x, y))):
        f, P = getattr(signal, name)(*args, **kw)
        fr, Pr = getattr(scipy.signal, name)(*(a.astype(np.float64) for a in args), **kw)
        assert np.array_equal(f, fr) and P.shape == Pr.shape == (3, 129)
        assert P.dtype == Pr.dtype == (np.complex128 if name == "csd" else np.float64)
        if name == "coherence":
            assert float(np.abs(P - Pr).max()) <= allowed
        else:
            assert normwise(P[..., None], Pr[..., None]) <= TOL_PSD
    f, P = signal.welch(x64[0], **kw)  # 1-D in, 1-D out; defaults as scipy's
    assert P.shape == (129,)
    f, P = signal.coherence(x64[:, :2048].reshape(3, 1, 2048), y64[:, :2048].reshape(3, 1, 2048))
    fr, Pr = scipy.signal.coherence(x64[:, :2048].reshape(3, 1, 2048),
                                    y64[:, :2048].reshape(3, 1, 2048))
    assert P.shape == Pr.shape == (3, 1, 129) and np.array_equal(f, fr)


def test_tensor_layer_shapes(gpu_device):
    from specenh import spectral

    x, y = signals(3, 9 * 256 + 37)
    xd, yd = torch.from_numpy(np.array(x)).to(gpu_device), torch.from_numpy(np.array(y)).to(gpu_device)
    f, t, est = spectral.spectral_estimates(xd, yd, fs=FS, nperseg=256, navg=4)
    assert sorted(est) == ["coh", "pxx", "pxy", "pyy"] and t.shape == (4,)
    assert all(v.shape == (3, 129, 4) for v in est.values())
    f, t, est = spectral.spectral_estimates(xd[0], yd[0], fs=FS, nperseg=256, want=("coh",))
    assert list(est) == ["coh"] and est["coh"].shape == (129, 1) and t.shape == (1,)
    f, C = spectral.coherence(xd, yd, fs=FS, nperseg=256)
    fr, Cr = scipy.signal.coherence(x.astype(np.float64), y.astype(np.float64), fs=FS, nperseg=256)
    assert C.shape == (3, 129) and np.array_equal(f, fr)
    assert float(np.abs(C.cpu().numpy() - Cr).max()) <= 5e-5
    f, P = spectral.welch(xd[1], fs=FS, nperseg=256)
    assert P.shape == (129,)


def test_opcheck(gpu_device):
    from specenh import ops

    dev = gpu_device
    x, y = signals(3, 9 * 256 + 37)
    xd, yd = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(y)).to(dev)
    args = (256, 128, "hann", FS, 0, 2)
    op = torch.ops.specenh.spectral_mean.default
    torch.library.opcheck(op, (xd, yd, *args, 4, ALL))
    torch.library.opcheck(op, (xd, None, *args, 0, 1))
    torch.library.opcheck(op, (xd, yd, *args, 0, 8 | 4))
    shape = (3, 129, 4)
    ws = ops.spectral_workspace(xd, *args, 4)
    torch.library.opcheck(torch.ops.specenh.spectral_mean_out.default,
                          (xd, yd, *args, 4, torch.empty(shape, device=dev), None,
                           torch.empty(shape, dtype=torch.complex64, device=dev),
                           torch.empty(shape, device=dev), ws))
