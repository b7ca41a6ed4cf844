"""The two-point wavenumber-frequency spectrum S(k, f) on the GPU (csrc/wavenumber.hip) against
the numpy oracle of tests/wavenumber_local.py run in fp64 on the fp32 samples widened.

Rounding can move a sample across a bin edge, so a histogram is compared row by row
(wavenumber_local.compare / check): a row (b, g, f) is flipped when sum_j |S - S_ref| /
sum_j S_ref > 1e-5; at most max(1, 1 %) of a configuration's rows may be flipped; the
unflipped rows agree to 1e-5 normwise per shot (the project's bound for every averaged
spectrum); in a flipped row the total still agrees to 1e-5 and the moved weight went to a
cyclically adjacent bin. tests/test_wavenumber_cpu.py asserts that the oracle's own float32
run meets the cap. Integer spectra through wavenumber_spectra leave no rounding at all: there
the histogram must equal the oracle bit for bit. Every output buffer is NaN-filled before the
launch. The tests print their measured values (pytest -s); DESIGN.md 5.11 records them.
"""
import numpy as np
import pytest
import torch

import wavenumber_local as wl

pytestmark = pytest.mark.gpu

FS = wl.FS
SCALING = {"density": 0, "spectrum": 1}
DETREND = {False: 0, "constant": 1, "linear": 2}


def upload(dev, *arrs):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrs]


def op_args(cfg):
    n, nov, _, _, _, navg, w, detrend = cfg
    return (n, nov, w, FS, SCALING["density"], DETREND[detrend], navg)


def shape_of(cfg, B=None):
    n, nov, L, nk, b, navg = cfg[:6]
    T = (L - n) // (n - nov) + 1
    return (b if B is None else B, 1 if navg <= 0 else T // navg, n // 2 + 1, nk)


def launch(dev, x, y, cfg, ws=None):
    """torch.ops.specenh.wavenumber_spectrum_out into a NaN-filled buffer."""
    S = torch.full(shape_of(cfg, x.shape[0]), float("nan"), device=dev)
    torch.ops.specenh.wavenumber_spectrum_out(x, y, *op_args(cfg), cfg[3], S, ws)
    return S


@pytest.mark.parametrize("cfg", wl.PARITY, ids=[wl.cfg_id(c) for c in wl.PARITY])
def test_parity_with_the_fp64_oracle(gpu_device, cfg):
    dev = gpu_device
    ref = wl.reference(cfg, np.float64)
    x, y = upload(dev, *wl.signals(cfg[4], cfg[2]))
    S = launch(dev, x, y, cfg)
    assert S.shape == ref.shape and S.dtype == torch.float32
    assert not torch.isnan(S).any() and (S >= 0).all()
    m = wl.compare(S.cpu().numpy(), ref)
    print(f"\n[wavenumber {wl.cfg_id(cfg)}] flipped {m['flipped']} of {m['rows']} (cap "
          f"{m['cap']:.0f}); unflipped {m['unflipped']:.2e} (bound {wl.TOL:.0e}); flipped rows: "
          f"total {m['total']:.2e}, transport / moved weight {m['emd']:.4f}")
    wl.check(m)


def integer_pair(B, T, F, seed):
    """X with integer parts in [-8, 8]; Y = X u s, u one of the eight Gaussian-integer
    directions, s in {1, 2, 3}: conj(X) Y = |X|^2 u s exactly, its phase a multiple of 45
    degrees. Some frames have X = 0 with Y != 0, some both zero."""
    rng = np.random.default_rng(seed)
    X = (rng.integers(-8, 9, (B, T, F)) + 1j * rng.integers(-8, 9, (B, T, F)))
    u = np.array([1, -1, 1j, -1j, 1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j])[rng.integers(0, 8, X.shape)]
    Y = X * u * rng.integers(1, 4, X.shape)
    hole = rng.random(X.shape)
    X[hole < 0.06] = 0
    Y[hole < 0.03] = 0                                  # both zero
    only_y = (hole >= 0.03) & (hole < 0.06)             # X = 0, Y != 0: weight lands in j = K/2
    Y[only_y] = (rng.integers(1, 9, X.shape) - 1j * rng.integers(1, 9, X.shape))[only_y]
    assert (X == 0).sum() > 50 and ((X == 0) & (Y != 0)).sum() > 20
    return X.astype(np.complex64), Y.astype(np.complex64)


@pytest.mark.parametrize("navg", [0, 7])
@pytest.mark.parametrize("nk", [8, 64])
def test_exact_arithmetic_from_spectra(gpu_device, navg, nk):
    """T = 45 (crosses the chunk), F = 70 (crosses a 64-bin tile): every phase is a bin centre
    and every partial sum an integer or half-integer below 2^24, so nothing but the final
    rounding separates the kernel from numpy."""
    from specenh import wavenumber as wn

    dev = gpu_device
    B, T, F = 2, 45, 70
    X, Y = integer_pair(B, T, F, 7)
    glen = navg or T
    ref = np.stack([wl.histogram(
        *(s[:, g * glen:(g + 1) * glen].transpose(0, 2, 1).astype(np.complex128) for s in (X, Y)),
        nk, np.ones(F)) for g in range(T // glen)], axis=1)
    assert ref.shape == (B, T // glen, F, nk) and (ref > 0).sum() > 500
    Xd, Yd = upload(dev, X, Y)
    S = torch.full(ref.shape, float("nan"), device=dev)
    torch.ops.specenh.wavenumber_spectra_out(Xd, Yd, navg, nk, S)
    assert torch.equal(S.cpu(), torch.from_numpy(ref.astype(np.float32)))  # zeros included
    assert torch.equal(wn.wavenumber_spectrum_from_spectra(Xd, Yd, navg=navg, nk=nk), S)
    one = wn.wavenumber_spectrum_from_spectra(Xd[1], Yd[1], navg=navg, nk=nk)
    assert torch.equal(one, S[1])
    # a frame with X = 0 lands in j = K/2 with weight |Y|^2 / 2
    Z = np.zeros((1, 1, 3), np.complex64)
    W = np.array([[[3 - 4j, 0, -2j]]], np.complex64)
    got = wn.wavenumber_spectrum_from_spectra(*upload(dev, Z, W), nk=nk).cpu().numpy()
    want = np.zeros((1, 1, 3, nk), np.float32)
    want[0, 0, :, nk // 2] = [12.5, 0, 2]
    assert np.array_equal(got, want)


MID = wl.PARITY[3]  # 128 / 96 / 4096, nk = 64, navg = 7: T = 125, G = 17


def test_invariant_row_sums_are_the_mean_welch_spectrum(gpu_device):
    from specenh import spectral
    from specenh import wavenumber as wn

    dev = gpu_device
    for cfg in (MID, wl.PARITY[5], wl.PARITY[6]):
        n, nov, L, nk, B, navg, w, detrend = cfg
        x, y = upload(dev, *wl.signals(B, L))
        kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, navg=navg)
        f, k, t, S = wn.wavenumber_spectrum(x, y, nk=nk, dx=0.02, **kw)
        f2, t2, est = spectral.spectral_estimates(x, y, want=("pxx", "pyy"), **kw)
        assert np.array_equal(f, f2) and np.array_equal(t, t2)
        want = ((est["pxx"].double() + est["pyy"].double()) / 2).transpose(1, 2)  # [B, G, F]
        got = S.double().sum(-1)
        err = float(((got - want).abs().amax(dim=(1, 2)) / want.amax(dim=(1, 2))).max())
        print(f"\n[wavenumber invariant {wl.cfg_id(cfg)}] sum_j S against (pxx + pyy) / 2: "
              f"{err:.2e} (bound {wl.TOL:.0e})")
        assert err <= wl.TOL


def test_aliasing_puts_all_weight_at_zero_phase(gpu_device):
    from specenh import ops

    dev = gpu_device
    x, y = upload(dev, *wl.signals(MID[4], MID[2]))
    nk = MID[3]
    S = launch(dev, x, x, MID)
    rest = torch.cat([S[..., :nk // 2], S[..., nk // 2 + 1:]], dim=-1)
    assert not torch.isnan(S).any() and not rest.any() and (S[..., nk // 2] > 0).all()
    one = ops.wavenumber_workspace(x, x, *op_args(MID)).numel()
    two = ops.wavenumber_workspace(x, y, *op_args(MID)).numel()
    assert one == 3 * 17 * 7 * 65 * 8 and two == 2 * one
    assert ops.wavenumber_workspace(x, x.clone(), *op_args(MID)).numel() == two
    # the same samples under another tensor: two signals, the same values
    assert torch.equal(launch(dev, x, x.clone(), MID), S)


@pytest.mark.parametrize("cfg", [wl.PARITY[1], wl.PARITY[4]], ids=["navg0-nk64", "navg7-nk256"])
def test_batch_stride_and_split_independence(gpu_device, cfg, monkeypatch):
    from specenh import wavenumber as wn

    dev = gpu_device
    n, nov, L, nk, _, navg, w, detrend = cfg
    x, y = upload(dev, *wl.signals(5, L))
    full = launch(dev, x, y, cfg)
    assert not torch.isnan(full).any()
    for b in range(5):  # a batch of 5 = five batches of 1, bitwise
        assert torch.equal(launch(dev, x[b:b + 1], y[b:b + 1], cfg)[0], full[b])
    assert torch.equal(launch(dev, x[3:], y[3:], cfg), full[3:])  # batch position
    wide = [torch.zeros(5, L + 100 + 28 * i, device=dev) for i in range(2)]
    for wd, s in zip(wide, (x, y)):
        wd[:, :L] = s
    assert torch.equal(launch(dev, wide[0][:, :L], wide[1][:, :L], cfg), full)  # row strides
    kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, navg=navg, nk=nk)
    S = wn.wavenumber_spectrum(x, y, **kw)[3]
    assert torch.equal(S, full)
    T = (L - n) // (n - nov) + 1
    with monkeypatch.context() as mp:  # launches of two shots
        mp.setattr(wn, "CSM_WORKSPACE_CAP", 2 * 8 * 2 * (T // (navg or T)) * (navg or T) * 65)
        split = wn.wavenumber_spectrum(x, y, **kw)[3]
    assert torch.equal(split, full)


def test_workspace_is_fully_written(gpu_device):
    from specenh import ops

    dev = gpu_device
    x, y = upload(dev, *wl.signals(MID[4], MID[2]))
    for sig, nsig in (((x, x), 1), ((x, y), 2)):
        need = ops.wavenumber_workspace(*sig, *op_args(MID)).numel()
        assert need == 3 * nsig * 119 * 65 * 8  # 17 groups of 7, six frames dropped
        ws = torch.full((need // 4,), float("nan"), device=dev)
        S = launch(dev, *sig, MID, ws=ws)
        assert not torch.isnan(ws).any()
        assert torch.equal(S, launch(dev, *sig, MID))
        with pytest.raises(ValueError, match="workspace"):
            launch(dev, *sig, MID, ws=ws.view(torch.uint8)[:-1])


def test_all_zero_input(gpu_device):
    dev = gpu_device
    zero = torch.zeros(2, 4096, device=dev)
    for cfg in (MID, wl.PARITY[1]):
        for sig in ((zero, zero), (zero, torch.zeros_like(zero))):
            S = launch(dev, *sig, cfg)
            assert torch.equal(S, torch.zeros_like(S))


def test_delayed_pair_ridge_and_dispersion(gpu_device):
    """The recipe of tests/test_wavenumber_cpu.py on the GPU. The ridge follows the delay on
    every bin but DC and Nyquist. dispersion is a linear, not a circular, moment: it is checked
    where the true phase keeps two bin widths away from +-pi, so that the ridge's skirts do not
    wrap to the other end of the k axis."""
    from specenh import wavenumber as wn

    dev = gpu_device
    x, y = upload(dev, *wl.delayed_pair())
    K, dx = wl.DELAY["nk"], 0.015
    f, k, t, S = wn.wavenumber_spectrum(x, y, dx=dx, **wl.DELAY)
    assert S.shape == (1, 65, K) and k.shape == (K,) and t.shape == (1,)
    S = S[0]
    theta = wl.delay_phase()
    want = wl.phase_bin(theta, K)
    bins = np.arange(1, 64)
    ridge = S.argmax(-1).cpu().numpy()
    assert np.array_equal(ridge[bins], want[bins])
    kbar, sigma = wn.dispersion(S, k)
    assert kbar.device == S.device and kbar.dtype == torch.float64 and kbar.shape == (65,)
    wrapped = np.angle(np.exp(1j * theta))
    width = 2 * np.pi / K
    inner = bins[np.abs(wrapped[bins]) <= np.pi - 2 * width]
    assert inner.size >= 50
    # -2 pi f d / (fs dx), wrapped onto the k axis
    err = np.abs(kbar.cpu().numpy()[inner] - wrapped[inner] / dx)
    print(f"\n[wavenumber delayed pair] ridge exact on {bins.size} bins; |kbar - k_true| max "
          f"{err.max() * dx / width:.3f} bin widths on {inner.size} bins; sigma_k max "
          f"{float(sigma[inner].max()) * dx / width:.3f} bin widths")
    assert err.max() <= width / dx
    np.testing.assert_array_equal(k, wl.k_grid(K, dx))


def test_tensor_and_numpy_layers(gpu_device):
    from specenh import signal, stft
    from specenh import wavenumber as wn

    dev = gpu_device
    n, nov, L, nk, B, navg, w, detrend = MID
    x, y = wl.signals(B, L)
    xd, yd = upload(dev, x, y)
    kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, navg=navg, nk=nk)
    f, k, t, S = wn.wavenumber_spectrum(xd, yd, dx=0.5, **kw)
    assert np.array_equal(f, stft.frequencies(n, FS)) and t.shape == (17,)
    assert np.array_equal(k, wl.k_grid(nk, 0.5))
    assert S.shape == (B, 17, 65, nk) and S.dtype == torch.float32
    assert torch.equal(S, launch(dev, xd, yd, MID))
    one = wn.wavenumber_spectrum(xd[1], yd[1], **kw)[3]  # 1-D in drops B
    assert torch.equal(one, S[1])
    # float64 and strided input are converted, the values those of the fp32 copy
    assert torch.equal(wn.wavenumber_spectrum(xd.double(), yd.double(), **kw)[3], S)
    # numpy layer: leading axes flattened into the batch and restored, fp64 out
    f, k, t, N = signal.wavenumber_spectrum(x.reshape(B, 1, -1), y.reshape(B, 1, -1), dx=0.5, **kw)
    assert N.shape == (B, 1, 17, 65, nk) and N.dtype == np.float64 and k.shape == (nk,)
    assert np.array_equal(N[:, 0], S.cpu().numpy().astype(np.float64))
    N1 = signal.wavenumber_spectrum(x[0].astype(np.float64), y[0].astype(np.float64), **kw)[3]
    assert np.array_equal(N1, N[0, 0])
    # spectrum scaling: the same histogram, rescaled rows
    P = wn.wavenumber_spectrum(xd, yd, scaling="spectrum", **kw)[3]
    assert P.shape == S.shape and torch.equal(P > 0, S > 0)


def test_opcheck(gpu_device):
    from specenh import ops

    dev = gpu_device
    x, y = upload(dev, *wl.signals(MID[4], MID[2]))
    args = op_args(MID)
    op = torch.ops.specenh.wavenumber_spectrum.default
    torch.library.opcheck(op, (x, y, *args, 64))
    torch.library.opcheck(op, (x, x, *args[:-1], 0, 8))
    ws = ops.wavenumber_workspace(x, y, *args)
    torch.library.opcheck(torch.ops.specenh.wavenumber_spectrum_out.default,
                          (x, y, *args, 64, torch.empty(3, 17, 65, 64, device=dev), ws))
    torch.library.opcheck(torch.ops.specenh.wavenumber_spectrum_out.default,
                          (x, y, *args, 16, torch.empty(3, 17, 65, 16, device=dev), None))
    X, Y = upload(dev, *integer_pair(2, 45, 70, 7))
    torch.library.opcheck(torch.ops.specenh.wavenumber_spectra.default, (X, Y, 0, 8))
    torch.library.opcheck(torch.ops.specenh.wavenumber_spectra.default, (X, Y, 7, 256))
    torch.library.opcheck(torch.ops.specenh.wavenumber_spectra_out.default,
                          (X, Y, 7, 8, torch.empty(2, 6, 70, 8, device=dev)))


def test_graph_capture(gpu_device):
    """Both entry points launch without allocating, so a captured single-stream graph replays
    them: the replay on new samples equals the eager call bit for bit."""
    from specenh import ops

    dev = gpu_device
    x, y = upload(dev, *wl.signals(MID[4], MID[2]))
    ws = ops.wavenumber_workspace(x, y, *op_args(MID))
    eager = launch(dev, x, y, MID, ws=ws)
    X, Y = upload(dev, *integer_pair(2, 45, 70, 7))
    eager_s = torch.full((2, 6, 70, 256), float("nan"), device=dev)
    torch.ops.specenh.wavenumber_spectra_out(X, Y, 7, 256, eager_s)
    xs, ys, Xs, Ys = (torch.zeros_like(v) for v in (x, y, X, Y))
    out = torch.full_like(eager, float("nan"))
    out_s = torch.full_like(eager_s, float("nan"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        torch.ops.specenh.wavenumber_spectrum_out(xs, ys, *op_args(MID), MID[3], out, ws)
        torch.ops.specenh.wavenumber_spectra_out(Xs, Ys, 7, 256, out_s)
    xs.copy_(x), ys.copy_(y), Xs.copy_(X), Ys.copy_(Y)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(out_s, eager_s)
