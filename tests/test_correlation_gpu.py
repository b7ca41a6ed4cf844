"""The block-averaged cross-correlation on the GPU (csrc/correlation.hip) against the float64
direct-sum restatement of tests/correlation_local.py on the fp32 samples widened.

The error of an FFT correlation scales with the signals' energies, so it is measured on the
coefficient scale (correlation_local.compare): for every row (b, g),
max_m |R - R_ref| / sqrt(Ex_ref Ey_ref) <= 1e-5, the project's bound for every averaged
spectrum; tests/test_correlation_cpu.py asserts that a float32 run of the same formulation
meets it. Every output buffer is NaN-filled before the launch. The tests print their measured
values (pytest -s); DESIGN.md 5.12 records them.
"""
import numpy as np
import pytest
import scipy.signal
import torch

import correlation_local as cl

pytestmark = pytest.mark.gpu

FS = cl.FS
DETREND = {False: 0, "constant": 1, "linear": 2}
RAW, COEFF = 0, 1


def upload(dev, *arrs):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrs]


def op_args(cfg):
    n, nov, _, M, _, navg, w, detrend = cfg
    return (n, nov, w, FS, 0, DETREND[detrend], navg, M)


def launch(dev, x, y, cfg, mode, ws=None):
    """torch.ops.specenh.correlation_out into NaN-filled buffers: (out, energies)."""
    shape = cl.shape_of(cfg, x.shape[0])
    out = torch.full(shape, float("nan"), device=dev)
    en = torch.full(shape[:2] + (2,), float("nan"), device=dev)
    torch.ops.specenh.correlation_out(x, y, *op_args(cfg), mode, out, en, ws)
    return out, en


@pytest.mark.parametrize("cfg", cl.PARITY, ids=[cl.cfg_id(c) for c in cl.PARITY])
def test_parity_with_the_fp64_restatement(gpu_device, cfg):
    dev = gpu_device
    ref = cl.reference(cfg)
    x, y = upload(dev, *cl.signals(cfg[4], cfg[2]))
    scale = np.sqrt(ref["Ex"] * ref["Ey"])
    R, en = launch(dev, x, y, cfg, RAW)
    rho, en2 = launch(dev, x, y, cfg, COEFF)
    assert R.shape == ref["R"].shape and R.dtype == torch.float32
    assert not torch.isnan(R).any() and not torch.isnan(rho).any() and not torch.isnan(en).any()
    assert torch.equal(en, en2)
    e_raw = cl.compare(R.cpu().numpy(), ref["R"], scale)
    e_rho = cl.compare(rho.cpu().numpy(), cl.coefficient(ref), 1.0)
    want = np.stack([ref["Ex"], ref["Ey"]], axis=-1)
    e_en = float((np.abs(en.cpu().numpy().astype(np.float64) - want) / want).max())
    print(f"\n[correlation {cl.cfg_id(cfg)}] max |R - R_ref| / sqrt(Ex Ey): raw {e_raw:.2e}, "
          f"coeff {e_rho:.2e} (bound {cl.TOL:.0e}); energies {e_en:.2e} relative (bound 1e-05); "
          f"max |rho| {float(rho.abs().max()):.4f}")
    assert e_raw <= cl.TOL and e_rho <= cl.TOL
    assert e_en <= 1e-5
    assert float(rho.abs().max()) <= 1.0 + cl.TOL


AUTO = [cl.PARITY[1], cl.PARITY[2], cl.PARITY[5]]  # chunk records folded; blocks; N = 2048


@pytest.mark.parametrize("cfg", AUTO, ids=[cl.cfg_id(c) for c in AUTO])
def test_autocorrelation(gpu_device, cfg):
    """y the same tensor: loaded and transformed once. Lag 0 of the coefficient is 1, the
    function is even, it is that of the restatement, and a copy of x (two signals, the same
    samples) gives the same values within the bound."""
    dev = gpu_device
    M = cfg[3]
    ref = cl.reference(cfg, auto=True)
    x, = upload(dev, cl.signals(cfg[4], cfg[2])[0])
    R, en = launch(dev, x, x, cfg, RAW)
    rho, _ = launch(dev, x, x, cfg, COEFF)
    assert not torch.isnan(R).any() and not torch.isnan(rho).any()
    assert torch.equal(en[..., 0], en[..., 1])
    lag0 = float((rho[..., M] - 1).abs().max())
    Rn = R.cpu().numpy().astype(np.float64)
    even = float((np.abs(Rn - Rn[..., ::-1]).max(-1) / ref["Ex"]).max())
    e_ref = cl.compare(Rn, ref["R"], ref["Ex"])
    Rc, enc = launch(dev, x, x.clone(), cfg, RAW)
    e_copy = cl.compare(Rc.cpu().numpy(), Rn, ref["Ex"])
    print(f"\n[correlation auto {cl.cfg_id(cfg)}] |rho[0] - 1| {lag0:.2e} (bound 1e-06); "
          f"|R[m] - R[-m]| / Ex {even:.2e}; against the restatement {e_ref:.2e}; a copy of x "
          f"against the aliased call {e_copy:.2e} (bound {cl.TOL:.0e})")
    assert lag0 <= 1e-6
    assert even <= cl.TOL and e_ref <= cl.TOL and e_copy <= cl.TOL
    assert torch.equal(enc, en)  # the energies are taken in the time domain, signal by signal


def test_constant_signal_has_zero_coefficient(gpu_device):
    """A constant is removed exactly by the constant detrend: Ex == 0, and rho is defined as 0
    there (no 0/0)."""
    dev = gpu_device
    cfg = cl.PARITY[2]
    _, y = upload(dev, *cl.signals(cfg[4], cfg[2]))
    const = torch.full_like(y, 3.5)
    for sig in ((const, y), (y, const), (const, const), (const, const.clone())):
        rho, en = launch(dev, *sig, cfg, COEFF)
        R, _ = launch(dev, *sig, cfg, RAW)
        assert torch.equal(rho, torch.zeros_like(rho)) and torch.equal(R, torch.zeros_like(R))
        assert (en[..., 0] == 0).all() or (en[..., 1] == 0).all()


@pytest.mark.parametrize("d", cl.DELAYS)
def test_delayed_pair_time_delay(gpu_device, d):
    """y[n] = x[n - d] + 1 % noise, white x, boxcar 256 / 128 in blocks of 8 frames: in every
    group time_delay on the GPU result is within 1e-3 samples of what it gives on the float64
    restatement, and that is within 0.5 samples of d."""
    from specenh import correlation as co

    dev = gpu_device
    x, y = cl.delayed_pair(d)
    ref = cl.correlation(x, y, maxlag=cl.DELAY_MAXLAG, **cl.DELAY)
    lags_s, t, rho = co.correlate(*upload(dev, x, y), maxlag=cl.DELAY_MAXLAG, fs=1.0, **cl.DELAY)
    assert rho.shape == (4, 2 * cl.DELAY_MAXLAG + 1) and t.shape == (4,)
    assert np.array_equal(lags_s, np.arange(-cl.DELAY_MAXLAG, cl.DELAY_MAXLAG + 1))
    tau, peak = co.time_delay(rho, lags_s)
    tau_ref, peak_ref = co.time_delay(torch.from_numpy(cl.coefficient(ref)[0]), lags_s)
    assert tau.device == rho.device and tau.dtype == torch.float64 and tau.shape == (4,)
    e_gpu = float((tau.cpu() - tau_ref).abs().max())
    e_ref = float((tau_ref - d).abs().max())
    print(f"\n[correlation delayed pair d = {d}] tau per group {tau.cpu().numpy().round(4)}; "
          f"|tau - tau_ref| max {e_gpu:.2e} samples (bound 1e-03); |tau_ref - d| max "
          f"{e_ref:.3f} (bound 0.5); peak {float(peak.min()):.4f} .. {float(peak.max()):.4f}")
    assert e_gpu <= 1e-3
    assert e_ref <= 0.5


WHOLE, BLOCKS = cl.PARITY[1], cl.PARITY[2]  # 128 / 96 / 4096: T = 125 in chunks; G = 17 of 7


@pytest.mark.parametrize("cfg", [WHOLE, BLOCKS], ids=["navg0-chunks", "navg7"])
@pytest.mark.parametrize("mode", [RAW, COEFF], ids=["raw", "coeff"])
def test_batch_stride_and_split_independence(gpu_device, cfg, mode, monkeypatch):
    from specenh import correlation as co

    dev = gpu_device
    n, nov, L, M, _, navg, w, detrend = cfg
    x, y = upload(dev, *cl.signals(5, L))
    full, en = launch(dev, x, y, cfg, mode)
    assert not torch.isnan(full).any() and not torch.isnan(en).any()
    for b in range(5):  # a batch of 5 = five batches of 1, bitwise
        one, e1 = launch(dev, x[b:b + 1], y[b:b + 1], cfg, mode)
        assert torch.equal(one[0], full[b]) and torch.equal(e1[0], en[b])
    tail, et = launch(dev, x[3:], y[3:], cfg, mode)  # batch position
    assert torch.equal(tail, full[3:]) and torch.equal(et, en[3:])
    wide = [torch.zeros(5, L + 100 + 28 * i, device=dev) for i in range(2)]
    for wd, s in zip(wide, (x, y)):
        wd[:, :L] = s
    ws_, es_ = launch(dev, wide[0][:, :L], wide[1][:, :L], cfg, mode)  # strides beyond the length
    assert torch.equal(ws_, full) and torch.equal(es_, en)
    kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, navg=navg, maxlag=M,
              normalize="coeff" if mode == COEFF else "raw")
    assert torch.equal(co.correlate(x, y, **kw)[2], full)
    T = (L - n) // (n - nov) + 1
    glen = navg or T
    ncg = -(-glen // 32)
    with monkeypatch.context() as mp:  # launches of two shots (navg = 7 needs no workspace:
        # there the split has nothing to cut and the call is one launch)
        mp.setattr(co, "CSM_WORKSPACE_CAP", 2 * 8 * (n + 3) * (T // glen) * ncg)
        split = co.correlate(x, y, **kw)[2]
    assert torch.equal(split, full)


def test_workspace_size_and_use(gpu_device):
    from specenh import ops

    dev = gpu_device
    x, y = upload(dev, *cl.signals(WHOLE[4], WHOLE[2]))
    need = ops.correlation_workspace(x, y, *op_args(WHOLE)).numel()
    assert need == 3 * 4 * (128 + 3) * 8  # T = 125: four chunks a shot
    assert ops.correlation_workspace(x, y, *op_args(BLOCKS)).numel() == 1  # none needed
    ws = torch.full((need // 4,), float("nan"), device=dev)
    R, _ = launch(dev, x, y, WHOLE, RAW, ws=ws)
    assert not torch.isnan(ws).any()  # every record is written
    assert torch.equal(R, launch(dev, x, y, WHOLE, RAW)[0])
    with pytest.raises(ValueError, match="workspace"):
        launch(dev, x, y, WHOLE, RAW, ws=ws.view(torch.uint8)[:-1])
    # no energies requested
    out = torch.full(cl.shape_of(WHOLE), float("nan"), device=dev)
    torch.ops.specenh.correlation_out(x, y, *op_args(WHOLE), RAW, out, None, ws)
    assert torch.equal(out, R)


def test_graph_capture(gpu_device):
    """The entry point launches without allocating, so a captured single-stream graph replays
    it: the replay on new samples equals the eager call bit for bit."""
    from specenh import ops

    dev = gpu_device
    x, y = upload(dev, *cl.signals(WHOLE[4], WHOLE[2]))
    ws = ops.correlation_workspace(x, y, *op_args(WHOLE))
    eager, een = launch(dev, x, y, WHOLE, COEFF, ws=ws)
    eager_b, _ = launch(dev, x, y, BLOCKS, RAW)
    xs, ys = torch.zeros_like(x), torch.zeros_like(y)
    out, en = torch.full_like(eager, float("nan")), torch.full_like(een, float("nan"))
    out_b = torch.full_like(eager_b, float("nan"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        torch.ops.specenh.correlation_out(xs, ys, *op_args(WHOLE), COEFF, out, en, ws)
        torch.ops.specenh.correlation_out(xs, ys, *op_args(BLOCKS), RAW, out_b, None, None)
    xs.copy_(x), ys.copy_(y)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(en, een) and torch.equal(out_b, eager_b)


def test_tensor_and_numpy_layers(gpu_device):
    from specenh import correlation as co
    from specenh import signal, spectral

    dev = gpu_device
    n, nov, L, M, B, navg, w, detrend = BLOCKS
    x, y = cl.signals(B, L)
    xd, yd = upload(dev, x, y)
    kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, navg=navg, maxlag=M)
    lags, t, rho = co.correlate(xd, yd, **kw)
    assert np.array_equal(lags, np.arange(-M, M + 1) / FS)
    assert np.array_equal(t, spectral.group_times(L, n, nov, FS, navg)) and t.shape == (17,)
    assert rho.shape == (B, 17, 2 * M + 1) and rho.dtype == torch.float32
    assert torch.equal(rho, launch(dev, xd, yd, BLOCKS, COEFF)[0])
    raw = co.correlate(xd, yd, normalize="raw", **kw)[2]
    assert torch.equal(raw, launch(dev, xd, yd, BLOCKS, RAW)[0])
    assert torch.equal(co.correlate(xd[1], yd[1], **kw)[2], rho[1])  # 1-D in drops B
    assert torch.equal(co.correlate(xd.double(), yd.double(), **kw)[2], rho)
    assert torch.equal(co.autocorrelate(xd, **kw)[2], launch(dev, xd, xd, BLOCKS, COEFF)[0])
    # maxlag None: every lag; the inner lags are those of the short call
    every = co.correlate(xd, yd, **dict(kw, maxlag=None))[2]
    assert every.shape == (B, 17, 2 * n - 1)
    assert torch.equal(every[..., n - 1 - M:n + M], rho)
    # unbiased: divided by the window's lag product (raw), by c[m] / c[0] (coeff)
    c = torch.as_tensor(co.window_lag_product(w, n, M), device=dev)
    ub = co.correlate(xd, yd, normalize="raw", unbiased=True, **kw)[2]
    assert torch.equal(ub, (raw.double() / c).float())
    ubc = co.correlate(xd, yd, unbiased=True, **kw)[2]
    assert torch.equal(ubc, (rho.double() / (c / c[M])).float())
    # the correlation time of the GPU auto-correlation is that of the restatement's
    ac = co.autocorrelate(xd, **kw)[2]
    ref = cl.coefficient(cl.reference(BLOCKS, auto=True))
    tc, tc_ref = co.correlation_time(ac, lags), co.correlation_time(torch.from_numpy(ref), lags)
    assert tc.shape == (B, 17) and torch.equal(torch.isnan(tc).cpu(), torch.isnan(tc_ref))
    assert not torch.isnan(tc_ref).all()
    assert float(torch.nan_to_num((tc.cpu() - tc_ref) * FS).abs().max()) <= 1e-3  # in samples
    # numpy layer: leading axes flattened into the batch and restored, fp64 out
    lg, tn, N = signal.correlate(x.reshape(B, 1, -1), y.reshape(B, 1, -1), **kw)
    assert N.shape == (B, 1, 17, 2 * M + 1) and N.dtype == np.float64
    assert np.array_equal(lg, lags) and np.array_equal(tn, t)
    assert np.array_equal(N[:, 0], rho.cpu().numpy().astype(np.float64))


def test_numpy_layer_against_scipy_correlate(gpu_device):
    """One frame, no detrend, boxcar: specenh.signal.correlate is scipy.signal.correlate(y, x)
    on scipy's own lag axis."""
    from specenh import signal

    rng = np.random.default_rng(12)
    N = 512
    x = rng.standard_normal(N)
    y = 0.8 * np.roll(x, 6) + 0.6 * rng.standard_normal(N) + 0.25
    lags, t, R = signal.correlate(x, y, window="boxcar", nperseg=N, noverlap=0, detrend=False,
                                  normalize="raw", fs=2.0)
    assert R.shape == (1, 2 * N - 1) and R.dtype == np.float64 and t.shape == (1,)
    x32, y32 = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    want = scipy.signal.correlate(y32, x32, "full", method="direct")
    assert np.array_equal(lags, scipy.signal.correlation_lags(N, N, "full") / 2.0)
    err = np.abs(R[0] - want).max() / np.sqrt((x32 ** 2).sum() * (y32 ** 2).sum())
    print(f"\n[correlation numpy layer] against scipy.signal.correlate: {err:.2e} on the "
          f"coefficient scale (bound {cl.TOL:.0e}); peak at lag {lags[np.argmax(R[0])] * 2.0:.0f}")
    assert err <= cl.TOL
    assert lags[np.argmax(R[0])] * 2.0 == 6


def test_opcheck(gpu_device):
    from specenh import ops

    dev = gpu_device
    x, y = upload(dev, *cl.signals(WHOLE[4], WHOLE[2]))
    op = torch.ops.specenh.correlation.default
    torch.library.opcheck(op, (x, y, *op_args(WHOLE), COEFF))
    torch.library.opcheck(op, (x, x, *op_args(BLOCKS), RAW))
    ws = ops.correlation_workspace(x, y, *op_args(WHOLE))
    out_op = torch.ops.specenh.correlation_out.default
    torch.library.opcheck(out_op, (x, y, *op_args(WHOLE), RAW,
                                   torch.empty(cl.shape_of(WHOLE), device=dev),
                                   torch.empty(3, 1, 2, device=dev), ws))
    torch.library.opcheck(out_op, (x, y, *op_args(BLOCKS), COEFF,
                                   torch.empty(cl.shape_of(BLOCKS), device=dev), None, None))
