"""The cross-spectral matrix of a channel array on the GPU (csrc/spectral_matrix.hip) against
scipy.signal.csd broadcast over all channel pairs, in fp64 on the fp32 samples widened. Group
g of a block-averaged call is scipy on the slice x[g navg hop : g navg hop + (navg - 1) hop +
nperseg].

Bounds (the project's, as tests/test_spectral_gpu.py). csm: 1e-5 normwise per (shot, group,
i, j), max_f |got - ref| / max_f |ref|. Coherence: max abs error against fp64, allowed
max(4 x scipy's own float32 error on the same inputs, 2e-6), capped at 5e-5. Every output and
the workspace are NaN-filled before the launch, so an element the kernels do not write fails
the comparison. Each test prints its measured and allowed values (pytest -s); DESIGN.md 5.8
records them.
"""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

pytestmark = pytest.mark.gpu

FS = 5e5
TOL_CSM = 1e-5
SCALING = {"density": 0, "spectrum": 1}
DETREND = {False: 0, "constant": 1, "linear": 2}
BOTH = 3

# (C, nperseg, noverlap, window, detrend, navg, scaling); L = 9 nperseg + 37, B = 2
PARITY = [
    (2, 256, 128, "hann", "constant", 0, "density"),
    (3, 64, 48, "hann", "linear", 0, "density"),       # T = 35: two chunks
    (5, 256, 128, "hann", "linear", 2, "spectrum"),    # G = 8, one frame dropped
    (16, 512, 256, "hamm", "linear", 4, "density"),
    (17, 64, 48, "hann", "linear", 5, "density"),      # 2C = 34 crosses a 32-wide tile
    (33, 256, 128, "hamm", "constant", 0, "density"),  # C crosses the tile
    (64, 1024, 768, "hamm", "linear", 1, "density"),   # the maximum C, groups of one frame
    (5, 4096, 3072, "hann", False, 3, "density"),
    (9, 128, 96, "hann", "linear", 0, "density"),      # 8 + 1 channels: a ragged second block
    (5, 2048, 1536, "hann", "linear", 0, "density"),   # 4 slots: blocks of 4 + 1
    (6, 2048, 1024, "hamm", False, 2, "spectrum"),     # 4 slots with frame groups
]
LONG = [(3, 64, 48, "hann", "linear", 0, "density"),   # T = 4101: 129 chunks
        (3, 64, 48, "hann", "linear", 7, "density")]   # G = 585, 6 frames dropped
L_LONG = 65664
MID = (5, 256, 128, "hann", "linear", 2, "density")
L_MID = 9 * 256 + 37


def _id(c):
    return "-".join(str(v) for v in c)


@functools.lru_cache(maxsize=None)
def signals(B, C, L):
    """x_c = (0.4 + 0.6 ((7c) mod C) / C) roll(base, 3c) + 0.5 noise_c, fp64 recipe cast to
    fp32; shot b takes the seeds 11 + b and 111 + 1000 b."""
    from specenh.synthetic import plasma_chirps

    x = np.empty((B, C, L), dtype=np.float64)
    for b in range(B):
        base = plasma_chirps(1, L, seed0=11 + b, dtype=np.float64)[0]
        noise = plasma_chirps(C, L, seed0=111 + 1000 * b, dtype=np.float64)
        for c in range(C):
            x[b, c] = (0.4 + 0.6 * ((7 * c) % C) / C) * np.roll(base, 3 * c) + 0.5 * noise[c]
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def scipy_groups(x, cfg, dtype):
    """csm [B, F, G, C, C] and coh from scipy on each group's slice, computed in `dtype`."""
    _, n, nov, w, detrend, navg, scaling = cfg
    hop = n - nov
    x = x.astype(dtype)
    T = (x.shape[-1] - n) // hop + 1
    glen = navg if navg >= 1 else T
    kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, scaling=scaling)
    S = []
    for g in range(T // glen):
        s = x[..., g * glen * hop: g * glen * hop + (glen - 1) * hop + n]
        _, p = scipy.signal.csd(s[:, :, None, :], s[:, None, :, :], **kw)  # [B, C, C, F]
        S.append(np.moveaxis(p, -1, 1))
    S = np.stack(S, axis=2)  # [B, F, G, C, C]
    d = np.real(np.diagonal(S, axis1=-2, axis2=-1))
    coh = np.abs(S) ** 2 / d[..., :, None] / d[..., None, :]
    return S, coh


@functools.lru_cache(maxsize=None)
def reference(B, L, cfg):
    """The fp64 truth, and the coherence error allowed: from scipy's own float32 run."""
    x = signals(B, cfg[0], L)
    with np.errstate(invalid="ignore", divide="ignore"):
        S, coh = scipy_groups(x, cfg, np.float64)
        S32, coh32 = scipy_groups(x, cfg, np.float32)
    assert S32.dtype == np.complex64  # scipy really ran in float32
    err32 = float(np.abs(coh32.astype(np.float64) - coh).max())
    allowed = min(max(4.0 * err32, 2e-6), 5e-5)
    S.setflags(write=False)
    coh.setflags(write=False)
    return S, coh, err32, allowed


def op_args(cfg):
    _, n, nov, w, detrend, navg, scaling = cfg
    return (n, nov, w, FS, SCALING[scaling], DETREND[detrend], navg)


def launch(dev, x, cfg, mask=BOTH, ws=None):
    """torch.ops.specenh.csm_out into NaN-filled buffers and a NaN-filled workspace; returns
    (csm, coh) (None where not asked for) and the workspace."""
    from specenh import ops

    _, n, nov, _, _, navg, _ = cfg
    B, C, L = x.shape
    T = (L - n) // (n - nov) + 1
    shape = (B, n // 2 + 1, 1 if navg <= 0 else T // navg, C, C)
    nan = float("nan")
    csm = torch.full(shape, complex(nan, nan), dtype=torch.complex64, device=dev) \
        if mask & 1 else None
    coh = torch.full(shape, nan, dtype=torch.float32, device=dev) if mask & 2 else None
    if ws is None:
        ws = ops.csm_workspace(x, *op_args(cfg))
        ws.view(torch.float32).fill_(nan)
    ops.ops.csm_out(x, *op_args(cfg), csm, coh, ws)
    return (csm, coh), ws


def normwise(got, ref):
    """max over (shot, group, i, j) of max_f |got - ref| / max_f |ref|; [B, F, G, C, C]."""
    num = np.abs(got - ref).max(axis=1)
    den = np.abs(ref).max(axis=1)
    return float((num / den).max())


def upload(dev, x):
    return torch.from_numpy(np.array(x)).to(dev)


def check_case(dev, B, L, cfg, label):
    S, coh, err32, allowed = reference(B, L, cfg)
    (gs, gc), ws = launch(dev, upload(dev, signals(B, cfg[0], L)), cfg)
    assert not torch.isnan(ws.view(torch.float32)).any()  # the workspace is fully written
    gs, gc = gs.cpu().numpy(), gc.cpu().numpy()
    assert gs.dtype == np.complex64 and gs.shape == S.shape and gc.shape == coh.shape
    err = normwise(gs.astype(np.complex128), S)
    cerr = float(np.abs(gc.astype(np.float64) - coh).max())
    C = cfg[0]
    off = coh[..., ~np.eye(C, dtype=bool)]
    print(f"\n[csm {label}] csm {err:.2e} (bound {TOL_CSM:.0e}); coherence {cerr:.2e} allowed "
          f"{allowed:.2e} (scipy float32 {err32:.2e}); off-diagonal coherence "
          f"{off.min():.1e}..{off.max():.3f}")
    assert err <= TOL_CSM
    assert cerr <= allowed
    return gs, gc


@pytest.mark.parametrize("cfg", PARITY, ids=[_id(c) for c in PARITY])
def test_parity_with_scipy(gpu_device, cfg):
    C, n, nov = cfg[:3]
    L = 9 * n + 37
    gs, _ = check_case(gpu_device, 2, L, cfg, _id(cfg))
    T = (L - n) // (n - nov) + 1
    assert gs.shape == (2, n // 2 + 1, 1 if cfg[5] <= 0 else T // cfg[5], C, C)


@pytest.mark.parametrize("cfg", LONG, ids=[_id(c) for c in LONG])
def test_long_reduction(gpu_device, cfg):
    from specenh import spectral

    T = (L_LONG - 64) // 16 + 1
    assert T == 4101 and T > spectral.CHUNK_FRAMES
    check_case(gpu_device, 2, L_LONG, cfg, "long " + _id(cfg))


@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("L,navg", [(256, 0), (256, 1), (384, 0), (384, 2), (384, 1),
                                    (9 * 256 + 37, 17), (9 * 256 + 37, 1)])
def test_edge_shapes(gpu_device, C, L, navg):
    cfg = (C, 256, 128, "hann", "constant", navg, "density")
    _, gc = check_case(gpu_device, 2, L, cfg, f"edge C={C} L={L} navg={navg}")
    T = (L - 256) // 128 + 1
    if navg == 1 or T == 1:  # one frame a group: every coherence is 1
        _, _, _, allowed = reference(2, L, cfg)
        assert float(np.abs(gc - 1.0).max()) <= allowed


def test_consistency_with_pair_form(gpu_device):
    """csm[..., i, j] is spectral_mean's pxy of (x_i, x_j), the diagonal its pxx."""
    from specenh import spectral

    dev = gpu_device
    C, n, nov, w, detrend, navg, scaling = MID
    x = upload(dev, signals(2, C, L_MID))
    (gs, _), _ = launch(dev, x, MID)
    gs = gs.cpu().numpy().astype(np.complex128)
    worst = 0.0
    for i in range(C):
        for j in range(i, C):
            _, _, est = spectral.spectral_estimates(
                x[:, i], x[:, j], fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend,
                scaling=scaling, navg=navg, want=("pxx", "pxy"))
            pxy = est["pxy"].cpu().numpy().astype(np.complex128)  # [B, F, G]
            e = np.abs(gs[..., i, j] - pxy).max(axis=1) / np.abs(pxy).max(axis=1)
            worst = max(worst, float(e.max()))
            if i == j:
                pxx = est["pxx"].cpu().numpy().astype(np.float64)
                e = np.abs(gs[..., i, i].real - pxx).max(axis=1) / pxx.max(axis=1)
                worst = max(worst, float(e.max()))
    print(f"\n[csm vs pair form] {worst:.2e} (bound {TOL_CSM:.0e})")
    assert worst <= TOL_CSM


STRUCT = [MID, (33, 256, 128, "hamm", "constant", 0, "density"),
          (40, 64, 48, "hann", "linear", 5, "density")]


@pytest.mark.parametrize("cfg", STRUCT, ids=[_id(c) for c in STRUCT])
def test_structure_is_bitwise_hermitian(gpu_device, cfg):
    dev = gpu_device
    L = 9 * cfg[1] + 37
    (gs, gc), _ = launch(dev, upload(dev, signals(2, cfg[0], L)), cfg)
    assert not torch.isnan(torch.view_as_real(gs)).any() and not torch.isnan(gc).any()
    assert torch.equal(gs.transpose(-1, -2), gs.conj().resolve_conj())
    re_im = torch.view_as_real(gs)
    assert torch.equal(re_im[..., 0].transpose(-1, -2), re_im[..., 0])
    assert torch.equal(re_im[..., 1].transpose(-1, -2), -re_im[..., 1])
    diag_im = torch.diagonal(re_im[..., 1], dim1=-2, dim2=-1)
    assert torch.equal(diag_im, torch.zeros_like(diag_im))
    assert torch.equal(gc.transpose(-1, -2), gc)
    d = torch.diagonal(gc, dim1=-2, dim2=-1)
    print(f"\n[csm structure {_id(cfg)}] diagonal coherence - 1: {float((d - 1).abs().max()):.1e}")
    assert float((d - 1).abs().max()) <= 2e-6


@pytest.mark.parametrize("cfg", STRUCT, ids=[_id(c) for c in STRUCT])
def test_channel_permutation_permutes_rows_and_columns(gpu_device, cfg):
    """Bitwise: catches an i / j mix-up or a transposed conjugate that symmetry alone misses."""
    dev = gpu_device
    C = cfg[0]
    L = 9 * cfg[1] + 37
    x = upload(dev, signals(2, C, L))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(C)).to(dev)
    assert not torch.equal(perm, torch.arange(C, device=dev))
    (gs, gc), _ = launch(dev, x, cfg)
    (ps, pc), _ = launch(dev, x[:, perm].contiguous(), cfg)
    assert torch.equal(torch.view_as_real(ps),
                       torch.view_as_real(gs[..., perm, :][..., :, perm].contiguous()))
    assert torch.equal(pc, gc[..., perm, :][..., :, perm])
    # asymmetric content: the imaginary parts are not all zero, so a conjugate would show
    assert float(torch.view_as_real(gs)[..., 1].abs().max()) > 0


@pytest.mark.parametrize("cfg", [MID, (40, 64, 48, "hann", "linear", 0, "density")],
                         ids=["C5-navg2", "C40-navg0"])
def test_batch_stride_subset_and_split_independence(gpu_device, cfg):
    from specenh import spectral

    dev = gpu_device
    C, n, nov, w, detrend, navg, scaling = cfg
    L = 9 * n + 37
    x = upload(dev, signals(3, C, L))
    full, _ = launch(dev, x, cfg)
    for b in range(3):  # a batch of 3 = three batches of 1
        one, _ = launch(dev, x[b:b + 1], cfg)
        for o, f in zip(one, full):
            assert torch.equal(torch.view_as_real(o[0]) if o.is_complex() else o[0],
                               torch.view_as_real(f[b]) if f.is_complex() else f[b])
    wide = torch.zeros(3, C + 2, L + 50, device=dev)  # channel_stride > L, batch_stride > C cs
    wide[:, :C, :L] = x
    view = wide[:, :C, :L]
    assert view.stride(1) > L and view.stride(0) > C * view.stride(1)
    strided, _ = launch(dev, view, cfg)
    for o, f in zip(strided, full):
        assert torch.equal(o, f)
    for bit in range(2):  # each output alone = the same values
        sub, _ = launch(dev, x, cfg, mask=1 << bit)
        assert [o is None for o in sub] == [i != bit for i in range(2)]
        assert torch.equal(sub[bit], full[bit])
    # the tensor layer, one launch against the batch split by a forced-down workspace cap
    kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, scaling=scaling,
              navg=navg)
    _, _, est = spectral.cross_spectral_matrix(x, **kw)
    assert torch.equal(est["csm"], full[0]) and torch.equal(est["coh"], full[1])
    cap = spectral.CSM_WORKSPACE_CAP
    try:
        spectral.CSM_WORKSPACE_CAP = 1  # below one shot: every shot runs alone
        _, _, split = spectral.cross_spectral_matrix(x, **kw)
    finally:
        spectral.CSM_WORKSPACE_CAP = cap
    assert torch.equal(split["csm"], full[0]) and torch.equal(split["coh"], full[1])


def test_workspace_size_and_all_zero_input(gpu_device):
    from specenh import ops

    dev = gpu_device
    C, n, nov = MID[:3]
    x = upload(dev, signals(2, C, L_MID))
    ws = ops.csm_workspace(x, *op_args(MID))
    assert ws.numel() == 2 * (n // 2 + 1) * 16 * 2 * C * 4  # T = 17: 8 groups of 2 enter
    with pytest.raises(ValueError, match="workspace"):
        launch(dev, x, MID, ws=ws[:-1])
    z = torch.zeros(2, C, L_MID, device=dev)
    for navg in (0, 2):
        (gs, gc), _ = launch(dev, z, MID[:5] + (navg, "density"))
        assert torch.equal(torch.view_as_real(gs), torch.zeros_like(torch.view_as_real(gs)))
        assert torch.isnan(gc).all()


def test_opcheck(gpu_device):
    from specenh import ops

    dev = gpu_device
    x = upload(dev, signals(2, 5, L_MID))
    args = op_args(MID)[:-1]
    op = torch.ops.specenh.csm.default
    torch.library.opcheck(op, (x, *args, 2, BOTH))
    torch.library.opcheck(op, (x, *args, 0, 1))
    torch.library.opcheck(op, (x, *args, 0, 2))
    shape = (2, 129, 8, 5, 5)
    ws = ops.csm_workspace(x, *args, 2)
    torch.library.opcheck(torch.ops.specenh.csm_out.default,
                          (x, *args, 2, torch.empty(shape, dtype=torch.complex64, device=dev),
                           torch.empty(shape, device=dev), ws))
    torch.library.opcheck(torch.ops.specenh.csm_out.default,
                          (x, *args, 2, None, torch.empty(shape, device=dev), None))


def test_tensor_and_numpy_layers(gpu_device):
    from specenh import signal, spectral

    dev = gpu_device
    C, n, nov, w, detrend, navg, scaling = MID
    x = signals(2, C, L_MID)
    xd = upload(dev, x)
    S, coh, _, allowed = reference(2, L_MID, MID)
    kw = dict(fs=FS, window=w, nperseg=n, noverlap=nov, detrend=detrend, scaling=scaling)
    f, t, est = spectral.cross_spectral_matrix(xd, navg=navg, **kw)
    fr, _ = scipy.signal.csd(x[0, 0].astype(np.float64), x[0, 1].astype(np.float64), **kw)
    assert np.array_equal(f, fr) and t.shape == (8,) and t.dtype == np.float64
    assert sorted(est) == ["coh", "csm"]
    assert est["csm"].shape == est["coh"].shape == (2, 129, 8, C, C)
    assert (est["csm"].dtype, est["coh"].dtype) == (torch.complex64, torch.float32)
    f, t, one = spectral.cross_spectral_matrix(xd[1], navg=navg, want=("csm",), **kw)
    assert list(one) == ["csm"] and one["csm"].shape == (129, 8, C, C)
    assert torch.equal(one["csm"], est["csm"][1])
    f, Cm = spectral.coherence_matrix(xd, fs=FS, window=w, nperseg=n, noverlap=nov,
                                      detrend=detrend)
    assert Cm.shape == (2, 129, C, C) and Cm.dtype == torch.float32
    f, Cm1 = spectral.coherence_matrix(xd[0], fs=FS, window=w, nperseg=n, noverlap=nov,
                                       detrend=detrend)
    assert Cm1.shape == (129, C, C) and torch.equal(Cm1, Cm[0])
    # numpy layer: leading axes flattened into the batch and restored, fp64 / complex128 out
    x4 = x.reshape(2, 1, C, L_MID)
    f, t, out = signal.cross_spectral_matrix(x4, navg=navg, **kw)
    assert np.array_equal(f, fr) and t.shape == (8,)
    assert out["csm"].shape == out["coh"].shape == (2, 1, 129, 8, C, C)
    assert (out["csm"].dtype, out["coh"].dtype) == (np.complex128, np.float64)
    assert normwise(out["csm"][:, 0], S) <= TOL_CSM
    assert float(np.abs(out["coh"][:, 0] - coh).max()) <= allowed
    f, t, out = signal.cross_spectral_matrix(x[0], nperseg=n, want=("coh",))
    assert list(out) == ["coh"] and out["coh"].shape == (129, 1, C, C)
