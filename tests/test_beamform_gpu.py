"""GPU checks of the steered-response spectra (csrc/steered_power.hip): the kernel against the
fp64 restatement (tests/beamform_local.py) on the same inputs over the tile edges, the long
reduction, the fused Bartlett path end to end against scipy.signal.csd matrices and against the
GPU's own cross_spectral_matrix, Capon and MUSIC end to end on plane-wave modes, the bitwise
structure, special inputs, opcheck, and the tensor layer against the numpy layer.

Kernel tolerance, normwise per matrix (max_n |got - ref| / max_n |ref|): 4 x the error of the
fp32 restatement of the same arithmetic on the CPU (beamform_local.raw_q32 against raw_q over
KERNEL_CASES, w null and given), measured 5.12e-7 for the SUM and BARTLETT epilogues and
9.59e-7 for INVERSE and MUSIC (2.5e-6 pointwise): TOL_Q = 2.05e-6, TOL_INV = 3.84e-6. The 4 x
covers the order of summation, which differs between numpy and the MFMA chain.

Capon and MUSIC against scipy matrices: the bound is 8 x the normwise difference, measured on
the CPU on these same signals, between oracle/herm_eig.py (the fp32 restatement of the solver)
feeding the fp64 projection and the all-fp64 chain: beamform_local.chain32, recorded in
beamform_local.CHAIN32 and recomputed by tests/test_beamform_cpu.py (Capon / MUSIC at C = 5:
4.03e-6 / 1.83e-5; 12: 1.79e-5 / 1.45e-5; 20: 3.04e-5 / 1.27e-5; 40: 5.62e-5 / 1.26e-5; 44:
5.64e-5 / 1.43e-5; 52: 7.23e-5 / 1.02e-5; 64: 6.90e-5 / 1.18e-5; pointwise up to 3.5e-4). The
8 x covers the CSM's own 5e-7 and the projection's rounding on top of the eigenpairs'.

The channel axis: steered_power_kernel<KH> has eight instantiations picked by (C - 1) / 8;
beamform_local.CHANNEL_CASES runs the kernel at every C in 1 .. 64 at the same tolerances
(tests/test_beamform_cpu.py asserts that the fp32 restatement is no worse there), the padding
channels of an instantiation are compared bit for bit with explicit zeros, and the fused and
end-to-end tests run at C = 12, 20, 44 and 52 as well (KH = 8, 12, 24, 28).

Every output is NaN-filled before the launch. Each test prints measured against allowed
(pytest -s)."""
import numpy as np
import pytest
import scipy.signal
import torch

import beamform_local as bl

pytestmark = pytest.mark.gpu

FS = bl.FS
CPU32_Q, CPU32_INV = 5.12e-7, 9.59e-7
TOL_Q, TOL_INV = 4 * CPU32_Q, 4 * CPU32_INV
TOL_POST = (TOL_Q, TOL_Q, TOL_INV, TOL_INV)
TOL_CSM = 1e-5
CHAIN32 = bl.CHAIN32
N_MODES = bl.N_MODES
NAN = float("nan")
SCALING = {"density": 0, "spectrum": 1}
DETREND = {False: 0, "constant": 1, "linear": 2}


def up(dev, a):
    return None if a is None else torch.from_numpy(np.array(a, order="C")).to(dev)


def steer(dev, V, w, A, post, scale=1.0, conj=False, table=None):
    """torch.ops.specenh.steered_power_out into a NaN-filled buffer -> numpy."""
    import specenh  # noqa: F401  (registers the operators)

    V, w, A = (a if isinstance(a, torch.Tensor) or a is None else up(dev, a) for a in (V, w, A))
    out = torch.full(tuple(V.shape[:-2]) + (A.shape[-2],), NAN, device=dev)
    torch.ops.specenh.steered_power_out(V, w, A, post, scale, conj, table, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def fused(dev, x, n, nov, window, detrend, navg, A, scaling="density", nan_ws=True):
    """torch.ops.specenh.array_spectrum_out into a NaN-filled buffer with a NaN-filled
    workspace -> (numpy [B, F, G, K], workspace)."""
    from specenh import ops

    args = (n, nov, window, FS, SCALING[scaling], DETREND[detrend], navg)
    B, _, L = x.shape
    T = (L - n) // (n - nov) + 1
    out = torch.full((B, n // 2 + 1, 1 if navg <= 0 else T // navg, A.shape[-2]), NAN, device=dev)
    ws = ops.array_spectrum_workspace(x, *args)
    if nan_ws:
        ws.view(torch.float32).fill_(NAN)
    ops.ops.array_spectrum_out(x, *args, A, out, ws)
    torch.cuda.synchronize()
    return out.cpu().numpy(), ws


def case_id(c):
    return "M%d-C%d-K%d-n%d-%s" % (c[:4] + ("perbin" if c[4] else "one",))


def kernel_against_the_restatement(gpu_device, case):
    """The four epilogues with w null and given, then conj(A) with a scale and a factor per
    table, against the fp64 restatement on the same inputs."""
    M, C, K, count, per_bin = case
    V, A, w = bl.kernel_case(*case)
    worst = [0.0] * 4
    for ww in (None, w):
        q = bl.raw_q(V, ww, A)
        for post in range(4):
            got = steer(gpu_device, V, ww, A, post)
            assert got.shape == (count, 1, K) and np.isfinite(got).all()
            worst[post] = max(worst[post], bl.normwise(got, bl.post(q, A, post)))
    print(f"[{case}] normwise SUM {worst[0]:.2e} BARTLETT {worst[1]:.2e} (allowed {TOL_Q:.2e}) "
          f"INVERSE {worst[2]:.2e} MUSIC {worst[3]:.2e} (allowed {TOL_INV:.2e})")
    for post in range(4):
        assert worst[post] <= TOL_POST[post]
    # conj(A), a scale and a factor per table
    table = np.linspace(0.5, 2.0, count) if per_bin else np.array([1.5])
    got = steer(gpu_device, V, w, A, bl.BARTLETT, 0.75, True, up(gpu_device, table))
    ref = bl.post(bl.raw_q(V, w, A, conj=True), A, bl.BARTLETT, 0.75) * table[:, None, None]
    err = bl.normwise(got, ref)
    print(f"[{case}] conj, scaled: {err:.2e} (allowed {TOL_Q:.2e})")
    assert err <= TOL_Q


@pytest.mark.parametrize("case", bl.KERNEL_CASES, ids=case_id)
def test_kernel_against_the_restatement(gpu_device, case):
    kernel_against_the_restatement(gpu_device, case)


@pytest.mark.parametrize("case", bl.CHANNEL_CASES, ids=case_id)
def test_kernel_at_every_channel_count(gpu_device, case):
    """Every C in 1 .. 64: all eight instantiations steered_power_kernel<KH>, eight channel
    counts each, with one to four row tiles and one or two workgroups a matrix, at the
    tolerances of test_kernel_against_the_restatement."""
    print(f"[C={case[1]}: KH = {4 * (bl.instantiation(case[1]) + 1)}]")
    kernel_against_the_restatement(gpu_device, case)


PAD_CHANNELS = (9, 12, 17, 20, 25, 41, 44, 49, 52, 57)


@pytest.mark.parametrize("C", PAD_CHANNELS)
def test_padding_channels_are_exact_zeros(gpu_device, C):
    """The channels between C and the 2 KH an instantiation walks are predicated zero loads:
    the result equals, bit for bit, that of the same data padded with explicit zeros to
    8 ceil(C / 8) channels (the same instantiation; a lane's k order depends on KH alone and
    a zero operand adds +-0). The rows of V are views into a wider buffer whose gaps are NaN,
    as in test_generic_structure_is_bitwise. The operator takes the table contiguous only (the
    C ABI has no row stride for it), so A sits in a flat NaN-filled buffer with NaN right before
    its first and after its last row: a load past a row of V or past the table's end puts NaN
    into the output, one past an inner row of A changes |a|^2 and so the MUSIC bits."""
    dev = gpu_device
    M, K, count = 33, 33, 3  # two row tiles and two waves, the second ones with a single row
    V, A, w = bl.kernel_case(M, C, K, count, False)
    Cp = 8 * -(-C // 8)
    assert Cp > C and bl.instantiation(Cp) == bl.instantiation(C)
    Vp = np.zeros((count, 1, M, Cp), np.complex64)
    Vp[..., :C] = V
    Ap = np.zeros((K, Cp), np.complex64)
    Ap[:, :C] = A
    wide = torch.full((count, 1, M + 3, Cp + 5), complex(NAN, NAN), dtype=torch.complex64,
                      device=dev)
    wide[:, :, :M, :C] = up(dev, V)
    view = wide[:, :, :M, :C]
    assert not view.is_contiguous() and view.stride(-2) > C
    flat = torch.full((K * C + 2 * Cp,), complex(NAN, NAN), dtype=torch.complex64, device=dev)
    flat[Cp:Cp + K * C] = up(dev, A).reshape(-1)
    table = flat[Cp:Cp + K * C].view(K, C)
    assert table.is_contiguous() and table.data_ptr() % 8 == 0
    for post in (bl.SUM, bl.MUSIC):
        got = steer(dev, view, up(dev, w), table, post)
        assert not np.isnan(got).any(), "a predicated load read past a row"
        padded = steer(dev, Vp, w, Ap, post)
        differ = int((got.view(np.uint32) != padded.view(np.uint32)).sum())
        print(f"[C={C} as {Cp}, post {post}] elements that differ from explicit zeros: {differ} "
              f"of {got.size}, normwise {bl.normwise(got, padded):.2e} (allowed: none)")
        assert np.array_equal(got, padded)


def test_w_all_ones_is_w_null_bitwise(gpu_device):
    for case in ((33, 64, 65, 7, True), (17, 32, 65, 1, False), (2, 2, 31, 7, False)):
        V, A, w = bl.kernel_case(*case)
        for post in range(4):
            a = steer(gpu_device, V, None, A, post)
            b = steer(gpu_device, V, np.ones_like(w), A, post)
            assert np.array_equal(a, b)


def test_generic_structure_is_bitwise(gpu_device):
    """Rows of the table, matrices of the batch, the row and matrix strides: a value depends on
    its own matrix and its own steering row."""
    dev = gpu_device
    V, A, w = bl.kernel_case(33, 64, 65, 7, False)
    full = steer(dev, V, w, A, bl.SUM)
    rows = [0, 5, 31, 32, 64]
    assert np.array_equal(steer(dev, V, w, A[rows], bl.SUM), full[..., rows])
    assert np.array_equal(steer(dev, V, w, np.tile(A, (4, 1))[:257], bl.SUM)[..., 130:195],
                          full)  # K = 257: three workgroups a matrix, the rows in another tile
    for j in (0, 3, 6):
        assert np.array_equal(steer(dev, V[j:j + 1], w[j:j + 1], A, bl.SUM), full[j:j + 1])
    # rows and matrices with gaps (NaN between them), read in place
    wide = torch.full((7, 1, 40, 70), complex(NAN, NAN), dtype=torch.complex64, device=dev)
    wide[:, :, :33, :64] = up(dev, V)
    view = wide[:, :, :33, :64]
    assert not view.is_contiguous()
    assert np.array_equal(steer(dev, view, up(dev, w), up(dev, A), bl.SUM), full)
    # a layout that has to be copied
    turned = up(dev, V).transpose(-1, -2).contiguous().transpose(-1, -2)
    assert turned.stride(-1) != 1
    assert np.array_equal(steer(dev, turned, up(dev, w), up(dev, A), bl.SUM), full)
    # a table per bin: matrix j with table j alone
    V, A, w = bl.kernel_case(31, 33, 257, 7, True)
    full = steer(dev, V, w, A, bl.MUSIC)
    for j in (0, 4, 6):
        assert np.array_equal(steer(dev, V[j:j + 1], w[j:j + 1], A[j], bl.MUSIC), full[j:j + 1])


def window_scale(window, n):
    win = scipy.signal.get_window(window, n)
    return 1.0 / (FS * (win ** 2).sum())


def test_long_reduction(gpu_device):
    """T = 4101 frames in one group (129 chunks of fp32 handed to fp64): the fused Bartlett
    against fp64 on the workspace's own rows, and against scipy matrices."""
    from test_csm_gpu import L_LONG, signals

    C, n, nov = 3, 64, 48
    x = signals(2, C, L_LONG)
    A = bl.steering(np.array([0.0, 0.7, 1.9]), np.arange(-2, 3)).astype(np.complex64)
    got, ws = fused(gpu_device, up(gpu_device, x), n, nov, "hann", "linear", 0, up(gpu_device, A))
    T = (L_LONG - n) // (n - nov) + 1
    assert T == 4101 and got.shape == (2, 33, 1, 5) and np.isfinite(got).all()
    rows = ws.view(torch.complex64).cpu().numpy().reshape(2, 33, 1, T, C)  # 2 X
    m = np.full(33, 2.0)
    m[[0, -1]] = 1.0
    m = m * window_scale("hann", n) / (4.0 * T)
    ref = bl.post(bl.raw_q(rows, None, A, conj=True), A, bl.BARTLETT) * m[None, :, None, None]
    err = bl.normwise(got, ref)
    S = bl.scipy_csm(x, n, nov, "hann", "linear", 0)
    err_s = bl.normwise(got, bl.bartlett(S, A))
    print(f"[long] against fp64 on the same rows {err:.2e}, against scipy matrices {err_s:.2e} "
          f"(allowed {TOL_Q:.2e})")
    assert err <= TOL_Q and err_s <= TOL_Q


# (C, nperseg, noverlap, window, detrend, navg, K, per_bin)
FUSED = [(5, 256, 128, "hann", "linear", 2, 17, False),
         (40, 64, 48, "hann", "constant", 0, 65, False),
         (33, 256, 128, "hamm", "constant", 0, 17, True)]
# the instantiations KH = 8, 12, 24, 28, which no other fused case launches
FUSED += [(C, 64, 48, "hann", "constant", 0, 65, False) for C in (12, 20, 44, 52)]


def table(C, K, F, per_bin, seed=0):
    """Mode-number steering vectors on bl.angles(C), or delay steering per bin."""
    if not per_bin:
        return bl.steering(bl.angles(C), np.arange(K) - K // 2).astype(np.complex64)
    tau = np.random.default_rng(seed + C).uniform(-2e-5, 2e-5, (K, C))
    f = np.arange(F) * FS / (2 * (F - 1))
    return np.exp(-2j * np.pi * f[:, None, None] * tau[None]).astype(np.complex64)


@pytest.mark.parametrize("cfg", FUSED, ids=["C5", "C40", "C33-perbin", "C12", "C20", "C44", "C52"])
def test_fused_bartlett_end_to_end(gpu_device, cfg):
    from test_csm_gpu import signals

    from specenh import beamform, spectral

    C, n, nov, window, detrend, navg, K, per_bin = cfg
    dev = gpu_device
    x = signals(2, C, 9 * n + 37)
    A = table(C, K, n // 2 + 1, per_bin)
    xt, At = up(dev, x), up(dev, A)
    got, _ = fused(dev, xt, n, nov, window, detrend, navg, At)
    assert np.isfinite(got).all()
    S = bl.scipy_csm(x, n, nov, window, detrend, navg)
    err = bl.normwise(got, bl.bartlett(S, A))
    kw = dict(fs=FS, window=window, nperseg=n, noverlap=nov, detrend=detrend, navg=navg)
    _, _, est = spectral.cross_spectral_matrix(xt, want=("csm",), **kw)
    err_g = bl.normwise(got, bl.bartlett(est["csm"].cpu().numpy(), A))
    print(f"[fused {cfg}] against scipy matrices {err:.2e}, against the GPU's matrices "
          f"{err_g:.2e} (allowed {TOL_CSM:.0e})")
    assert err <= TOL_CSM and err_g <= TOL_CSM
    # the tensor layer is the operator, bit for bit, and gives f and the group times
    f, t, P = beamform.array_spectrum(xt, At, **kw)
    f2, t2, _ = spectral.cross_spectral_matrix(xt, want=("csm",), **kw)
    assert np.array_equal(f, f2) and np.array_equal(t, t2)
    assert P.dtype == torch.float32 and np.array_equal(P.cpu().numpy(), got)


@pytest.mark.parametrize("L,navg", [(256, 0), (256, 1), (9 * 256 + 37, 1)],
                         ids=["one-frame", "one-frame-navg1", "navg1"])
def test_fused_bartlett_edge_lengths(gpu_device, L, navg):
    from test_csm_gpu import signals

    C, n, nov = 5, 256, 128
    x = signals(2, C, L)
    A = table(C, 17, n // 2 + 1, False)
    got, _ = fused(gpu_device, up(gpu_device, x), n, nov, "hann", "linear", navg,
                   up(gpu_device, A))
    S = bl.scipy_csm(x, n, nov, "hann", "linear", navg)
    assert got.shape == S.shape[:3] + (17,) and np.isfinite(got).all()
    err = bl.normwise(got, bl.bartlett(S, A))
    print(f"[fused L={L} navg={navg}] {err:.2e} (allowed {TOL_CSM:.0e})")
    assert err <= TOL_CSM


L_E2E = bl.L_E2E  # 24 frames of 64 / 48: three blocks of 8, 5 samples left over
E2E_KW = bl.E2E_KW
e2e_reference = bl.e2e_reference


@pytest.mark.parametrize("C", [5, 40, 64, 12, 20, 44, 52])
def test_capon_and_music_end_to_end(gpu_device, C):
    """Blocks of 8 frames (< C from 12 channels up: rank-deficient matrices), loading 1e-2,
    two sources. C = 12, 20, 44, 52: the instantiations KH = 8, 12, 24, 28."""
    from specenh import beamform, spectral

    x, S, A = e2e_reference(C)
    xt, At = up(gpu_device, x), up(gpu_device, A)
    _, _, modes = spectral.array_modes(xt, k=C, **E2E_KW)
    lam, v = modes["power"].cpu().numpy(), modes["modes"].cpu().numpy()
    for method, tol in (("capon", TOL_INV), ("music", TOL_INV), ("bartlett", TOL_CSM)):
        _, _, P = beamform.array_spectrum(xt, At, method=method, nsources=2, loading=1e-2,
                                          **E2E_KW)
        got = P.cpu().numpy()
        assert got.shape == (2, 33, 3, N_MODES.size) and np.isfinite(got).all()
        ref = bl.estimate(S, A, method, 2, 1e-2)
        err_s = bl.normwise(got, ref)
        if method == "bartlett":
            print(f"[C={C} bartlett] against scipy matrices {err_s:.2e} (allowed {tol:.0e})")
            assert err_s <= tol
        else:
            # (a) the fp64 restatement on the GPU's own eigenpairs; (b) on scipy matrices
            err_a = bl.normwise(got, bl.from_eigenpairs(lam, v, A, method, 2, 1e-2))
            allowed = 8 * CHAIN32[(C, method)]
            print(f"[C={C} {method}] on the GPU's eigenpairs {err_a:.2e} (allowed {tol:.2e}), "
                  f"against scipy matrices {err_s:.2e} (allowed {allowed:.2e})")
            assert err_a <= tol and err_s <= allowed
            assert method != "music" or got.min() >= 1 - TOL_INV
        # (c) the peaks, in the bands' bins: the injected mode numbers
        for k in bl.BINS:
            for b in range(2):
                for g in range(3):
                    for p in (got[b, k, g], ref[b, k, g]):
                        if method == "bartlett":
                            assert N_MODES[np.argmax(p)] in (3, -2)
                        else:
                            assert set(N_MODES[bl.local_maxima(p)[:2]]) == {3, -2}


@pytest.mark.parametrize("method", ["bartlett", "capon", "music"])
def test_array_spectrum_structure(gpu_device, method, monkeypatch):
    from specenh import beamform, spectral

    C = 40
    dev = gpu_device
    x, _, A = e2e_reference(C)
    x = np.concatenate((x, bl.signals(1, C, L_E2E, seed=1)))  # three shots
    xt, At = up(dev, x), up(dev, A)
    kw = dict(method=method, nsources=2, **E2E_KW)
    full = beamform.array_spectrum(xt, At, **kw)[2]
    assert full.shape == (3, 33, 3, 17)
    # a subset of the steering rows, a subset of the shots, one shot without its batch axis
    rows = [0, 3, 16]
    assert torch.equal(beamform.array_spectrum(xt, At[rows], **kw)[2], full[..., rows])
    assert torch.equal(beamform.array_spectrum(xt[1:], At, **kw)[2], full[1:])
    one = beamform.array_spectrum(xt[2], At, **kw)[2]
    assert one.shape == (33, 3, 17) and torch.equal(one, full[2])
    # a strided batch: batch_stride > C * channel_stride, NaN in the gaps
    wide = torch.full((3, C + 3, L_E2E + 11), NAN, device=dev)
    wide[:, :C, :L_E2E] = xt
    view = wide[:, :C, :L_E2E]
    assert view.stride(0) > C * view.stride(1) > C * L_E2E
    assert torch.equal(beamform.array_spectrum(view, At, **kw)[2], full)
    # one-shot slices of the batch
    monkeypatch.setattr(spectral, "CSM_WORKSPACE_CAP", 1)
    sliced = beamform.array_spectrum(xt, At, **kw)[2]
    monkeypatch.undo()
    assert torch.equal(sliced, full)
    # a permutation of the channels, signals and table alike. Bartlett: every channel's spectra
    # are the same bits, only the kernel's c order changes: the kernel tolerance. Capon and
    # MUSIC: the solver rotates other pairs in another order, so its own rounding (CHAIN32)
    # enters twice.
    perm = np.random.default_rng(4).permutation(C)
    got = beamform.array_spectrum(up(dev, x[:, perm]), up(dev, A[:, perm]), **kw)[2]
    tol = TOL_Q if method == "bartlett" else 8 * CHAIN32[(C, method)]
    err = bl.normwise(got.cpu().numpy(), full.cpu().numpy())
    print(f"[{method}] permuted channels {err:.2e} (allowed {tol:.2e})")
    assert err <= tol


def test_a_channel_permutation_of_the_kernel(gpu_device):
    """The generic operator under a permutation of c, rows and table alike: within the kernel
    tolerance (not bitwise: the order of the c sum changes)."""
    V, A, w = bl.kernel_case(33, 64, 65, 7, False)
    perm = np.random.default_rng(9).permutation(64)
    for post in range(4):
        a = steer(gpu_device, V, w, A, post)
        b = steer(gpu_device, V[..., perm], w, A[:, perm], post)
        err = bl.normwise(b, a)
        print(f"[post {post}] permuted channels {err:.2e} (allowed {TOL_POST[post]:.2e})")
        assert err <= TOL_POST[post]


def test_all_zero_input(gpu_device):
    from specenh import beamform

    C = 5
    A = up(gpu_device, bl.steering(bl.angles(C), N_MODES).astype(np.complex64))
    x = torch.zeros(2, C, L_E2E, device=gpu_device)
    P = beamform.array_spectrum(x, A, **E2E_KW)[2]
    assert P.shape == (2, 33, 3, 17) and (P == 0).all()
    # the eigenvectors of the zero matrix are e_m: the noise subspace holds C - 2 of them
    P = beamform.array_spectrum(x, A, method="music", nsources=2, **E2E_KW)[2]
    assert torch.allclose(P, torch.full_like(P, C / (C - 2)), rtol=1e-6)


def test_all_zero_input_capon_is_inf(gpu_device):
    """A matrix without power has lambda = 0 and delta = 0: every term of the Capon sum has a
    zero denominator and so no weight (the pseudo-inverse), q = 0 and P_capon = 1 / 0 = inf. A
    zero shot beside a live one: inf in that shot alone, the other bit for bit what it is."""
    from specenh import beamform

    C = 5
    A = up(gpu_device, bl.steering(bl.angles(C), N_MODES).astype(np.complex64))
    x = torch.zeros(2, C, L_E2E, device=gpu_device)
    P = beamform.array_spectrum(x, A, method="capon", **E2E_KW)[2]
    print(f"[zero input] Capon min {float(P.min())} max {float(P.max())}")
    assert torch.isinf(P).all() and (P > 0).all()
    live = up(gpu_device, e2e_reference(C)[0])
    clean = beamform.array_spectrum(live, A, method="capon", **E2E_KW)[2]
    live[1] = 0
    P = beamform.array_spectrum(live, A, method="capon", **E2E_KW)[2]
    assert torch.isinf(P[1]).all() and (P[1] > 0).all() and torch.equal(P[0], clean[0])
    ref = bl.from_eigenpairs(np.zeros((1, C)), np.eye(C)[None], A.cpu().numpy(), "capon")
    assert np.isposinf(ref).all()  # the restatement's convention is the same


@pytest.mark.parametrize("method", ["bartlett", "capon", "music"])
def test_a_nan_sample_stays_in_its_shot(gpu_device, method):
    from specenh import beamform

    C = 5
    x, _, A = e2e_reference(C)
    At = up(gpu_device, A)
    kw = dict(method=method, nsources=2, **E2E_KW)
    clean = beamform.array_spectrum(up(gpu_device, x), At, **kw)[2]
    bad = np.array(x)
    bad[1, 2, 100] = np.nan  # frames 3..6 of block 0 of shot 1
    got = beamform.array_spectrum(up(gpu_device, bad), At, **kw)[2]
    assert torch.isnan(got[1, :, 0]).all()
    assert torch.equal(got[0], clean[0]) and torch.equal(got[1, :, 1:], clean[1, :, 1:])


def test_opcheck(gpu_device):
    import specenh  # noqa: F401  (registers the operators)

    dev = gpu_device
    V, A, w = bl.kernel_case(17, 32, 65, 1, False)
    V, A, w = up(dev, V), up(dev, A), up(dev, w)
    torch.library.opcheck(torch.ops.specenh.steered_power, (V, w, A, 0, 1.0, False, None))
    torch.library.opcheck(torch.ops.specenh.steered_power, (V, None, A, 3, 2.0, True, None))
    out = torch.empty(1, 1, 65, device=dev)
    torch.library.opcheck(torch.ops.specenh.steered_power_out,
                          (V, w, A, 2, 1.0, False, None, out))
    x = up(dev, bl.signals(2, 5, L_E2E))
    As = up(dev, bl.steering(bl.angles(5), N_MODES).astype(np.complex64))
    out = torch.empty(2, 33, 3, 17, device=dev)
    torch.library.opcheck(torch.ops.specenh.array_spectrum_out,
                          (x, 64, 48, "hann", FS, 0, 1, 8, As, out, None))


@pytest.mark.parametrize("method", ["bartlett", "capon", "music"])
def test_the_tensor_layer_and_the_numpy_layer_agree(gpu_device, method):
    from specenh import beamform, signal

    C = 5
    x, _, A = e2e_reference(C)
    kw = dict(method=method, nsources=2, **E2E_KW)
    f, t, P = beamform.array_spectrum(up(gpu_device, x), up(gpu_device, A), **kw)
    fn, tn, Pn = signal.array_spectrum(x, A, **kw)
    assert Pn.dtype == np.float64 and np.array_equal(f, fn) and np.array_equal(t, tn)
    assert np.array_equal(Pn, P.cpu().numpy().astype(np.float64))
    _, _, P1 = signal.array_spectrum(x[1], A, **kw)
    assert P1.shape == (33, 3, 17) and np.array_equal(P1, Pn[1])
    fm, tm, n, Pm = beamform.mode_number_spectrum(up(gpu_device, x), bl.angles(C), 8, **kw)
    assert np.array_equal(n, N_MODES) and torch.equal(Pm, P)
