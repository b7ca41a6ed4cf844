"""GPU checks of the batched Hermitian eigensolver (csrc/herm_eig.hip) and the array mode
decomposition built on it: parity with numpy.linalg.eigh in complex128 under the project's
1e-5 contract, the output conventions, k selection, bitwise structure (batch position,
stride, unread elements), special matrices (diagonal, zero, c I, a NaN that must stay in its
matrix and must not keep the kernel busy), the output combinations of herm_eig_out, one launch
of 100,003 2 x 2 matrices against the closed form, and array_modes end to end from 2 to 64
channels. tests/test_modes_sizes_gpu.py runs every n, tests/test_modes_spectra_gpu.py other
spectra and scales.

Inputs are made on the CPU from a seeded generator, independent of the CSM kernels; every
output buffer is NaN-filled before the launch. Each test prints measured against allowed
(pytest -s); DESIGN.md §5.9 records the values."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 1e-5
M = 37  # not a multiple of any matrices-per-workgroup
# (n, T): T snapshots, rank min(n, T)
PARITY = [(2, 9), (3, 7), (5, 4), (16, 40), (17, 40), (32, 64), (33, 35), (40, 8), (40, 500),
          (63, 100), (64, 1), (64, 200)]


@functools.lru_cache(maxsize=None)
def matrices(n, T, count=M, seed=0):
    """S = X^H X / T in complex128 from X[count, T, n]: 3 coherent modes of amplitude 3^-j plus
    0.3 noise, per-channel gains 10^U(-1, 1); cast to complex64, the lower triangle the exact
    conjugate of the upper. Returns (S complex64, w_ref descending, V_ref columns) with the
    truth numpy.linalg.eigh in complex128 of that complex64 matrix."""
    rng = np.random.default_rng(1000 * n + T + 7919 * seed)

    def cn(*s):
        return (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2)

    X = 0.3 * cn(count, T, n)
    for j in range(3):
        shape = (np.exp(2j * np.pi * rng.uniform(size=(count, 1, n)))
                 * rng.uniform(0.5, 1, (count, 1, n)))
        X = X + 3.0 ** -j * cn(count, T, 1) * shape
    X = X * 10.0 ** rng.uniform(-1, 1, size=(count, 1, n))
    S = (np.einsum("mti,mtj->mij", X.conj(), X) / T).astype(np.complex64)
    iu = np.triu_indices(n, 1)
    S[:, iu[1], iu[0]] = S[:, iu[0], iu[1]].conj()
    S[:, np.arange(n), np.arange(n)] = S[:, np.arange(n), np.arange(n)].real
    w, V = np.linalg.eigh(S.astype(np.complex128))
    w, V = w[:, ::-1].copy(), V[:, :, ::-1].copy()
    for a in (S, w, V):
        a.setflags(write=False)
    return S, w, V


def run(dev, S, k, sweeps=True):
    """torch.ops.specenh.herm_eig_out into NaN-filled buffers -> numpy (w, v, sweeps)."""
    a = S if isinstance(S, torch.Tensor) else torch.from_numpy(np.array(S)).to(dev)
    n, lead = a.shape[-1], tuple(a.shape[:-2])
    w = torch.full(lead + (n,), float("nan"), device=dev)
    v = torch.full(lead + (k, n), complex("nan+nanj"), dtype=torch.complex64, device=dev)
    sw = torch.full(lead, -1, dtype=torch.int32, device=dev) if sweeps else None
    torch.ops.specenh.herm_eig_out(a, k, w, v, sw)
    torch.cuda.synchronize()
    return w.cpu().numpy(), v.cpu().numpy(), (sw.cpu().numpy() if sweeps else None)


def check_conventions(v, label):
    """Unit 2-norm; some component of (nearly) the largest modulus is real positive."""
    v = v.reshape(-1, v.shape[-1])
    norm = np.linalg.norm(v.astype(np.complex128), axis=-1)
    mod = np.abs(v.astype(np.complex128))
    top = mod >= (1 - 1e-6) * mod.max(axis=-1, keepdims=True)
    ok = (top & (v.imag == 0) & (v.real > 0)).any(axis=-1)
    print(f"[{label}] | ||v|| - 1 | max {np.abs(norm - 1).max():.2e} (allowed 1e-6)")
    assert np.abs(norm - 1).max() <= 1e-6
    assert ok.all()


def check_parity(S, w, v, wref, Vref, label):
    """The 1e-5 contract relative to the truth's spectral norm max |lambda| per matrix (written
    l1: it is lambda_1 where the matrix is positive semidefinite); S [m, n, n], w [m, n],
    v [m, k, n] (eigenvectors as rows), wref [m, n], Vref [m, n, n] (columns)."""
    S = S.astype(np.complex128)
    k = v.shape[1]
    l1 = np.abs(wref).max(axis=1)
    assert np.isfinite(w).all() and np.isfinite(v.view(np.float32)).all()
    e_w = (np.abs(w - wref).max(axis=1) / l1).max()
    vc = np.swapaxes(v.astype(np.complex128), 1, 2)  # columns
    res = np.linalg.norm(S @ vc - vc * w[:, None, :k], axis=1)  # [m, k]
    e_r = (res.max(axis=1) / l1).max()
    gram = np.swapaxes(vc, 1, 2).conj() @ vc
    e_o = np.abs(gram - np.eye(k)).max()
    print(f"[{label}] |w - w_ref|/l1 {e_w:.2e}  residual/l1 {e_r:.2e}  |VV^H - I| {e_o:.2e} "
          f"(allowed {TOL:.0e} each)")
    assert e_w <= TOL and e_r <= TOL and e_o <= TOL
    assert (np.diff(w, axis=1) <= 0).all()
    # leading mode: sin(theta) = ||v - v_ref <v_ref, v>||, v renormalised in fp64, against the
    # Davis-Kahan bound of a 1e-5 l1 residual, where the truth has a gap
    gap = (wref[:, 0] - wref[:, 1]) / l1
    sel = gap >= 0.05
    if sel.any():
        v0 = vc[sel, :, 0]
        v0 = v0 / np.linalg.norm(v0, axis=1, keepdims=True)
        r0 = Vref[sel, :, 0]
        sin = np.linalg.norm(v0 - r0 * np.einsum("mi,mi->m", r0.conj(), v0)[:, None], axis=1)
        ratio = (sin * gap[sel] / 2e-5).max()
        print(f"[{label}] leading mode: sin(theta) max {sin.max():.2e}, worst fraction of the "
              f"allowed 2e-5 l1/(l1 - l2): {ratio:.2f} ({int(sel.sum())} matrices with a gap)")
        assert ratio <= 1.0
    check_conventions(v, label)


@pytest.mark.parametrize("n,T", PARITY, ids=[f"n{n}-T{T}" for n, T in PARITY])
def test_parity_with_eigh(gpu_device, n, T):
    from specenh import _lib

    S, wref, Vref = matrices(n, T)
    w, v, sw = run(gpu_device, S, n)
    print(f"[n={n} T={T}] sweeps mean {sw.mean():.2f} max {sw.max()} "
          f"(bound {_lib.HERM_EIG_MAX_SWEEPS})")
    check_parity(S, w, v, wref, Vref, f"n={n} T={T}")
    assert (sw >= 1).all() and (sw <= _lib.HERM_EIG_MAX_SWEEPS).all()
    if T >= n:
        assert (sw < _lib.HERM_EIG_MAX_SWEEPS).all()


def test_single_matrix(gpu_device):
    S, wref, Vref = matrices(5, 4, count=1)
    w, v, sw = run(gpu_device, S, 5)
    check_parity(S, w, v, wref, Vref, "n=5 count=1")
    assert sw.shape == (1,) and 1 <= sw[0]


@pytest.mark.parametrize("n,T", [(5, 4), (33, 35)])
def test_k_selects_leading_rows(gpu_device, n, T):
    S = matrices(n, T)[0]
    w, v, sw = run(gpu_device, S, n)
    for k in (0, 1, 3):
        wk, vk, swk = run(gpu_device, S, k)
        assert vk.shape == (M, k, n)
        assert np.array_equal(wk, w) and np.array_equal(swk, sw)
        assert np.array_equal(vk.view(np.float32), v[:, :k].copy().view(np.float32))
    wk, vk = torch.ops.specenh.herm_eig(torch.from_numpy(np.array(S)).to(gpu_device), 3)
    assert np.array_equal(wk.cpu().numpy(), w)
    assert np.array_equal(vk.cpu().numpy().view(np.float32), v[:, :3].copy().view(np.float32))


@pytest.mark.parametrize("n,T", [(5, 4), (33, 35), (64, 200)])
def test_structure_is_bitwise(gpu_device, n, T):
    dev = gpu_device
    S = matrices(n, T)[0]
    w, v, sw = run(dev, S, 2)
    bits = lambda a: np.ascontiguousarray(a).view(np.float32)  # noqa: E731
    # a batch of 37 against 37 batches of 1
    a = torch.from_numpy(np.array(S)).to(dev)
    for m in range(M):
        w1, v1, s1 = run(dev, a[m:m + 1], 2)
        assert np.array_equal(w1[0], w[m]) and np.array_equal(bits(v1[0]), bits(v[m]))
        assert s1[0] == sw[m]
    # a strided input (matrix_stride = n^2 + 5) against its copy
    wide = torch.full((M, n * n + 5), complex("nan+nanj"), dtype=torch.complex64, device=dev)
    wide[:, :n * n] = a.reshape(M, n * n)
    strided = wide[:, :n * n].view(M, n, n)
    assert strided.stride() == (n * n + 5, n, 1)
    w2, v2, s2 = run(dev, strided, 2)
    assert np.array_equal(w2, w) and np.array_equal(bits(v2), bits(v)) and np.array_equal(s2, sw)
    # a leading shape that has to be copied (a permuted batch of batches) agrees too
    four = a[:36].reshape(4, 9, n, n).permute(1, 0, 2, 3)
    w3, v3, _ = run(dev, four, 2)
    assert np.array_equal(w3, np.swapaxes(w[:36].reshape(4, 9, n), 0, 1))
    assert np.array_equal(bits(v3), bits(np.swapaxes(v[:36].reshape(4, 9, 2, n), 0, 1)))
    # the lower triangle and the diagonal's imaginary part are never read
    dirty = np.array(S)
    il = np.tril_indices(n, -1)
    dirty[:, il[0], il[1]] = complex("nan+nanj")
    dirty.view(np.float32).reshape(M, n, n, 2)[:, np.arange(n), np.arange(n), 1] = np.nan
    assert np.isnan(dirty.imag[:, 0, 0]).all()
    assert np.array_equal(dirty.real[:, 0, 0], S.real[:, 0, 0])
    w4, v4, s4 = run(dev, dirty, 2)
    assert np.array_equal(w4, w) and np.array_equal(bits(v4), bits(v)) and np.array_equal(s4, sw)


@pytest.mark.parametrize("n", [5, 33])
def test_special_matrices(gpu_device, n):
    dev = gpu_device
    rng = np.random.default_rng(n)
    # already diagonal with distinct entries: exact
    d = rng.permutation(np.linspace(-2.0, 3.0, n)).astype(np.float32)
    D = np.zeros((2, n, n), np.complex64)
    D[:, np.arange(n), np.arange(n)] = d
    w, v, sw = run(dev, D, n)
    order = np.argsort(-d, kind="stable")
    assert np.array_equal(w[0], d[order]) and np.array_equal(w[1], w[0])
    assert np.array_equal(v[0], np.eye(n, dtype=np.complex64)[order]) and (sw == 1).all()
    # all zero: w = 0, v[m] = e_m
    w, v, sw = run(dev, np.zeros((3, n, n), np.complex64), n)
    assert (w == 0).all() and np.array_equal(v[1], np.eye(n, dtype=np.complex64))
    # c I: the vectors are arbitrary, the eigenvalues, residual and orthonormality are not
    c = 7.25
    I = np.broadcast_to(c * np.eye(n, dtype=np.complex64), (2, n, n)).copy()
    w, v, sw = run(dev, I, n)
    vc = v[0].astype(np.complex128)
    print(f"[n={n} cI] |w - c| max {np.abs(w - c).max():.2e} (allowed {TOL * c:.2e})")
    assert np.abs(w - c).max() <= TOL * c
    assert np.linalg.norm(c * vc.T - vc.T * w[0][None, :], axis=0).max() <= TOL * c
    assert np.abs(vc @ vc.conj().T - np.eye(n)).max() <= TOL
    # one NaN in the upper triangle of matrix 3 of 8: that matrix is NaN, the others are
    # bitwise what they are without it, and the call returns (bounded sweeps)
    S = np.array(matrices(n, 40, count=8)[0])
    w0, v0, s0 = run(dev, S, 2)
    S[3, 1, n - 1] = np.float32("nan")
    w1, v1, s1 = run(dev, S, 2)
    assert np.isnan(w1[3]).all() and np.isnan(v1[3].real).all() and np.isnan(v1[3].imag).all()
    keep = [m for m in range(8) if m != 3]
    assert np.array_equal(w1[keep], w0[keep]) and np.array_equal(s1[keep], s0[keep])
    assert np.array_equal(v1[keep].view(np.float32), v0[keep].view(np.float32))
    S[3, 1, n - 1] = np.float32("inf")  # and an infinity likewise
    assert np.isnan(run(dev, S, 2)[0][3]).all()


@pytest.mark.parametrize("n,T", [(5, 4), (33, 35)])
def test_output_combinations_are_bitwise(gpu_device, n, T):
    """Eigenvectors alone (w and sweeps absent) and eigenvalues alone (k = 0, an empty v, sweeps
    absent) are the bits of the call with every output."""
    dev = gpu_device
    S = matrices(n, T)[0]
    w, v, _ = run(dev, S, 2)
    a = torch.from_numpy(np.array(S)).to(dev)
    v1 = torch.full((M, 2, n), complex("nan+nanj"), dtype=torch.complex64, device=dev)
    torch.ops.specenh.herm_eig_out(a, 2, None, v1, None)
    w2 = torch.full((M, n), float("nan"), device=dev)
    v2 = torch.empty((M, 0, n), dtype=torch.complex64, device=dev)
    torch.ops.specenh.herm_eig_out(a, 0, w2, v2, None)
    torch.cuda.synchronize()
    assert np.isfinite(w).all() and np.isfinite(v.view(np.float32)).all()
    assert np.array_equal(v1.cpu().numpy().view(np.float32), v.view(np.float32))
    assert np.array_equal(w2.cpu().numpy(), w)


@functools.lru_cache(maxsize=None)
def two_by_two(count, seed=2):
    """`count` Hermitian 2 x 2 matrices [[a, b], [conj b, d]] in complex64 and their fp64 closed
    form: lambda = (a + d) / 2 +- rho, rho = sqrt(((a - d) / 2)^2 + |b|^2); the eigenvector of
    +rho is (delta + rho, conj b) for delta = (a - d) / 2 >= 0 and (b, rho - delta) otherwise
    (the form without cancellation), that of -rho its orthogonal complement."""
    rng = np.random.default_rng(seed)
    S = np.zeros((count, 2, 2), np.complex64)
    S[:, 0, 0], S[:, 1, 1] = rng.standard_normal(count), rng.standard_normal(count)
    S[:, 0, 1] = rng.standard_normal(count) + 1j * rng.standard_normal(count)
    S[:, 1, 0] = S[:, 0, 1].conj()
    a, d = S[:, 0, 0].real.astype(np.float64), S[:, 1, 1].real.astype(np.float64)
    b = S[:, 0, 1].astype(np.complex128)
    delta = (a - d) / 2
    rho = np.sqrt(delta ** 2 + np.abs(b) ** 2)
    wref = np.stack([(a + d) / 2 + rho, (a + d) / 2 - rho], axis=1)
    pos = delta >= 0
    x = np.where(pos, delta + rho, b)
    y = np.where(pos, b.conj(), rho - delta)
    norm = np.sqrt(np.abs(x) ** 2 + np.abs(y) ** 2)
    x, y = x / norm, y / norm
    Vref = np.stack([np.stack([x, -y.conj()], axis=1), np.stack([y, x.conj()], axis=1)], axis=1)
    for arr in (S, wref, Vref):
        arr.setflags(write=False)
    return S, wref, Vref


def test_large_batch_of_2x2(gpu_device):
    """100,003 matrices in one launch (25,001 workgroups of 4, the last one with 3 idle waves)
    against the closed form, and three of them against single-matrix calls."""
    count = 100_003
    S, wref, Vref = two_by_two(count)
    # the closed form is an eigendecomposition (the generator's own check, on the CPU)
    S128 = S.astype(np.complex128)
    assert np.abs(S128 @ Vref - Vref * wref[:, None, :]).max() <= 1e-12
    assert np.abs(np.swapaxes(Vref, 1, 2).conj() @ Vref - np.eye(2)).max() <= 1e-12
    w, v, sw = run(gpu_device, S, 2)
    print(f"[2x2 count={count}] sweeps max {sw.max()}")
    check_parity(S, w, v, wref, Vref, f"2x2 count={count}")
    # one rotation stores a_pq = 0 exactly, so the second sweep finds nothing to rotate
    assert (sw >= 1).all() and (sw <= 2).all()
    for m in (0, 50_001, count - 1):
        w1, v1, s1 = run(gpu_device, S[m:m + 1], 2)
        assert np.array_equal(w1[0], w[m]) and s1[0] == sw[m]
        assert np.array_equal(v1[0].view(np.float32), v[m].view(np.float32))


E2E = [(5, 256, 128, "hann", "linear", 2), (17, 64, 48, "hann", "linear", 5),
       (2, 64, 48, "hann", "linear", 0), (64, 64, 48, "hann", "constant", 3)]


@pytest.mark.parametrize("cfg", E2E, ids=["C5", "C17", "C2", "C64"])
def test_array_modes_end_to_end(gpu_device, cfg, monkeypatch):
    from test_csm_gpu import FS, signals

    from specenh import signal, spectral

    C, n, nov, win, detrend, navg = cfg
    x = signals(2, C, 9 * n + 37)
    xt = torch.from_numpy(np.array(x)).to(gpu_device)
    kw = dict(fs=FS, window=win, nperseg=n, noverlap=nov, detrend=detrend, navg=navg)
    f, t, est = spectral.array_modes(xt, k=2, **kw)
    f2, t2, csm = spectral.cross_spectral_matrix(xt, **kw)
    w, v, sw = spectral.hermitian_modes(csm["csm"], 2, return_sweeps=True)
    assert np.array_equal(f, f2) and np.array_equal(t, t2)
    B, F, G = w.shape[:3]
    assert est["power"].shape == (B, F, G, C) and est["modes"].shape == (B, F, G, 2, C)
    assert est["fraction"].shape == (B, F, G, 2) and sw.shape == (B, F, G)
    assert torch.equal(est["power"], w)
    assert torch.equal(torch.view_as_real(est["modes"]), torch.view_as_real(v))
    frac = est["power"][..., :2] / est["power"].sum(-1, keepdim=True)
    assert torch.equal(est["fraction"], frac)
    # the same through one-shot slices of the batch
    monkeypatch.setattr(spectral, "CSM_WORKSPACE_CAP", 1)
    _, _, est1 = spectral.array_modes(xt, k=2, **kw)
    monkeypatch.undo()
    for name in est:
        assert torch.equal(torch.view_as_real(est1[name]) if est[name].is_complex() else
                           est1[name], torch.view_as_real(est[name]) if est[name].is_complex()
                           else est[name])
    # parity against eigh of the downloaded GPU CSM
    S = csm["csm"].cpu().numpy().reshape(-1, C, C)
    wref, Vref = np.linalg.eigh(S.astype(np.complex128))
    wref, Vref = wref[:, ::-1], Vref[:, :, ::-1]
    wn, vn = spectral.hermitian_modes(csm["csm"], C)
    check_parity(S, wn.cpu().numpy().reshape(-1, C), vn.cpu().numpy().reshape(-1, C, C), wref,
                 Vref, f"array C={C}")
    check_parity(S, est["power"].cpu().numpy().reshape(-1, C),
                 est["modes"].cpu().numpy().reshape(-1, 2, C), wref, Vref, f"array C={C} k=2")
    # the numpy form: the same values widened, leading axes kept
    fn, tn, en = signal.array_modes(x, k=2, **kw)
    assert en["power"].dtype == np.float64 and en["modes"].dtype == np.complex128
    for name in est:
        assert np.array_equal(en[name], est[name].cpu().numpy().astype(en[name].dtype),
                              equal_nan=True)
    _, _, e1 = signal.array_modes(x[1], k=2, **kw)
    assert e1["power"].shape == (F, G, C) and e1["modes"].shape == (F, G, 2, C)
    assert np.array_equal(e1["power"], en["power"][1])
    assert np.array_equal(e1["modes"], en["modes"][1])
    _, _, e0 = spectral.array_modes(xt[0], k=2, **kw)
    assert torch.equal(e0["power"], est["power"][0]) and e0["fraction"].shape == (F, G, 2)


def test_opcheck(gpu_device):
    S = torch.from_numpy(np.array(matrices(5, 4)[0][:6])).to(gpu_device)
    torch.library.opcheck(torch.ops.specenh.herm_eig, (S, 2))
    torch.library.opcheck(torch.ops.specenh.herm_eig, (S.reshape(2, 3, 5, 5), 0))
    w = torch.empty(6, 5, device=gpu_device)
    v = torch.empty(6, 2, 5, dtype=torch.complex64, device=gpu_device)
    sw = torch.empty(6, dtype=torch.int32, device=gpu_device)
    torch.library.opcheck(torch.ops.specenh.herm_eig_out, (S, 2, w, v, sw))
