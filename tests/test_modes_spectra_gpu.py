"""GPU checks of the batched Hermitian eigensolver (csrc/herm_eig.hip) on spectra with a known
answer and across the scale of the input.

Spectra: S = Q diag(lambda) Q^H in complex128, Q a Haar unitary (QR of a complex Gaussian, the
phases of diag(R) divided out), cast to complex64 with the lower triangle the exact conjugate
of the upper; indefinite, negative definite, clustered, graded over 1e8, degenerate and rank-one
spectra, a Hermitian matrix with an exactly zero diagonal (d_max = 0: the skip floor vanishes)
and a Gram matrix under channel gains spread over 1e8. n = 8, 21, 33, 45, 64 cover the narrow
kernel, the wide kernel with four waves a workgroup and pass loops of 2, 3 and 4 trips
(tests/test_modes_sizes_gpu.py has the table). The truth is numpy.linalg.eigh in complex128 of
the complex64 matrix; the contract is test_modes_gpu.check_parity's 1e-5 of the spectral norm.
tests/test_modes_oracle_cpu.py runs the method's numpy restatement on the same inputs, the
standing proof that they are fair to the method.

Scale: a power-of-two factor commutes with every rounding of the kernel (the skip threshold,
tau, hx / r and the normalisation are ratios or scale with the input), so the eigenvalues
scale exactly and the vectors and sweep counts do not change, bit for bit; other factors
(1e-6 is the size of the project's real cross-spectral matrices) and 2^+-80 hold the contract.

Each test prints measured against allowed (pytest -s); DESIGN.md §5.9 records the values."""
import functools

import numpy as np
import pytest
import torch

from test_modes_gpu import check_parity, matrices, run

pytestmark = pytest.mark.gpu

COUNT = 9
SPECTRA_N = [8, 21, 33, 45, 64]
SCALE_N = [5, 21, 33, 45, 64]


def clustered(n):
    return np.concatenate([[1.0, 1 - 3e-6, 1 - 6e-6], np.geomspace(0.3, 1e-3, n - 3)])


# prescribed spectra, as written (not sorted)
PRESCRIBED = {
    "indefinite": lambda n: np.linspace(-2.0, 3.0, n),
    "negative-definite": lambda n: -np.geomspace(1.0, 1e-3, n),
    "clustered-top": clustered,
    "graded": lambda n: np.geomspace(1.0, 1e-8, n),
    "two-levels": lambda n: np.concatenate([np.ones(n // 2), np.full(n - n // 2, 1e-2)]),
    "rank-one": lambda n: np.concatenate([[1.0], np.zeros(n - 1)]),
    "signed-pairs": lambda n: np.concatenate([np.ones(n // 2), -np.ones(n - n // 2)]),
}
FAMILIES = list(PRESCRIBED) + ["hollow", "channel-gains"]


def hermitian64(S):
    """complex128 -> complex64, the lower triangle the exact conjugate of the upper, the diagonal
    real."""
    S = S.astype(np.complex64)
    n = S.shape[-1]
    iu = np.triu_indices(n, 1)
    S[..., iu[1], iu[0]] = S[..., iu[0], iu[1]].conj()
    S[..., np.arange(n), np.arange(n)] = S[..., np.arange(n), np.arange(n)].real
    return S


def truth(S):
    """numpy.linalg.eigh in complex128 of the complex64 matrices, descending."""
    w, V = np.linalg.eigh(S.astype(np.complex128))
    return w[..., ::-1].copy(), V[..., :, ::-1].copy()


@functools.lru_cache(maxsize=None)
def family(name, n, count=COUNT):
    """(S complex64 [count, n, n], w_ref, V_ref, lambda): lambda the prescribed spectrum sorted
    descending, None for the two families that have none."""
    rng = np.random.default_rng(100 * n + FAMILIES.index(name))

    def cn(*s):
        return (rng.standard_normal(s) + 1j * rng.standard_normal(s)) / np.sqrt(2)

    lam = None
    if name in PRESCRIBED:
        lam = PRESCRIBED[name](n)
        assert lam.shape == (n,)
        Q, R = np.linalg.qr(cn(count, n, n))
        d = np.diagonal(R, axis1=-2, axis2=-1)
        Q = Q * (d / np.abs(d))[:, None, :]
        S = (Q * lam) @ np.swapaxes(Q, 1, 2).conj()
        lam = np.sort(lam)[::-1].copy()
    elif name == "hollow":
        G = cn(count, n, n)
        S = (G + np.swapaxes(G, 1, 2).conj()) / 2
        S[:, np.arange(n), np.arange(n)] = 0
    else:  # channel gains
        T = 3 * n
        X = cn(count, T, n)
        g = 10.0 ** rng.uniform(-4, 4, size=(count, n))
        S = np.einsum("mti,mtj->mij", X.conj(), X) / T * g[:, :, None] * g[:, None, :]
    S = hermitian64(S)
    if name == "hollow":
        assert (S[:, np.arange(n), np.arange(n)] == 0).all()
    w, V = truth(S)
    for a in (S, w, V) + (() if lam is None else (lam,)):
        a.setflags(write=False)
    return S, w, V, lam


def check_generator(wref, lam, label):
    """The cast to complex64 moves the prescribed spectrum by at most 1e-6 max |lambda|."""
    e = np.abs(wref - lam).max() / np.abs(lam).max()
    print(f"[{label}] generator: |w_ref - lambda| / max|lambda| {e:.2e} (allowed 1e-6)")
    assert e <= 1e-6


def check_cluster(v, wref, Vref, size, label):
    """sin of the largest principal angle between the span of the `size` leading returned
    vectors and the truth's, against the Davis-Kahan bound 2e-5 / gap of a 1e-5 residual, gap
    the distance from the cluster to the next eigenvalue over max |lambda|."""
    worst = 0.0
    for m in range(v.shape[0]):
        got = np.linalg.qr(v[m, :size].astype(np.complex128).T)[0]  # [n, size]
        ref = Vref[m, :, :size]
        sin = np.linalg.norm(got - ref @ (ref.conj().T @ got), 2)
        gap = (wref[m, size - 1] - wref[m, size]) / np.abs(wref[m]).max()
        worst = max(worst, sin * gap / 2e-5)
    print(f"[{label}] leading {size}-dimensional subspace: worst fraction of the allowed "
          f"2e-5 / gap: {worst:.3f}")
    assert worst <= 1.0


def check_family(name, n, S, w, v, sw, max_sweeps):
    """Everything asserted of one family's result; shared with the CPU restatement's test."""
    _, wref, Vref, lam = family(name, n, S.shape[0])
    label = f"{name} n={n}"
    print(f"[{label}] sweeps mean {np.mean(sw):.2f} max {np.max(sw)} (bound {max_sweeps})")
    if lam is not None:
        check_generator(wref, lam, label)
    check_parity(S, w, v, wref, Vref, label)
    if name == "clustered-top":
        check_cluster(v, wref, Vref, 3, label)
    assert (np.asarray(sw) >= 1).all() and (np.asarray(sw) <= max_sweeps).all()


@pytest.mark.parametrize("n", SPECTRA_N)
@pytest.mark.parametrize("name", FAMILIES)
def test_spectrum_families(gpu_device, name, n):
    from specenh import _lib

    S = family(name, n)[0]
    w, v, sw = run(gpu_device, S, n)
    check_family(name, n, S, w, v, sw, _lib.HERM_EIG_MAX_SWEEPS)


def bits(a):
    return np.ascontiguousarray(a).view(np.float32 if a.dtype == np.complex64 else a.dtype)


@pytest.mark.parametrize("e", [-40, -24, 24, 40])
@pytest.mark.parametrize("n", SCALE_N)
def test_power_of_two_scale_is_bitwise(gpu_device, n, e):
    S = matrices(n, 2 * n)[0]
    f = np.float32(2.0) ** e
    w0, v0, s0 = run(gpu_device, S, 2)
    w1, v1, s1 = run(gpu_device, S * f, 2)
    assert np.isfinite(w0).all() and np.isfinite(w1).all()
    bad_w, bad_v = int((w1 != w0 * f).sum()), int((bits(v1) != bits(v0)).sum())
    bad_s = int((s1 != s0).sum())
    print(f"[n={n} 2^{e}] elements that differ: w {bad_w} of {w0.size}, v {bad_v} of "
          f"{bits(v0).size}, sweeps {bad_s} of {s0.size} (allowed 0)")
    assert bad_w == 0 and bad_v == 0 and bad_s == 0


FACTORS = {"1e-6": 1e-6, "1e-12": 1e-12, "2^-80": 2.0 ** -80, "2^80": 2.0 ** 80}


@pytest.mark.parametrize("factor", list(FACTORS))
@pytest.mark.parametrize("n", SCALE_N)
def test_contract_holds_at_every_scale(gpu_device, n, factor):
    from specenh import _lib

    S = hermitian64(matrices(n, 2 * n)[0].astype(np.complex128) * FACTORS[factor])
    assert np.isfinite(S.view(np.float32)).all()
    wref, Vref = truth(S)
    w, v, sw = run(gpu_device, S, 2)
    print(f"[n={n} x {factor}] sweeps mean {sw.mean():.2f} max {sw.max()}")
    check_parity(S, w, v, wref, Vref, f"n={n} x {factor}")  # asserts that w and v are finite
    assert (sw >= 1).all() and (sw <= _lib.HERM_EIG_MAX_SWEEPS).all()


@pytest.mark.parametrize("navg", [0, 2])
def test_array_modes_scale_is_bitwise(gpu_device, navg):
    """x 2^-12 -> power 2^-24, modes and fraction unchanged: every step from the detrend to the
    Gram product is linear or quadratic in x."""
    from test_csm_gpu import FS, signals

    from specenh import spectral

    x = torch.from_numpy(np.array(signals(2, 5, 9 * 64 + 37))).to(gpu_device)
    kw = dict(k=2, fs=FS, window="hann", nperseg=64, noverlap=48, detrend="linear", navg=navg)
    _, _, est0 = spectral.array_modes(x, **kw)
    _, _, est1 = spectral.array_modes(x * 2.0 ** -12, **kw)
    p0, p1 = est0["power"].cpu().numpy(), est1["power"].cpu().numpy()
    assert np.isfinite(p0).all() and (p0[..., 0] > 0).all()
    bad = {"power": int((p1 != p0 * np.float32(2.0 ** -24)).sum())}
    for name in ("modes", "fraction"):
        a0, a1 = est0[name].cpu().numpy(), est1[name].cpu().numpy()
        assert np.isfinite(bits(a0)).all()
        bad[name] = int((bits(a1) != bits(a0)).sum())
    print(f"[array_modes navg={navg} x 2^-12] elements that differ: {bad} of {p0.size} power "
          f"(allowed 0)")
    assert not any(bad.values())
