"""The method of csrc/herm_eig.hip on the CPU (no GPU): oracle/herm_eig.py, its plain numpy
restatement (fp32 storage, fp64 angles, the kernel's skip rule, round-robin rounds, the sweep
bound, the output conventions), held to the contract the GPU tests hold the kernel to, on one
matrix of every spectrum family of tests/test_modes_spectra_gpu.py and on the 2^+-40 scalings.
This is the standing proof that those inputs are fair to the method: where the kernel misses
the contract on one of them, the fault is the kernel's.

Each test prints measured against allowed (pytest -s); DESIGN.md §5.9 records the values."""
import numpy as np
import pytest

from oracle import herm_eig as oracle
from test_modes_gpu import check_parity, matrices
from test_modes_spectra_gpu import FAMILIES, bits, check_family, family


def test_constants_match_the_library():
    from specenh import _lib

    assert oracle.MAX_SWEEPS == _lib.HERM_EIG_MAX_SWEEPS
    assert oracle.MAX_N == _lib.HERM_EIG_MAX_N


@pytest.mark.parametrize("P", [2, 4, 6, 34, 64])
def test_round_robin_meets_every_pair_once(P):
    seen = set()
    for rnd in range(P - 1):
        a, b = oracle.round_pairs(P, rnd)
        assert (a < b).all() and sorted(np.concatenate([a, b])) == list(range(P))
        seen |= set(zip(a.tolist(), b.tolist()))
    assert len(seen) == P * (P - 1) // 2


@pytest.mark.parametrize("n", [8, 33])
@pytest.mark.parametrize("name", FAMILIES)
def test_method_on_spectrum_families(name, n):
    S = family(name, n, 1)[0]
    w, v, sw = oracle.herm_eig_batch(S)
    check_family(name, n, S, w, v, sw, oracle.MAX_SWEEPS)


@pytest.mark.parametrize("n", [5, 33])
def test_method_under_power_of_two_scale(n):
    """2^+-40: the eigenvalues scale exactly, the vectors and the sweep count are the same bits,
    and the contract holds at each scale."""
    S, wref, Vref = matrices(n, 2 * n, count=1)
    w0, v0, s0 = oracle.herm_eig_batch(S, 2)
    check_parity(S, w0, v0, wref, Vref, f"restatement n={n}")
    assert 1 <= s0[0] < oracle.MAX_SWEEPS
    for e in (-40, 40):
        f = np.float32(2.0) ** e
        w1, v1, s1 = oracle.herm_eig_batch(S * f, 2)
        check_parity(S * f, w1, v1, wref * float(f), Vref, f"restatement n={n} x 2^{e}")
        assert np.array_equal(w1, w0 * f) and np.array_equal(bits(v1), bits(v0))
        assert np.array_equal(s1, s0)


def test_conventions_and_edges():
    """Diagonal input is answered exactly in one sweep, a zero matrix with the unit vectors,
    a non-finite element with NaN and 0 sweeps; the lower triangle is never read."""
    d = np.array([0.5, -2.0, 3.0, 1.0, 0.0], np.float32)
    w, v, sw = oracle.herm_eig(np.diag(d).astype(np.complex64))
    order = np.argsort(-d, kind="stable")
    assert np.array_equal(w, d[order]) and sw == 1
    assert np.array_equal(v, np.eye(5, dtype=np.complex64)[order])
    w, v, sw = oracle.herm_eig(np.zeros((3, 3), np.complex64))
    assert (w == 0).all() and np.array_equal(v, np.eye(3, dtype=np.complex64)) and sw == 1
    S = np.array(matrices(5, 4, count=1)[0][0])
    ref = oracle.herm_eig(S, 2)
    S[np.tril_indices(5, -1)] = complex("nan+nanj")
    got = oracle.herm_eig(S, 2)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ref[:2], got[:2]))
    S[1, 4] = np.inf
    w, v, sw = oracle.herm_eig(S, 2)
    assert np.isnan(w).all() and np.isnan(v.real).all() and v.shape == (2, 5) and sw == 0
