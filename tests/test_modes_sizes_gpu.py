"""GPU checks of the batched Hermitian eigensolver (csrc/herm_eig.hip) at every size it accepts.

The launch shape follows from n: the padded size P = n rounded up to even, the row stride S
(a 32-entry table), L = min(64 / (P / 2), P) lanes per pair, the unroll U (8 where a lane has
more than 4 elements a pass), the matrices per workgroup (as many as fit 64 KiB of LDS, 4 at
most) and 64 - L P / 2 idle lanes. From specenh_herm_eig's own arithmetic the sizes fall into
these launch classes (the pass loop of a lane goes round ceil(P / (L U)) times; the last trip is
partly filled wherever L U does not divide P, which is where the clamped reads and the k < P
write guard act):

| U | trips of the pass loop per lane | matrices per workgroup | n      |
|---|---------------------------------|------------------------|--------|
| 4 | 1                               | 4                      | 2..20  |
| 8 | 1                               | 4                      | 21..28 |
| 8 | 1                               | 3                      | 29..32 |
| 8 | 2                               | 3                      | 33..36 |
| 8 | 2                               | 2                      | 37..42 |
| 8 | 3                               | 1                      | 43..48 |
| 8 | 4                               | 1                      | 49..64 |

Every n in 2..64 runs the whole 1e-5 contract of test_modes_gpu.check_parity on 37 matrices
(not a multiple of any matrices-per-workgroup), full rank (T = 2 n) and rank deficient
(T = max(1, n // 3)), all n eigenvectors emitted. For every odd n the padded row and column are
pinned against the even-size call on the same matrix bordered with zeros.

Each test prints measured against allowed (pytest -s); DESIGN.md §5.9 records the values."""
import numpy as np
import pytest

from test_modes_gpu import M, TOL, check_parity, matrices, run

pytestmark = pytest.mark.gpu

SIZES = list(range(2, 65))


def launch_class(n):
    """The row of the table above, as 'U/trips/matrices per workgroup' (for the printed record;
    restated from the arithmetic of specenh_herm_eig with its pad table)."""
    pad = [1, 2, 3, 2, 4, 2, 4, 2, 2, 2, 4, 2, 2, 1, 4, 4,
           3, 1, 4, 3, 1, 2, 4, 2, 4, 2, 4, 2, 4, 2, 4, 2]
    P = n + (n & 1)
    S = P + pad[P // 2 - 1]
    L = min(64 // (P // 2), P)
    U = 8 if -(-P // L) > 4 else 4
    lds = (16 * P * S + 512 + 15) // 16 * 16
    return f"U{U}/{-(-P // (L * U))}/{max(1, min(4, 65536 // lds))}"


def test_launch_classes_of_the_table():
    """The docstring's table is what launch_class computes (no GPU work)."""
    rows = {"U4/1/4": (2, 20), "U8/1/4": (21, 28), "U8/1/3": (29, 32), "U8/2/3": (33, 36),
            "U8/2/2": (37, 42), "U8/3/1": (43, 48), "U8/4/1": (49, 64)}
    for n in SIZES:
        lo, hi = rows[launch_class(n)]
        assert lo <= n <= hi


@pytest.mark.parametrize("rank", ["full", "deficient"])
@pytest.mark.parametrize("n", SIZES)
def test_every_size(gpu_device, n, rank):
    from specenh import _lib

    T = 2 * n if rank == "full" else max(1, n // 3)
    S, wref, Vref = matrices(n, T)
    assert S.shape == (M, n, n)
    w, v, sw = run(gpu_device, S, n)
    label = f"n={n} T={T} {launch_class(n)}"
    print(f"[{label}] sweeps mean {sw.mean():.2f} max {sw.max()} "
          f"(bound {_lib.HERM_EIG_MAX_SWEEPS})")
    check_parity(S, w, v, wref, Vref, label)
    assert (sw >= 1).all() and (sw <= _lib.HERM_EIG_MAX_SWEEPS).all()
    if rank == "full":
        assert (sw < _lib.HERM_EIG_MAX_SWEEPS).all()


@pytest.mark.parametrize("n", [n for n in SIZES if n % 2], ids=lambda n: f"{n}in{n + 1}")
def test_odd_size_against_zero_bordered_even_size(gpu_device, n):
    """S (odd n, full rank) and [[S, 0], [0, 0]] (n + 1): the even-size call returns S's
    eigenvalues and one more, an exact 0. The kernel pads an odd matrix to that same bordered
    matrix, so a padded row or column that is not zero shows here."""
    S, wref, _ = matrices(n, 2 * n)
    big = np.zeros((M, n + 1, n + 1), np.complex64)
    big[:, :n, :n] = S
    w, _, sw = run(gpu_device, S, 0)
    wb, _, swb = run(gpu_device, big, 0)
    assert np.isfinite(w).all() and np.isfinite(wb).all()
    scale = np.abs(wref).max(axis=1)
    shared = np.empty_like(w)
    for m in range(M):
        zero = np.flatnonzero(wb[m] == 0)
        assert zero.size >= 1, f"matrix {m}: no exact 0 among the eigenvalues of the bordered one"
        shared[m] = np.delete(wb[m], zero[0])
    e = (np.abs(shared - w).max(axis=1) / scale).max()
    e_ref = (np.abs(w - wref).max(axis=1) / scale).max()
    print(f"[n={n} in {n + 1}] |w_even - w_odd|/l1 {e:.2e}  |w_odd - w_ref|/l1 {e_ref:.2e} "
          f"(allowed {TOL:.0e} each), bitwise equal: {np.array_equal(shared, w)}, "
          f"sweeps equal: {np.array_equal(sw, swb)}")
    assert e <= TOL and e_ref <= TOL
