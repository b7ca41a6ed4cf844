"""CPU model of top1_kernel_reg's thread map (svd_denoise.hip): which thread owns which element
of the 128 x 128 X, and the two reductions built on it, emulated lane by lane in numpy with
the cross-lane moves the kernel uses (DPP row_ror:8, row_half_mirror, quad_perm;
v_permlane32_swap, v_permlane16_swap; the waves' partial sums in LDS at ppos). U = X Z and
Y = X^T U through the emulated reductions must equal the plain products, and the LDS patterns
of the iteration loop must be conflict-free in the bank model (tools/lds_banks.py)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

N = 128
TID = np.arange(256)
A, C, LANE, W = TID >> 4, TID & 15, TID & 63, TID >> 6


def ppos(i):
    return i ^ ((i >> 3) & 7)


def owned(tid):
    """(rows, columns) of thread tid in register order: rows a + 16 m, columns [h][e]."""
    return (tid >> 4) + 16 * np.arange(8), (4 * (tid & 15) + 64 * np.arange(2)[:, None]
                                            + np.arange(4)[None, :]).ravel()


def rs_dpp(vals, bit, partner):
    """One reduce-scatter step: vals[tid] = (lo, hi) halves; the lane with `bit` set keeps hi."""
    half = vals.shape[1] // 2
    lo, hi = vals[:, :half], vals[:, half:]
    up = bit.astype(bool)[:, None]
    keep, send = np.where(up, hi, lo), np.where(up, lo, hi)
    return keep + send[partner]


def swap(vdst, src, width):
    """v_permlane32_swap (width 32) / v_permlane16_swap (width 16) on 64-lane waves: the upper
    `width` lanes of each 2 * width block of vdst trade with the lower ones of src."""
    nd, ns = vdst.copy(), src.copy()
    upper = (LANE // width) % 2 == 1
    nd[upper] = src[TID[upper] - width]
    ns[~upper] = vdst[TID[~upper] + width]
    return nd, ns


def rs_swap(vals, width):
    half = vals.shape[1] // 2
    nd, ns = swap(vals[:, :half], vals[:, half:], width)
    return nd + ns


def test_every_element_owned_once():
    count = np.zeros((N, N), dtype=int)
    for tid in TID:
        k, i = owned(tid)
        count[np.ix_(k, i)] += 1
    assert np.all(count == 1)
    # a 16-lane group (one a) covers 256 contiguous bytes of a row per chunk
    for h in range(2):
        cols = np.concatenate([owned(t)[1][4 * h:4 * h + 4] for t in range(16)])
        assert np.array_equal(cols, 64 * h + np.arange(64))


def test_xz_reduce_scatter_equals_product():
    rng = np.random.default_rng(0)
    X, Z = rng.standard_normal((N, N)), rng.standard_normal((N, 4))
    acc = np.empty((256, 32))  # [m][p]
    for tid in TID:
        k, i = owned(tid)
        acc[tid] = (X[np.ix_(k, i)] @ Z[i]).ravel()
    row = TID & ~15
    v = rs_dpp(acc, C & 8, row | ((C + 8) & 15))          # row_ror:8
    v = rs_dpp(v, C & 4, (TID & ~7) | (7 - (TID & 7)))     # row_half_mirror
    v = rs_dpp(v, C & 2, TID ^ 2)                          # quad_perm [2, 3, 0, 1]
    v = rs_dpp(v, C & 1, TID ^ 1)                          # quad_perm [1, 0, 3, 2]
    U = np.full((N, 4), np.nan)
    for tid in TID:
        k, p = A[tid] + 16 * (C[tid] >> 1), 2 * (C[tid] & 1)
        assert np.all(np.isnan(U[k, p:p + 2]))
        U[k, p:p + 2] = v[tid]
    np.testing.assert_allclose(U, X @ Z, rtol=1e-12, atol=1e-12)


def test_xtu_reduction_equals_product():
    rng = np.random.default_rng(1)
    X, U = rng.standard_normal((N, N)), rng.standard_normal((N, 4))
    acc = np.empty((256, 32))  # [column 4 h + e][p]
    for tid in TID:
        k, i = owned(tid)
        acc[tid] = (X[np.ix_(k, i)].T @ U[k]).ravel()
    v = rs_swap(rs_swap(acc, 32), 16)  # lane bits 5, 4: two columns x 4 left
    i0 = 64 * (LANE >> 5) + 4 * C + 2 * ((LANE >> 4) & 1)
    sP = np.full((4, N, 4), np.nan)
    for tid in TID:
        for e in range(2):
            slot = ppos(i0[tid] + e)
            assert np.all(np.isnan(sP[W[tid], slot]))
            sP[W[tid], slot] = v[tid, 4 * e:4 * e + 4]
    Y = np.stack([sP[:, ppos(i)].sum(0) for i in range(N)])
    np.testing.assert_allclose(Y, X.T @ U, rtol=1e-12, atol=1e-12)


def test_fp64_row_sum_lands_on_even_lanes():
    """u = X v: 8 row sums per thread, scattered over lane bits 3, 2, 1 and summed over bit 0."""
    rng = np.random.default_rng(2)
    X, v = rng.standard_normal((N, N)), rng.standard_normal(N)
    s = np.empty((256, 8))
    for tid in TID:
        k, i = owned(tid)
        s[tid] = X[np.ix_(k, i)] @ v[i]
    row = TID & ~15
    s = rs_dpp(s, C & 8, row | ((C + 8) & 15))
    s = rs_dpp(s, C & 4, (TID & ~7) | (7 - (TID & 7)))
    s = rs_dpp(s, C & 2, TID ^ 2)
    s = s + s[TID ^ 1]
    u = np.full(N, np.nan)
    for tid in TID[(C & 1) == 0]:
        u[A[tid] + 16 * (C[tid] >> 1)] = s[tid, 0]
    np.testing.assert_allclose(u, X @ v, rtol=1e-12, atol=1e-12)


def test_iteration_loop_lds_patterns_conflict_free():
    from top1_reg_banks import table

    rows = table()
    assert len(rows) >= 12
    for name, instr, extra, cycles in rows:
        if not name.startswith("fp64"):  # the fp64 step runs once per matrix, not per round
            assert extra == 0, (name, instr, extra, cycles)
