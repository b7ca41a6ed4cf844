"""ORACLE (test infrastructure only): the method of the batched Hermitian eigensolver.

A plain numpy restatement of csrc/herm_eig.hip, one matrix at a time, every rotation of a
round applied at once as the kernel's lanes do:
  * A and V stored as float32 real and imaginary parts, P = n rounded up to even, the padded
    row and column zero; only the upper triangle and the real diagonal of the input are read;
  * cyclic Jacobi in the round-robin ordering: pair j of a round is the players j and
    P - 1 - j, player 0 fixed, player k > 0 at position 1 + (k - 1 + round) mod (P - 1);
  * for a_pq = r e^{i phi}: J = diag(1, e^{-i phi}) [[c, s], [-s, c]], (c, s) the real Jacobi
    angle of [[a_pp, r], [r, a_qq]] in float64, rounded to float32 with s e^{i phi} and
    c e^{i phi}; A <- J^H A J as a row pass then a column pass, V <- V J; the pair's 2 x 2
    block is stored as 0 and the float64 diagonal a_pp - t r, a_qq + t r;
  * a pair is skipped when |a_pq| <= eps max(sqrt|a_pp a_qq|, 16 eps d_max), eps = 2^-24,
    d_max the largest |a_ii| of the input; the matrix stops after a sweep without a rotation
    and after MAX_SWEEPS sweeps in any case;
  * output conventions: eigenvalues descending (stable by index), eigenvectors as rows, unit
    2-norm, the component of largest modulus (lowest index on ties) real positive.
A non-finite input element is answered with NaN and 0 sweeps.

The float32 products are rounded one operation at a time (numpy does not contract them into
fused multiply-adds as the compiler may), so the restatement is the method, not a bit-exact
model of the kernel: tests/test_modes_oracle_cpu.py holds it to the same 1e-5 contract, which
shows that an input is fair to the method whatever the kernel does with it.
"""
from __future__ import annotations

import numpy as np

MAX_SWEEPS = 16  # SPECENH_HERM_EIG_MAX_SWEEPS
MAX_N = 64       # SPECENH_HERM_EIG_MAX_N
EPS = 2.0 ** -24

_F = np.float32


def round_pairs(P: int, rnd: int):
    """The P / 2 disjoint index pairs (a < b) that round ``rnd`` of a sweep rotates."""
    j = np.arange(P // 2)
    kA, kB = j, P - 1 - j
    a = np.where(kA == 0, 0, 1 + (kA - 1 + rnd) % (P - 1))
    b = 1 + (kB - 1 + rnd) % (P - 1)
    return np.minimum(a, b), np.maximum(a, b)


def _rotate(xr, xi, yr, yi, c, s, ser, sei, cer, cei):
    """(c x - y se, s x + y ce) with complex y * z = (yr zr - yi zi, yr zi + yi zr), every
    operation rounded to float32."""
    p1r, p1i = yr * ser - yi * sei, yr * sei + yi * ser
    p2r, p2i = yr * cer - yi * cei, yr * cei + yi * cer
    return c * xr - p1r, c * xi - p1i, s * xr + p2r, s * xi + p2i


def herm_eig(a, k=None, max_sweeps=MAX_SWEEPS):
    """One Hermitian matrix ``a[n, n]`` (cast to complex64) -> (w float32 [n] descending,
    v complex64 [k, n] eigenvectors as rows, sweeps)."""
    a = np.asarray(a).astype(np.complex64)
    n = a.shape[-1]
    if a.shape != (n, n) or not 2 <= n <= MAX_N:
        raise ValueError(f"a must be [n, n] with n in [2, {MAX_N}]")
    k = n if k is None else int(k)
    if not 0 <= k <= n:
        raise ValueError(f"k must be in [0, {n}]")
    iu = np.triu_indices(n, 1)
    dg = np.arange(n)
    if not (np.isfinite(a.real[dg, dg]).all() and np.isfinite(a[iu].view(_F)).all()):
        return (np.full(n, np.nan, _F), np.full((k, n), complex("nan+nanj"), np.complex64), 0)

    P = n + (n & 1)
    Ar, Ai = np.zeros((P, P), _F), np.zeros((P, P), _F)
    Ar[dg, dg] = a.real[dg, dg]
    Ar[iu], Ai[iu] = a.real[iu], a.imag[iu]
    Ar[iu[1], iu[0]], Ai[iu[1], iu[0]] = a.real[iu], -a.imag[iu]
    Vr, Vi = np.eye(P, dtype=_F), np.zeros((P, P), _F)
    dfloor = 16.0 * EPS * float(np.abs(Ar[dg, dg]).max())

    sweep = 0
    with np.errstate(all="ignore"):
        while sweep < max_sweeps:
            rotated = False
            for rnd in range(P - 1):
                p, q = round_pairs(P, rnd)
                haa, hbb = Ar[p, p].astype(np.float64), Ar[q, q].astype(np.float64)
                hx, hy = Ar[p, q].astype(np.float64), Ai[p, q].astype(np.float64)
                r = np.sqrt(hx * hx + hy * hy)
                thr = EPS * np.maximum(np.sqrt(np.abs(haa * hbb)), dfloor)
                rot = ~(r <= thr)
                if not rot.any():
                    continue
                rotated = True
                p, q, haa, hbb, hx, hy, r = (z[rot] for z in (p, q, haa, hbb, hx, hy, r))
                tau = (hbb - haa) / (2.0 * r)
                tt = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                cd = 1.0 / np.sqrt(1.0 + tt * tt)
                sd = tt * cd
                ex, ey = hx / r, hy / r
                c, s = cd.astype(_F), sd.astype(_F)
                ser, sei = (sd * ex).astype(_F), (sd * ey).astype(_F)
                cer, cei = (cd * ex).astype(_F), (cd * ey).astype(_F)
                dpp, dqq = (haa - tt * r).astype(_F), (hbb + tt * r).astype(_F)
                # row pass: rows p, q of A <- J^H A
                col = lambda z: z[:, None]  # noqa: E731
                nar, nai, nbr, nbi = _rotate(Ar[p], Ai[p], Ar[q], Ai[q], col(c), col(s),
                                             col(ser), col(sei), col(cer), col(cei))
                Ar[p], Ai[p], Ar[q], Ai[q] = nar, nai, nbr, nbi
                # column pass: columns p, q of A <- A J and V <- V J (conjugated factors)
                for Xr, Xi in ((Ar, Ai), (Vr, Vi)):
                    nar, nai, nbr, nbi = _rotate(Xr[:, p], Xi[:, p], Xr[:, q], Xi[:, q], c, s,
                                                 ser, -sei, cer, -cei)
                    Xr[:, p], Xi[:, p], Xr[:, q], Xi[:, q] = nar, nai, nbr, nbi
                Ar[p, p], Ar[q, q] = dpp, dqq
                Ar[p, q] = Ar[q, p] = 0
                Ai[p, p] = Ai[q, q] = Ai[p, q] = Ai[q, p] = 0
            sweep += 1
            if not rotated:
                break

        d = Ar[dg, dg]
        # descending, stable by index; a NaN (from overflow) compares false and stays put
        rank = np.array([int(((d > d[i]) | ((d == d[i]) & (dg < i))).sum()) for i in range(n)])
        order = np.zeros(n, np.int64)
        w = np.zeros(n, _F)
        order[rank], w[rank] = dg, d
        v = np.zeros((k, n), np.complex64)
        for row in range(k):
            zx = Vr[:n, order[row]].astype(np.float64)
            zy = Vi[:n, order[row]].astype(np.float64)
            m2 = zx * zx + zy * zy
            bi = int(np.argmax(m2))  # the lowest index on ties
            am, inv = np.sqrt(m2[bi]), 1.0 / np.sqrt(m2.sum())
            px, py = zx[bi] / am, -zy[bi] / am
            o = ((zx * px - zy * py) * inv).astype(_F) + 1j * ((zx * py + zy * px) * inv).astype(_F)
            o[bi] = _F(am * inv)
            v[row] = o
    return w, v, sweep


def herm_eig_batch(a, k=None, max_sweeps=MAX_SWEEPS):
    """``a[m, n, n]`` -> (w [m, n], v [m, k, n], sweeps [m])."""
    out = [herm_eig(x, k, max_sweeps) for x in a]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            np.array([o[2] for o in out], np.int32))
