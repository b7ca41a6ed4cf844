/* specenh_modes.h — mode decomposition of a channel array: the batched eigendecomposition of
 * small complex Hermitian matrices (the cross-spectral matrices of specenh_csm.h) of
 * libspecenh.so, an extension of the C-ABI in specenh.h (same error codes and
 * specenh_last_error). */
#ifndef SPECENH_MODES_H
#define SPECENH_MODES_H

#include <stddef.h>

#include "specenh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- Hermitian eigensolver
 * Cyclic Jacobi in the round-robin (tournament) ordering, one wave per matrix, the matrix and
 * the accumulated eigenvectors in LDS (csrc/herm_eig.hip). For a pair (p, q) with
 * a_pq = r e^{i phi} the rotation is J = diag(1, e^{-i phi}) [[c, s], [-s, c]], (c, s) the real
 * Jacobi angle of [[a_pp, r], [r, a_qq]] in fp64; A <- J^H A J, V <- V J. A pair is skipped
 * when |a_pq| <= eps max(sqrt|a_pp a_qq|, 16 eps d_max), eps = 2^-24, d_max the largest
 * diagonal modulus of the input; a matrix stops after a sweep without a rotation, and after
 * SPECENH_HERM_EIG_MAX_SWEEPS sweeps whatever its content: no input makes the kernel spin.
 *
 * Only the upper triangle (i <= j) and the real part of the diagonal are read. A matrix with
 * a non-finite element among those gives all-NaN w and v (and 0 sweeps) for that matrix
 * alone. Eigenvalues descend (ties by index) and are not clamped at 0. Eigenvector m is row m
 * of v (numpy.linalg.eigh's V[:, m] of the same order), of unit 2-norm, its component of
 * largest modulus (lowest index on ties) real positive with imaginary part exactly 0. An
 * all-zero matrix gives w = 0 and v[m] = e_m.
 *
 * No workspace, no allocation at launch (graph-capturable), no atomics: a matrix's outputs
 * are a function of that matrix, n and nothing else (not of count, k or its position). */
#define SPECENH_HERM_EIG_MAX_N 64
#define SPECENH_HERM_EIG_MAX_SWEEPS 16

/* a: device float2 (re, im) [count][n][n], matrix m at a + m * matrix_stride float2
 * (matrix_stride >= n * n), 8-byte aligned. Outputs: device;
 *   w      fp32 [count][n], or null;
 *   v      float2 [count][k][n], 8-byte aligned; null iff k == 0;
 *   sweeps int [count], the sweeps each matrix ran, or null.
 * At least one output must be requested. count == 0 returns SPECENH_OK and touches nothing. */
int specenh_herm_eig(const void* a, long long count, long long n, long long matrix_stride,
                     long long k, float* w, void* v, int* sweeps, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_MODES_H */
