/* specenh_kmeans.h — k-means clustering (Lloyd iterations) of libspecenh.so, an extension of
 * the C-ABI in specenh.h (same error codes), the device side of `from sklearn.cluster import
 * KMeans` in the reference files. */
#ifndef SPECENH_KMEANS_H
#define SPECENH_KMEANS_H

#include <stddef.h>

#include "specenh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- one Lloyd iteration
 * Data X[batch][n][d], fp32: point p of item b at X + b*stride + p*ld, ld >= d, stride >= n*ld;
 * any d and ld, odd ones included (no vector loads). Centres C[batch][k][d], contiguous fp32.
 * All arithmetic is fp32. Limits: 1 <= k <= SPECENH_KMEANS_MAX_K, 1 <= d <=
 * SPECENH_KMEANS_MAX_D, n < 2^31; k > n is allowed.
 *
 * Assignment. label(p) = argmin_j s_j(p), s_j = |c_j|^2 - 2 x.c_j (|x|^2 is common to all j and
 * left out), the lowest j among exactly equal fp32 scores; the [n, k] scores are never
 * written. In the order the kernels work:
 *   |c_j|^2: lane l of one wave per centre takes the elements l, l + 64, ... as one chain
 *       v = fma(c, c, v) (ceil(d / 64) roundings), then six butterfly additions over the wave;
 *   x.c_j:   on the matrix cores (v_mfma_f32_32x32x2_f32, fp32 operands and accumulators).
 *       d is walked in chunks of SPECENH_KMEANS_CHUNK = 32; a chunk's products are one
 *       accumulator chain that starts at zero (at most 32 terms), and the chunk's sum is then
 *       added to the running dot product (ceil(d / 32) additions, the first onto zero);
 *   s_j = fma(-2, x.c_j, |c_j|^2), one rounding.
 * Every column j runs the same sequence of operations on its own row of C, so two identical
 * centre rows get identical score bits whatever their index, the tile or the batch item.
 * With T_j = |c_j|^2 + 2 sum_i |x_i c_ji| the error of a score is at most c_s 2^-24 T_j,
 *   c_s(d) = max(min(d, 32) + ceil(d / 32), ceil(d / 64) + 6) + 2
 * (the longer of the two chains, one rounding for a product that the matrix core may round on
 * its own, one for the final fma): c_s(1) = 9 and c_s(d) <= d + 8, far smaller for large d
 * because of the chunks. Hence for the chosen label l and the fp64 optimum j*:
 *   s_l - s_j* <= c_s 2^-24 (T_l + T_j*)                         (tests/kmeans_local.py)
 *
 * Update, given those labels and the input centres C:
 *   counts[b][j]: int32, exact (integer additions only);
 *   sums: onehot(labels)^T X on the matrix cores, the points split into slabs of
 *       L = SPECENH_KMEANS_SLAB (doubled while n needs more than 1024 slabs; a function of n
 *       alone). Within a slab a sum is one accumulator chain in point order (a point of another
 *       cluster adds an exact zero); the S = ceil(n / L) slab partials are then added in slab
 *       order. A cluster of m points therefore passes at most
 *   c_u(n, m) = min(m, L + S)
 *       roundings: |sum - sum64| <= c_u 2^-24 sum_members |x| per entry;
 *   C_new = sum / (float)count, one division; an empty cluster (count 0) keeps its previous
 *       centre bit for bit. This differs from scikit-learn, which relocates an empty cluster;
 *   inertia[b] = sum_p |x_p - c_label(p)|^2: e = x - c, v = fma(e, e, v), non-negative terms
 *       only: per lane a chain over every other point of a slab, six butterfly additions, then
 *       the S * ceil(d / 32) partials in 256 strided chains and an eight-level tree. Relative
 *       error at most c_i 2^-24, c_i(n, d) = 16 + ceil(min(L, n) / 2) + ceil(S ceil(d/32) / 256).
 * No floating-point atomics anywhere: every output's bits depend on the item's data, n, d, k
 * and ld alone, not on the run, the batch index, the batch size or the batch stride.
 *
 * Both calls launch on `stream`, allocate nothing and can be captured into a graph. The
 * workspace holds |c_j|^2, the slab partials and nothing that outlives the call. Algorithmic
 * traffic of one iteration: 2 n d 4 bytes (X is read once by each phase). */
#define SPECENH_KMEANS_MAX_K 256
#define SPECENH_KMEANS_MAX_D 65536
#define SPECENH_KMEANS_TILE 64
#define SPECENH_KMEANS_CHUNK 32
#define SPECENH_KMEANS_SLAB 1024

/* Bytes of workspace either call needs; 0 for arguments the calls would refuse. */
size_t specenh_kmeans_workspace_bytes(long long batch, long long n, int d, int k);

/* labels[batch][n] (int32, contiguous) = argmin_j s_j. X, C, labels, workspace: device.
 * SPECENH_EINVAL: batch or n < 0, d or k < 1, ld < d, stride < n*ld, a null pointer, a
 * workspace below specenh_kmeans_workspace_bytes. SPECENH_EUNSUPPORTED: k, d or n above the
 * limits. batch == 0 or n == 0 succeeds after the shape checks; pointers may then be null. */
int specenh_kmeans_assign(const void* X, long long batch, long long n, int d, long long ld,
                          long long stride, const void* C, int k, void* labels, void* workspace,
                          size_t workspace_bytes, void* stream);

/* Assignment and update in one call: labels as above, C_new[batch][k][d] (may be C itself),
 * counts[batch][k] int32, inertia[batch] fp32, the last against the input centres C. */
int specenh_kmeans_step(const void* X, long long batch, long long n, int d, long long ld,
                        long long stride, const void* C, int k, void* labels, void* C_new,
                        void* counts, void* inertia, void* workspace, size_t workspace_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_KMEANS_H */
