/* specenh_nlmeans.h — non-local means denoising of libspecenh.so, an extension of the C-ABI in
 * specenh.h (same error codes and dtype codes) beside the bilateral filter of
 * specenh_bilateral.h. */
#ifndef SPECENH_NLMEANS_H
#define SPECENH_NLMEANS_H

#include "specenh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- non-local means
 * Buades, Coll & Morel 2005, with the weighting of skimage.restoration.denoise_nl_means(
 * image, patch_size, patch_distance, h, fast_mode=True, sigma), the `from skimage import
 * restoration` toolbox of the reference files. For one image u [rows, cols] let
 *   u~(r, c) = u(reflect101(r), reflect101(c))
 * be its extension by reflection without edge repeat (numpy pad(mode="reflect"), applied as
 * often as needed for an image smaller than the halo), P = patch_size (odd), f = P / 2,
 * D = patch_distance. For every pixel x and every shift t in [-D, D]^2 (n = (2D+1)^2 shifts,
 * row-major, the centre included):
 *   d2(x,t) = (1/P^2) sum_{o in [-f,f]^2} (u~(x+o) - u~(x+t+o))^2      uniform patch weights
 *   a(x,t)  = max(d2(x,t) - 2 sigma^2, 0) / h^2
 *   w(x,t)  = exp(-a(x,t))
 *   out(x)  = sum_t w(x,t) u~(x+t) / sum_t w(x,t)
 * One deliberate difference from scikit-image: it skips the shifts with a > 5; here no weight
 * is dropped. A cutoff is a discontinuity that fp32 cannot reproduce against an fp64 truth, and
 * on a GPU skipping saves nothing. The centre shift has w = 1, so the denominator is >= 1.
 * Non-finite input gives unspecified values in the pixels whose windows reach it and nowhere
 * else. D = 0 returns the input bit for bit.
 *
 * Arithmetic is fp32 whatever the dtype: an fp64 image is cast to fp32 on load and the fp32
 * result is cast back on store, so the fp64 call equals the fp32 call on the cast image.
 * The kernel's operations per pixel and shift, each rounded once:
 *   e = one difference, then P^2 terms e*e summed as non-negative terms only: along a patch
 *       row s = e0*e0, s = fma(e, e, s) (P-1 times), then the P row sums added in order
 *       (P-1 additions). No sliding-window subtraction and no integral image: the error of
 *       the sum stays relative to the sum itself;
 *   x = fma(sum, (float)(log2(e) / (P^2 h^2)), -(float)(2 sigma^2 log2(e) / h^2)), max(x, 0);
 *   w = exp2(-x) by the hardware instruction (1 ulp; a result below 2^-126 becomes 0);
 *   sum_w += w; sum_wv = fma(w, v, sum_wv): one chain each in shift order, then one division.
 * Counting roundings relative to a + k, k = 2 sigma^2 / h^2: 2 for the difference (squared),
 * 1 + (P^2 - 1) for the square and the additions (fewer with the fused forms), 2 for the
 * scale and its constant, 1 for the constant 2 sigma^2, 1 for the subtraction: P^2 + 6, within
 * the c_d = P^2 + 8 the criterion uses; the exponential is within c_e = 4 units of 2^-24.
 * Criterion (tests/nlmeans_local.py), with the fp64 quantities a_t, w_t, v_t = u~(x+t),
 * W = sum w_t, q = sum w_t v_t / W and eps = 2^-24:
 *   eta_t = w_t (c_d eps (a_t + k) + c_e eps) + 2^-126
 *   |out(x) - q(x)| <= sum_t eta_t |v_t - q| / (W - sum_t eta_t) + (2n + 3) eps max_t |v_t|
 * at every pixel: the first term is the weights' error, whatever h; the second the two fp32
 * chains and the division, as in specenh_bilateral.h.
 *
 * A pixel's bits depend on its neighbourhood alone, not on the tile it falls in, the batch
 * index, the stride or the run. One workgroup of 256 threads per SPECENH_NLMEANS_TILE_ROWS x
 * SPECENH_NLMEANS_TILE_COLS output tile of one image; parameters travel as kernel arguments:
 * no allocation, no workspace, graph-capturable. */
#define SPECENH_NLMEANS_MAX_PATCH 9
#define SPECENH_NLMEANS_MAX_DISTANCE 15
#define SPECENH_NLMEANS_TILE_ROWS 16
#define SPECENH_NLMEANS_TILE_COLS 64

/* dtype: SPECENH_DTYPE_F32 or _F64. S: device, image b at S + b*stride elements, row-major
 * rows x cols, stride >= rows*cols; out: device, the same layout and stride, must not overlap S.
 * SPECENH_EINVAL: patch_size even or < 1, patch_distance < 0, h not finite or <= 0, sigma not
 * finite or < 0. SPECENH_EUNSUPPORTED: patch_size > SPECENH_NLMEANS_MAX_PATCH, patch_distance >
 * SPECENH_NLMEANS_MAX_DISTANCE, rows or cols of 2^30 or more (the kernel's coordinates are int),
 * or more than 2^31 - 1 tiles an image. batch == 0 succeeds after the checks. */
int specenh_nlmeans(int dtype, const void* S, long long batch, int rows, int cols,
                    long long stride, int patch_size, int patch_distance, double h, double sigma,
                    void* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_NLMEANS_H */
