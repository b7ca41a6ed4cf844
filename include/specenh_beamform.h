/* specenh_beamform.h — steered-response spectra of a channel array (Bartlett, Capon, MUSIC):
 * the projection of frame spectra or eigenvectors on steering vectors, of libspecenh.so, an
 * extension of the C-ABI in specenh.h (same error codes, plan object and specenh_last_error)
 * beside specenh_csm.h and specenh_modes.h. */
#ifndef SPECENH_BEAMFORM_H
#define SPECENH_BEAMFORM_H

#include <stddef.h>

#include "specenh.h"
#include "specenh_spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- conventions
 * S_ij = mean_t conj(X_i) X_j, the sign of scipy.signal.csd (specenh_csm.h). A steering vector
 * is a_c(kappa) = exp(i kappa p_c), p_c the position (m) or angle (rad) of channel c, kappa a
 * wavenumber or a mode number. A fluctuation X_c ~ exp(i kappa0 p_c), that is
 * arg S_ij = kappa0 (p_j - p_i), peaks at kappa = kappa0. With |a|^2 = sum_c |a_c|^2:
 *   P_bartlett = sum_ij a_i S_ij conj(a_j) / |a|^4 = mean_t |sum_c conj(a_c) X_c|^2 / |a|^4
 *                (one plane wave of PSD p gives p);
 *   P_capon    = 1 / sum_m |sum_c a_c v_m[c]|^2 / (max(lambda_m, 0) + delta),
 *                delta = loading * sum_m lambda_m / C;
 *   P_music    = |a|^2 / sum_{m >= p} |sum_c a_c v_m[c]|^2   (dimensionless, >= 1),
 * (lambda_m, v_m) the eigenpairs of S, v_m row m of specenh_herm_eig's v. A Capon term whose
 * max(lambda_m, 0) + delta is exactly 0 (no power, no loading) carries weight 0, as in the
 * pseudo-inverse of S: the caller that forms the weights sets it. The last division is IEEE's,
 * so a matrix without any power gives q = 0 and P_capon = 1 / 0 = inf, P_bartlett = 0.
 *
 * All three are one kernel (csrc/steered_power.hip),
 *   q[j][n] = sum_{m < rows} w[j][m] | sum_{c < channels} V[j][m][c] A[t(j)][n][c] |^2,
 * the complex product on the exact-fp32 matrix cores, the rows summed in ascending m, at most
 * SPECENH_SPECTRAL_CHUNK rows in fp32 before an fp64 accumulator in a register takes over,
 * followed by one of the epilogues below; |a_n|^2 = sum_c |A[t][n][c]|^2 is computed from the
 * table in a fixed order. No atomics, no workspace, no allocation at launch (graph-capturable):
 * out[j][n] is a function of V_j, w_j, row n of its table, rows and channels only, not of
 * count, nsteer or j's position. 1 / 0 is inf by IEEE; a non-finite element in V_j or w_j
 * makes the outputs of matrix j non-finite, and of no other matrix. */
#define SPECENH_STEER_MAX_CHANNELS 64
#define SPECENH_STEER_MAX_NSTEER 4096

#define SPECENH_STEER_SUM 0      /* q * scale */
#define SPECENH_STEER_BARTLETT 1 /* q * scale / |a_n|^4 */
#define SPECENH_STEER_INVERSE 2  /* scale / q */
#define SPECENH_STEER_MUSIC 3    /* |a_n|^2 / q */

/* The generic entry. All pointers device.
 *   v  float2 (re, im), 8-byte aligned: matrix j at v + j * v_matrix_stride float2, its row m
 *      at + m * v_row_stride (v_row_stride >= channels, v_matrix_stride >=
 *      (rows - 1) * v_row_stride + channels); rows in [1, 2^30], channels in [1, 64];
 *   w  fp32 [count][rows], or null: all ones;
 *   a  float2 [a_count][nsteer][channels], 8-byte aligned, nsteer in [1, 4096]; matrix j uses
 *      table t(j) = (j / a_inner) % a_count. a_count = 1: one table for every matrix. For
 *      a_count > 1 count must be a multiple of a_count * a_inner (matrices [.., a_count,
 *      a_inner]: a_count = F, a_inner = G is one table per frequency bin of [B][F][G]);
 *   conj_a  non-zero: the product takes conj(A), as the Bartlett form on frame spectra does;
 *   scale, scale_table  the epilogue's factor is scale, times scale_table[t(j)] (fp64
 *      [a_count]) unless that is null;
 *   post  one of SPECENH_STEER_*;
 *   out  fp32 [count][nsteer], every element written.
 * count == 0 returns SPECENH_OK and touches nothing. */
int specenh_steered_power(const void* v, const float* w, const void* a, long long count,
                          long long rows, long long channels, long long nsteer,
                          long long v_matrix_stride, long long v_row_stride, long long a_count,
                          long long a_inner, int conj_a, double scale,
                          const double* scale_table, int post, float* out, void* stream);

/* ---------------------------------------------------------------- fused Bartlett spectrum
 * P_bartlett of every frequency bin and averaging group of a channel array without forming the
 * cross-spectral matrix: the transform kernel of specenh_csm writes every channel's frame
 * spectra to the workspace, the steered-power kernel reads them there in place (rows = the
 * group's frames, conj_a, SPECENH_STEER_BARTLETT, the scale and one-sided doubling of
 * specenh_csm), so that out = a^T S conj(a) / |a|^4 with S from specenh_csm. The slice, scale,
 * detrend and group rules are those of specenh_csm; channels in [1, 64].
 *
 * Bytes of workspace, the same as specenh_csm_workspace_bytes: 0 with the error set when the
 * arguments are invalid. */
size_t specenh_array_spectrum_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                              long long channels, long long length,
                                              long long navg);

/* x: as specenh_csm's. a: device float2, 8-byte aligned, the steering vectors (not their
 * conjugates) [nsteer][channels], or [F][nsteer][channels] with a_per_bin != 0 (one table per
 * frequency bin: broadband delay-and-sum). out: device fp32 [batch][F][G][nsteer].
 * workspace: device, 16-byte aligned, workspace_bytes >=
 * specenh_array_spectrum_workspace_bytes(...). */
int specenh_array_spectrum(const specenh_stft_plan* plan, const float* x, long long batch,
                           long long channels, long long length, long long channel_stride,
                           long long batch_stride, long long navg, const void* a,
                           long long nsteer, int a_per_bin,
                           float* out /* fp32 [batch][F][G][nsteer] */, void* workspace,
                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_BEAMFORM_H */
