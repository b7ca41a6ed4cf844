/* specenh_correlation.h — the block-averaged lagged cross-correlation of two channels of
 * libspecenh.so (whole-shot or per block of frames), the time-domain counterpart of
 * specenh_spectral_mean: an extension of the C-ABI in specenh.h (same error codes, plan object
 * and stream argument) beside specenh_wavenumber.h. */
#ifndef SPECENH_CORRELATION_H
#define SPECENH_CORRELATION_H

#include <stddef.h>

#include "specenh.h"
#include "specenh_spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- cross-correlation
 * The time delay between two channels (the lag of the peak; dx / tau is the velocity) and the
 * correlation time (the width of the auto-correlation), per block of frames.
 *
 * Frames, groups, detrend and window are exactly those of specenh_spectral_mean and
 * specenh_wavenumber_spectrum: frame t is samples [t hop, t hop + N), hop = N - noverlap,
 * detrended (none, constant or linear) and multiplied by the plan's window; navg follows
 * specenh_spectral_groups (navg <= 0: one group of all T frames; navg >= 1: G = T / navg
 * groups of navg consecutive frames, the leftover frames dropped). The plan's fs and scaling
 * are not used: there is no spectral scaling.
 *
 * With x_t, y_t the detrended, windowed frames and a maximum lag 0 <= M <= N - 1:
 *
 *   r_t[m]      = sum_n x_t[n] * y_t[n + m]       m = -M .. M, terms outside [0, N) are zero
 *               = scipy.signal.correlate(y_t, x_t, 'full')[N - 1 + m]
 *   R[b][g][m]  = (1/T_g) * sum over the group's frames t of r_t[m]
 *   Ex[b][g]    = (1/T_g) * sum_t sum_n x_t[n]^2                    (Ey likewise)
 *   rho[b][g][m] = R[b][g][m] / sqrt(Ex * Ey),   defined as 0 where Ex * Ey == 0
 *
 * Sign: y[n] = x[n - d] peaks at m = +d, so a positive lag means y lags x (the convention of
 * the CSD, whose phase is that of y relative to x). R is in signal units squared; rho is
 * dimensionless, |rho| <= 1. This is the linear correlation (every frame zero-padded to 2N),
 * not the circular one that the inverse transform of an averaged CSD would give.
 *
 * The cross-spectra conj(X_t) Y_t of a group's frames (N + 1 bins of the padded frames) are
 * summed on the chip in fp32 over chunks of at most SPECENH_SPECTRAL_CHUNK frames, the chunk
 * sums are added in fp64 in ascending order, and one inverse real transform per group yields
 * the lags; the energies are summed in the time domain in fp64. No per-frame spectrum reaches
 * memory. No allocation at launch (graph-capturable on one stream), no atomics: an element is
 * a function of its own pair's samples, the plan, navg, maxlag and mode only, whatever the
 * batch, the shot's position and the strides. Every element of the outputs is written.
 * nperseg: a power of two in [64, 2048]; 4096 returns SPECENH_EUNSUPPORTED (the padded
 * transform would be 8192 points). */

#define SPECENH_CORR_RAW 0   /* out = R */
#define SPECENH_CORR_COEFF 1 /* out = rho */

/* Bytes of workspace specenh_correlation needs: 0 when every group is a single chunk of at
 * most SPECENH_SPECTRAL_CHUNK frames, else one record per chunk,
 *   batch * groups * chunks_per_group * (nperseg + 3) * 8
 * (nperseg + 1 float2 bins and two fp64 energies). Also 0, with the error set, when the
 * arguments are invalid. */
size_t specenh_correlation_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                           long long length, long long navg, long long maxlag);

/* x, y: device fp32, shot b at s + b * s_stride, `length` samples (s_stride >= length). A y
 * that equals x in pointer and stride is loaded and transformed once (the auto-correlation).
 * maxlag: M, 0 <= M <= nperseg - 1. mode: SPECENH_CORR_RAW or SPECENH_CORR_COEFF.
 * out: device fp32 [batch][G][2 M + 1], lag m at index m + M,
 * G = specenh_spectral_groups(frames, navg).
 * energies: device fp32 [batch][G][2] = (Ex, Ey), or NULL.
 * workspace: device, 16-byte aligned, workspace_bytes >=
 * specenh_correlation_workspace_bytes(...); may be NULL when that is 0. */
int specenh_correlation(const specenh_stft_plan* plan, const float* x, const float* y,
                        long long batch, long long length, long long x_stride,
                        long long y_stride, long long navg, long long maxlag, int mode,
                        float* out /* [batch][G][2 M + 1] */,
                        float* energies /* [batch][G][2], may be NULL */, void* workspace,
                        size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_CORRELATION_H */
