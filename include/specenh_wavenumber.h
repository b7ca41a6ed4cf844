/* specenh_wavenumber.h — the two-point (local) wavenumber-frequency spectrum S(k, f) of
 * libspecenh.so (whole-shot or block-averaged), an extension of the C-ABI in specenh.h (same
 * error codes, plan object, scaling and detrend codes) beside specenh_bispectrum.h. */
#ifndef SPECENH_WAVENUMBER_H
#define SPECENH_WAVENUMBER_H

#include <stddef.h>

#include "specenh.h"
#include "specenh_spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- S(k, f)
 * Which way, and how fast, a fluctuation moves between two channels dx apart (Beall, Kim &
 * Powers 1982): the distribution of the per-frame cross-phase, weighted by power.
 *
 * X_t[f], Y_t[f] are column t of scipy.signal.spectrogram(s, ..., mode='complex') on a
 * group's slice. That is exactly the operand, the groups and the slices of
 * specenh_bispectrum.h and specenh_spectral_mean. The plan supplies window, detrend, scaling
 * and fs; navg follows specenh_spectral_groups.
 *
 * For an even bin count K with 4 <= K <= 256:
 *
 *   c      = conj(X_t[f]) * Y_t[f]            (the sign of scipy.signal.csd: phase of y relative to x)
 *   theta  = atan2(Im c, Re c);  c == 0 -> theta = 0
 *   j      = (rint(theta * K / (2 pi)) + K/2) mod K          j in 0..K-1
 *   w      = o[f] * (|X_t[f]|^2 + |Y_t[f]|^2) / 2            o = 2 for 0 < f < N/2, else 1 (one-sided, as welch)
 *   S[b][g][f][j] = (1/T_g) * sum over the group's frames t with j_t[f] == j of w_t[f]
 *
 * Bin j is centred on theta_j = 2 pi (j - K/2) / K, so the k axis is theta_j / dx, i.e.
 * fftshift(fftfreq(K)) * 2 pi / dx.
 *
 * The bins are centred, not edge-aligned, on purpose. theta = 0 and theta = +-pi are bin
 * centres, and +-pi both fall in j = 0. The DC and Nyquist rows, whose spectra are real, are
 * what take exactly those values. They therefore never sit on an edge that rounding decides.
 *
 * Invariant: sum_j S[b][g][f][j] = (Pxx + Pyy) / 2 of specenh_spectral_mean on the same plan.
 *
 * Two kernels behind one entry point, on one stream: the frames of x and y are detrended,
 * windowed and transformed once into the workspace (the transform of specenh_bispectrum); an
 * accumulate kernel then walks each group's frames in ascending order and builds the
 * histogram in fp64, one private row of K cells per bin f. No allocation at launch
 * (graph-capturable), no atomics, no partial sums in memory: an element is a function of its
 * own pair's samples, the plan, navg and K only, whatever the batch, the shot's position and
 * the strides. Every element of the output is written, zeros included.
 * nperseg: a power of two in [64, 4096]. */

/* Bytes of workspace specenh_wavenumber_spectrum needs, never 0 for valid arguments: the
 * spectra of the frames that enter a group, float2 (re, im) [batch][nsignals][frames_used][F],
 *   batch * nsignals * frames_used * F * 8,
 * F = nperseg/2 + 1, frames_used = groups * navg (all frames for navg <= 0), nsignals 2, or 1
 * when y aliases x in pointer and stride. 0 with the error set when the arguments are
 * invalid. */
size_t specenh_wavenumber_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                          long long nsignals, long long length, long long navg);

/* x, y: device fp32, shot b at s + b * s_stride, `length` samples (s_stride >= length). A y
 * that equals x in pointer and stride is not transformed again (all weight then lies in
 * j = K/2).
 * nk: K, even, 4 <= K <= 256.
 * skf: device fp32 [batch][G][F][nk], G = specenh_spectral_groups(frames, navg).
 * workspace: device, 16-byte aligned, workspace_bytes >=
 * specenh_wavenumber_workspace_bytes(...) for the distinct signals. */
int specenh_wavenumber_spectrum(const specenh_stft_plan* plan, const float* x, const float* y,
                                long long batch, long long length, long long x_stride,
                                long long y_stride, long long navg, long long nk,
                                float* skf /* [batch][G][F][nk] */, void* workspace,
                                size_t workspace_bytes, void* stream);

/* The accumulate kernel alone on spectra the caller already has: X, Y device float2
 * [batch][frames][nfreq], contiguous, nfreq in [1, 2049]. No scaling and no one-sided doubling
 * is applied, so w = (|X|^2 + |Y|^2) / 2, and no workspace is needed. navg, nk and skf
 * [batch][G][nfreq][nk] as above, G = specenh_spectral_groups(frames, navg). */
int specenh_wavenumber_spectra(const void* X, const void* Y, long long batch, long long frames,
                               long long nfreq, long long navg, long long nk, float* skf,
                               void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_WAVENUMBER_H */
