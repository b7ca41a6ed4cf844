/* specenh_bispectrum.h — the bispectrum and squared bicoherence (whole-shot or
 * block-averaged) of libspecenh.so, an extension of the C-ABI in specenh.h (same error codes,
 * plan object, scaling and detrend codes) beside specenh_spectral.h and specenh_csm.h. */
#ifndef SPECENH_BISPECTRUM_H
#define SPECENH_BISPECTRUM_H

#include <stddef.h>

#include "specenh.h"
#include "specenh_spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- bispectrum, bicoherence
 * Whether three frequencies f1 + f2 = f3 of the signals x, y, z are phase-locked (Kim &
 * Powers 1979): with X_t[k] column t of scipy.signal.spectrogram(s, ..., mode='complex') on a
 * group's slice (rfft(detrend(frame) w) sqrt(scale), no one-sided doubling; the groups of
 * specenh_spectral_groups on the slices of specenh_spectral_mean), for 0 <= k, l < K and
 * k + l <= N/2
 *   B[k][l]  = mean_t X_t[k] Y_t[l] conj(Z_t[k+l])
 *   D[k][l]  = mean_t |X_t[k] Y_t[l]|^2,   E[m] = mean_t |Z_t[m]|^2
 *   b2[k][l] = |B[k][l]|^2 / (D[k][l] E[k+l])          in [0, 1]; 0/0 gives NaN.
 * Elements with k + l > N/2 are written as 0 in both outputs.
 *
 * Two kernels behind one entry point, on one stream: every distinct signal's frames are
 * detrended, windowed and transformed once into the workspace; an accumulate kernel then
 * sums the triple products of each (k, l) tile over the group's frames in ascending order, at
 * most SPECENH_SPECTRAL_CHUNK frames in fp32 before an fp64 accumulator in registers takes
 * over. No allocation at launch (graph-capturable), no atomics: an element is a function of
 * its signals' samples, the plan and navg only, whatever the batch and nbins. With y and z
 * aliasing x (the auto-bispectrum) [k][l] and [l][k] are bitwise equal.
 * nperseg: a power of two in [64, 4096]. */

/* Bytes of workspace specenh_bispectrum needs, never 0 for valid arguments: the spectra of
 * the frames that enter a group, float2 (re, im) [batch][nsignals][frames_used][F],
 *   batch * nsignals * frames_used * F * 8,
 * F = nperseg/2 + 1, frames_used = groups * navg (all frames for navg <= 0), nsignals in
 * 1..3 the number of distinct signals among x, y, z. 0 with the error set when the arguments
 * are invalid. */
size_t specenh_bispectrum_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                          long long nsignals, long long length, long long navg);

/* x, y, z: device fp32, shot b at s + b * s_stride, `length` samples (s_stride >= length).
 * y / z null: the signal is x (its stride is ignored); a y or z that equals another signal
 * in pointer and stride is not transformed again.
 * nbins: K, 1 <= K <= F; K <= 0 means F.
 * Outputs: device, [batch][G][K][K], G = specenh_spectral_groups(frames, navg):
 *   bispec float2 (re, im): B[k][l];
 *   bicoh  fp32: b2[k][l], in fp64 from the unrounded sums.
 * Each may be null, at least one must not be. workspace: device, 16-byte aligned,
 * workspace_bytes >= specenh_bispectrum_workspace_bytes(...) for the distinct signals. */
int specenh_bispectrum(const specenh_stft_plan* plan, const float* x, const float* y,
                       const float* z, long long batch, long long length, long long x_stride,
                       long long y_stride, long long z_stride, long long navg, long long nbins,
                       void* bispec /* float2 [batch][G][K][K] */, float* bicoh,
                       void* workspace, size_t workspace_bytes, void* stream);

/* The accumulate kernel alone on spectra the caller already has: X, Y, Z device float2
 * [batch][frames][nfreq], contiguous (Y / Z null: the spectrum is X), nfreq = F = N/2 + 1 in
 * [1, 2049], the domain k + l <= nfreq - 1. No scaling is applied and no workspace needed.
 * navg, nbins and the outputs as above, G = specenh_spectral_groups(frames, navg). */
int specenh_bispectrum_spectra(const void* X, const void* Y, const void* Z, long long batch,
                               long long frames, long long nfreq, long long navg,
                               long long nbins, void* bispec, float* bicoh, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_BISPECTRUM_H */
