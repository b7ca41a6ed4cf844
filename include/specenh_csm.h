/* specenh_csm.h — the cross-spectral matrix and coherence matrix of a channel array
 * (whole-shot or block-averaged) of libspecenh.so, an extension of the C-ABI in specenh.h
 * (same error codes, plan object, scaling and detrend codes) beside specenh_spectral.h. */
#ifndef SPECENH_CSM_H
#define SPECENH_CSM_H

#include <stddef.h>

#include "specenh.h"
#include "specenh_spectral.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- cross-spectral matrix
 * What mode analysis on a diagnostic array (ECE, BES, interferometer chords) is read from:
 * per frequency and averaging group the Hermitian matrix S[i][j] = mean_t conj(X_i) X_j of
 * all channel pairs, and the coherence matrix |S_ij|^2 / (S_ii S_jj). Element [i][j] is what
 * scipy.signal.csd(s_i, s_j, ..., average='mean') gives on the group's slice of channels i
 * and j: the slice identity, scale, one-sided doubling and detrend handling of
 * specenh_spectral_mean (specenh_spectral.h), the groups of specenh_spectral_groups.
 *
 * Two kernels behind one entry point, on one stream: every channel's frames are detrended,
 * windowed and transformed once into the workspace; a Gram kernel on the fp32 matrix cores
 * then sums conj(X_i) X_j over each group's frames in ascending order, at most
 * SPECENH_SPECTRAL_CHUNK frames in fp32 before an fp64 accumulator in registers takes over.
 * No allocation at launch (graph-capturable), no atomics: every output is a function of
 * (x, plan, navg) only, whatever the batch. nperseg: a power of two in [64, 4096].
 * Channels: 2 .. SPECENH_CSM_MAX_CHANNELS (one channel is specenh_spectral_mean's pxx). */
#define SPECENH_CSM_MAX_CHANNELS 64

/* Bytes of workspace specenh_csm needs, never 0 for valid arguments: the spectra of the
 * frames that enter a group, float2 (re, im) [batch][F][frames_used][channels],
 *   batch * F * frames_used * channels * 8,
 * F = nperseg/2 + 1, frames_used = groups * navg (all frames for navg <= 0).
 * 0 with the error set when the arguments are invalid. */
size_t specenh_csm_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                   long long channels, long long length, long long navg);

/* x: device fp32, channel c of shot b at x + b*batch_stride + c*channel_stride, `length`
 * samples (channel_stride >= length, batch_stride >= channels*channel_stride).
 * Outputs: device, [batch][F][G][channels][channels], each channels x channels matrix
 * contiguous, G = specenh_spectral_groups(frames, navg):
 *   csm  float2 (re, im): S[i][j]; the diagonal's imaginary part is exactly 0 and [j][i] is
 *        the exact conjugate of [i][j];
 *   coh  fp32: |S_ij|^2 / (S_ii S_jj) in fp64 from the unrounded sums (0/0 gives NaN).
 * Each may be null, at least one must not be. workspace: device, 16-byte aligned,
 * workspace_bytes >= specenh_csm_workspace_bytes(...). */
int specenh_csm(const specenh_stft_plan* plan, const float* x, long long batch,
                long long channels, long long length, long long channel_stride,
                long long batch_stride, long long navg,
                void* csm /* float2 [batch][F][G][C][C] */, float* coh, void* workspace,
                size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_CSM_H */
