/* specenh_spectral.h — time-averaged spectra (Welch PSD, averaged cross-spectral density,
 * magnitude-squared coherence, whole-shot or block-averaged) of libspecenh.so, an extension
 * of the C-ABI in specenh.h (same error codes, plan object, scaling and detrend codes). */
#ifndef SPECENH_SPECTRAL_H
#define SPECENH_SPECTRAL_H

#include <stddef.h>

#include "specenh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- averaged spectra
 * What the interferometer comparison of two chords is read from (the reference's
 * interferometer/crosspowerspec.py; scipy.signal.welch / csd / coherence with average='mean'
 * are the specification). One fused launch: frames are transformed and summed on the chip,
 * no per-frame spectrum goes to memory. The launch takes a specenh_stft_plan and uses its
 * window, nperseg, noverlap, fs, scaling and detrend (eps unused). nperseg: a power of two
 * in [64, 4096]. No allocation at launch (graph-capturable), no atomics: every output is a
 * function of (x, y, plan, navg) only, whatever the batch. */

/* Frames summed in fp32 before a partial goes to fp64 (the chunk). Groups longer than this
 * take the workspace; the split of a group into chunks depends on (frames, navg) only. */
#define SPECENH_SPECTRAL_CHUNK 32

/* Averaging groups over `frames` = specenh_stft_frames(...) frames:
 *   navg <= 0: 1 (all frames, scipy's welch / csd / coherence);
 *   navg >= 1: frames / navg groups of navg consecutive frames, group g = frames
 *              g*navg .. g*navg + navg - 1; the trailing frames % navg frames are dropped.
 * frames < 1 or navg > frames: SPECENH_EINVAL. */
long long specenh_spectral_groups(long long frames, long long navg);

/* Bytes of workspace specenh_spectral_mean needs: 0 when every group fits in one chunk
 * (the workspace pointer may then be null), else 16 bytes per (signal, group, chunk, bin).
 * 0 with the error set when the arguments are invalid. */
size_t specenh_spectral_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                        long long length, long long navg);

/* Replaces, per signal pair and group g (the slice s = x[g*navg*hop : g*navg*hop +
 * (navg-1)*hop + nperseg], the whole signal for navg <= 0),
 *   f, Pxx = scipy.signal.welch(s_x, ...)      f, Pyy = scipy.signal.welch(s_y, ...)
 *   f, Pxy = scipy.signal.csd(s_x, s_y, ...)   f, Cxy = scipy.signal.coherence(s_x, s_y, ...)
 * Per frame, as _spectral_helper(x, y, mode='psd'): detrend, window, rfft, Pxx = |X|^2 scale,
 * Pyy = |Y|^2 scale, Pxy = conj(X) Y scale, bins 1 .. nperseg/2 - 1 doubled; the mean over
 * the group's frames; coh = |Pxy|^2 / (Pxx Pyy) (0/0 gives NaN, as numpy does).
 * x, y: device fp32, signal b at x + b*x_stride (y + b*y_stride), `length` samples; y may be
 * null (Welch of x alone: only pxx may then be asked for). Outputs: device, frequency-major
 * [batch][F][G], F = nperseg/2 + 1, G = specenh_spectral_groups(frames, navg); pxx, pyy, coh
 * fp32, pxy float2 (re, im); each may be null, at least one must not be. workspace: device,
 * specenh_spectral_workspace_bytes(...) bytes, 16-byte aligned (with y null the first quarter
 * is used). */
int specenh_spectral_mean(const specenh_stft_plan* plan, const float* x, const float* y,
                          long long batch, long long length, long long x_stride,
                          long long y_stride, long long navg, float* pxx, float* pyy,
                          void* pxy /* float2 [batch][F][G] */, float* coh, void* workspace,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_SPECTRAL_H */
