/* specenh_stft_complex.h — the complex STFT / inverse STFT entry points of libspecenh.so,
 * an extension of the C-ABI in specenh.h (same error codes, plan object, scaling and detrend
 * codes; include specenh.h first or let this header do it). */
#ifndef SPECENH_STFT_COMPLEX_H
#define SPECENH_STFT_COMPLEX_H

#include "specenh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- complex STFT / inverse
 * The return path from a denoised spectrogram to a denoised signal (SURVEY.md §8 row A1,
 * "a complex stft mode"; no call site in the reference, scipy is the specification). Both
 * launches take a specenh_stft_plan and use its window, nperseg, noverlap, fs, scaling and
 * detrend (eps unused; detrend ignored by the inverse). No workspace, no allocation at
 * launch (graph-capturable), any batch. nperseg: a power of two in [64, 4096]. */
#define SPECENH_BOUNDARY_NONE 0  /* boundary=None */
#define SPECENH_BOUNDARY_ZEROS 1 /* boundary='zeros': nperseg/2 zeros at both ends */

/* Frames of scipy.signal.stft(x, nperseg, noverlap, boundary, padded):
 *   ext = length + (boundary ? nperseg : 0), hop = nperseg - noverlap,
 *   nadd = padded ? (-(ext - nperseg) % hop) % nperseg : 0,  T = (ext + nadd - nperseg)/hop + 1,
 * or a negative error (length < nperseg is SPECENH_EINVAL: scipy would shrink nperseg). */
long long specenh_stft_complex_frames(long long length, int nperseg, int noverlap, int boundary,
                                      int padded);
/* Replaces, per signal,
 *   f, t, Zxx = scipy.signal.stft(x, fs, window, nperseg, noverlap, detrend=..., boundary=...,
 *                                 padded=..., scaling='spectrum' | 'psd')
 * x: device fp32, signal b at x + b*x_stride, `length` samples. The boundary zeros and the
 * padding are not materialised: samples outside [0, length) read as 0 (before the per-frame
 * detrend, as in scipy). out: device float2 (re, im) [batch][F][T], F = nperseg/2 + 1,
 * T = specenh_stft_complex_frames(...); Zxx = rfft(detrend(frame) * w) * sqrt(scale) with the
 * plan's scale (SPECTRUM: 1/sum(w)^2, DENSITY: 1/(fs sum(w^2))), no one-sided doubling. */
int specenh_stft_complex(const specenh_stft_plan* plan, const float* x, long long batch,
                         long long length, long long x_stride, void* out /* float2 [batch][F][T] */,
                         int boundary, int padded, void* stream);
/* Output samples of scipy.signal.istft for `frames` frames:
 *   hop*(frames - 1) + nperseg - (boundary ? nperseg : 0), or a negative error. */
long long specenh_istft_length(long long frames, int nperseg, int noverlap, int boundary);
/* Replaces, per spectrogram,
 *   t, x = scipy.signal.istft(Zxx * gain, fs, window, nperseg, noverlap, boundary=...,
 *                             scaling='spectrum' | 'psd')
 * y_t = irfft(Z[:, t]) * (sum(w) | sqrt(fs sum(w^2))) * w, overlap-added at t*hop, divided by
 * norm = sum of w^2 over the frames present (where norm > 1e-10), nperseg/2 samples trimmed
 * from both ends when `boundary` is nonzero. Deterministic (no atomics): the result does not
 * depend on the batch or on how the output is split over workgroups. A failed NOLA condition
 * is not an error (scipy only warns).
 * Z: device float2 [batch][F][frames]. gain: optional device fp32 real mask multiplied into Z
 * on load (no masked copy is written): [batch][gain_rows][frames] with gain_rows = F, or
 * F - 1 (the DROP_NYQUIST shape of the denoisers; the Nyquist bin then gets gain 0); null
 * with gain_rows = 0. out: device fp32, signal b at out + b*out_stride,
 * specenh_istft_length(...) samples. */
int specenh_istft(const specenh_stft_plan* plan, const void* Z /* float2 [batch][F][frames] */,
                  const float* gain, int gain_rows /* 0, F or F-1 */, long long batch,
                  long long frames, float* out, long long out_stride, int boundary, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_STFT_COMPLEX_H */
