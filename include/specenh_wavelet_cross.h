/* specenh_wavelet_cross.h — the cross spectrum of two real signals through one bank of complex
 * FIR filters, in one fused pass of libspecenh.so: the cross-wavelet spectrum and the spectra
 * that wavelet coherence is formed from (Torrence & Webster 1999; Grinsted et al. 2004). An
 * extension of specenh_wavelet.h: the same tables, blocks, error codes and stream argument. */
#ifndef SPECENH_WAVELET_CROSS_H
#define SPECENH_WAVELET_CROSS_H

#include "specenh_wavelet.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- cross spectrum of a pair
 * With W of specenh_wavelet.h (filter s applied to a signal of `length` samples extended by
 * zeros), Wx of x_b and Wy of y_b, and j indexing the outputs:
 *
 *   SPECENH_XWT_POINT, To = (length - 1) / hop + 1:
 *     sxy[b][s][j] = conj(Wx[b][s][j hop]) * Wy[b][s][j hop]                         float2
 *     sxx[b][s][j] = |Wx[b][s][j hop]|^2,   syy[b][s][j] = |Wy[b][s][j hop]|^2       fp32
 *   SPECENH_XWT_MEAN, To = length / hop (whole windows only, length >= hop):
 *     sxy[b][s][j] = (1/hop) sum_{i < hop} conj(Wx[b][s][j hop + i]) * Wy[b][s][j hop + i]
 *     sxx[b][s][j] = (1/hop) sum_{i < hop} |Wx[b][s][j hop + i]|^2, syy likewise with Wy
 *
 * conj(x) y is the convention of specenh_spectral.h and specenh_csm.h: with Morlet taps a y
 * that is x delayed has a negative phase.
 *
 * Method: the overlap-save blocks of specenh_filterbank. A workgroup transforms its block of x
 * and of y once and forms Wx and Wy of a chunk of the filters on the chip; Wx, Wy, their
 * products and the inverse transforms never reach memory. No allocation at launch
 * (graph-capturable on one stream), no atomics: an element is a function of its own pair's
 * samples, the tables, hop and mode only, whatever the batch, the pair's position in it, the
 * strides and the split of the filters over workgroups. The mean of a hop window is a
 * fixed-order sum (runs of 16 ascending, then the runs ascending). Every element of the outputs
 * is written. */

#define SPECENH_XWT_POINT 0
#define SPECENH_XWT_MEAN 1

/* tables, nscales, nfft, lmax: as for specenh_filterbank (specenh_filterbank_tables fills the
 * tables; one set serves both entries), 2 lmax + hop <= nfft.
 * x, y: device fp32, pair b at x + b * x_stride and y + b * y_stride, `length` samples each
 * (strides >= length); x == y is allowed.
 * sxy: device [batch][nscales][To] float2. sxx, syy: device [batch][nscales][To] fp32, both
 * given or both null (null: the cross spectrum only). */
int specenh_filterbank_cross(const void* tables, int nscales, int nfft, int lmax, const float* x,
                             const float* y, long long batch, long long length,
                             long long x_stride, long long y_stride, long long hop, int mode,
                             void* sxy, float* sxx, float* syy, void* stream);

/* Host only, touches no device when cus > 0: the filters a workgroup loops over for this launch
 * on a device of `cus` compute units (0: the current device). 16, halved down to 4 while the
 * launch has fewer than two workgroups a compute unit; the outputs do not depend on it. A
 * negative error for arguments specenh_filterbank_cross refuses. */
int specenh_filterbank_cross_chunk(int nscales, int nfft, int lmax, long long batch,
                                   long long length, long long hop, int mode, int cus);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_WAVELET_CROSS_H */
