/* specenh_wavelet.h — a bank of complex FIR filters applied to real signals in one fused pass
 * of libspecenh.so: the continuous wavelet transform (Morlet scalogram) and FIR band-pass
 * filtering. An extension of the C-ABI in specenh.h (same error codes and stream argument)
 * beside specenh_correlation.h; it takes no plan object: the tables below are all it needs. */
#ifndef SPECENH_WAVELET_H
#define SPECENH_WAVELET_H

#include <stddef.h>

#include "specenh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- complex FIR filter bank
 * S filters; filter s has the odd length 2 L_s + 1 and complex taps h_s[m], m = -L_s .. L_s;
 * Lmax = max L_s. For a real signal x of `length` samples, extended by zeros on both sides:
 *
 *   W[b][s][n] = sum_{m = -L_s .. L_s} h_s[m] * x_b[n - m],    n = 0 .. length - 1
 *              = np.convolve(x_b, h_s)[L_s : L_s + length]     (linear, 'same' alignment)
 *
 * With the Morlet taps h_s[m] = pi^(-1/4) s^(-1/2) exp(i w0 m / s - m^2 / (2 s^2)) this is the
 * wavelet transform W_n(s) of Torrence & Compo (1998) eq. 2 with dt = 1 (for Morlet
 * conj psi(-eta) = psi(eta)).
 *
 * Outputs are decimated by hop >= 1:
 *   SPECENH_FB_COMPLEX     out[b][s][j] = W[b][s][j hop]               float2, To = (length-1)/hop + 1
 *   SPECENH_FB_POWER       out[b][s][j] = |W[b][s][j hop]|^2           fp32,   the same To
 *   SPECENH_FB_POWER_MEAN  out[b][s][j] = (1/hop) sum_{i < hop} |W[b][s][j hop + i]|^2
 *                                                                      fp32,   To = length / hop
 *                          (whole windows only, length >= hop: the time-smoothed scalogram)
 *
 * Method: overlap-save on one power-of-two transform length nfft in {256, 512, 1024, 2048,
 * 4096}. A block yields V consecutive outputs, V = nfft - 2 Lmax rounded down to a multiple of
 * hop (1 <= hop <= V is required); block q reads samples [q V - Lmax, q V - Lmax + nfft),
 * zeros outside [0, length), and only the transform's outputs [Lmax, Lmax + V) are used, so
 * the circular wrap never reaches an output. A workgroup transforms its block once and applies
 * a chunk of the filters to it on the chip (the products X H_s and the inverse transforms
 * never reach memory). No allocation at launch (graph-capturable on one stream), no atomics:
 * an element is a function of its own shot's samples, the tables, hop and mode only, whatever
 * the batch, the shot's position in it, the stride and the split of the filters over
 * workgroups. Every element of the output is written. */

#define SPECENH_FB_COMPLEX 0
#define SPECENH_FB_POWER 1
#define SPECENH_FB_POWER_MEAN 2
#define SPECENH_FB_MAX_HALF 1024 /* Lmax <= 1024 */

/* The transform length of a bank whose longest filter has the half length lmax: nfft itself
 * when it is an allowed size that holds the filter (2 lmax + 1 <= nfft); for nfft == 0 the
 * default, the smallest allowed power of two >= 4 lmax and at least 1024. A negative error
 * otherwise. */
int specenh_filterbank_nfft(int lmax, int nfft);

/* Bytes of the tables of a bank: (nscales + 1) * nfft float2; 0, with the error set, when
 * nscales < 1 or nfft is not an allowed size. */
size_t specenh_filterbank_tables_bytes(int nscales, int nfft);

/* Host only: fills tables_host, [nscales + 1][nfft] float2. Row s is the nfft-point DFT
 * (forward, exp(-2 pi i k n / nfft)) of h_s wrapped circularly (h_s[m] at index m mod nfft),
 * computed in fp64 from the taps as given and rounded once to fp32; row nscales holds the
 * twiddles W_nfft^n = exp(-2 pi i n / nfft). The caller copies the table to the device.
 * half_lengths: L_s, 0 <= L_s <= SPECENH_FB_MAX_HALF, 2 L_s + 1 <= nfft.
 * taps: the filters one after the other, filter s as 2 L_s + 1 (re, im) pairs from m = -L_s. */
int specenh_filterbank_tables(int nscales, const int* half_lengths, const double* taps, int nfft,
                              float* tables_host);

/* tables: device, 8-byte aligned, as specenh_filterbank_tables filled them for nscales, nfft.
 * lmax: Lmax of the bank (a larger value only shortens the blocks), 2 lmax + hop <= nfft.
 * x: device fp32, shot b at x + b * x_stride, `length` samples (x_stride >= length).
 * out: device [batch][nscales][To], float2 (SPECENH_FB_COMPLEX) or fp32. */
int specenh_filterbank(const void* tables, int nscales, int nfft, int lmax, const float* x,
                       long long batch, long long length, long long x_stride, long long hop,
                       int mode, void* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_WAVELET_H */
