// stft_plan.hpp — the STFT plan object shared by stft_psd.hip (which creates and destroys
// it) and stft_complex.hip (complex forward / inverse transforms on the same plan), and the
// host-side arithmetic on it that the averaging ops share (spectral_mean.hip,
// spectral_matrix.hip, bispectrum.hip, wavenumber.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "specenh_spectral.h"
#include "runtime.hpp"

struct specenh_stft_plan {
  int nperseg, noverlap, hop;
  double fs, eps, scale;
  int scaling, detrend;
  int device;
  float* d_window;
  float2* d_twiddle;
  double dc_alpha, dc_beta;  // DC coefficients from the fp32 window (StftArgs)
  double* d_dc;              // c_n = w_n - alpha - beta (n - kmid), fp64
  // complex STFT / inverse STFT (stft_complex.hip)
  double win_sum, win_sumsq;  // sum(w), sum(w^2) of the fp64 window
  float2* d_tw_nat;           // W_N^n = exp(-2 pi i n / N), n = 0 .. N-1, natural order
  // zero-padded frames (correlation.hip): a real 2N-point frame through an N-point transform
  float2* d_tw_pad;           // W_2N^n = exp(-pi i n / N), n = 0 .. N-1
};

namespace specenh {

// Real frames transformed side by side by a CSM or bispectrum workgroup: 8 where two buffers
// of S * N/2 complex fit 64 KiB.
inline int slots8_for(int N) { return N <= 1024 ? 8 : 8192 / N; }

// Frames, groups, frames per group, frames that enter a group and chunks (runs of at most
// SPECENH_SPECTRAL_CHUNK frames) per group of an averaging call.
struct FrameSplit {
  long long T, G, glen, Tu, ncg;
};
// Fills *s or returns a negative error; lds_sizes: nperseg must be one the LDS transform has.
inline int frame_split(const specenh_stft_plan* plan, long long length, long long navg,
                       bool lds_sizes, FrameSplit* s) {
  const int N = plan->nperseg;
  if (lds_sizes && (N < 64 || N > 4096 || (N & (N - 1))))
    return set_error(SPECENH_EUNSUPPORTED, "nperseg must be a power of two in [64, 4096]");
  s->T = specenh_stft_frames(length, N, plan->noverlap);
  if (s->T < 0) return (int)s->T;
  s->G = specenh_spectral_groups(s->T, navg);
  if (s->G < 0) return (int)s->G;
  if (s->T > (1ll << 30)) return set_error(SPECENH_EINVAL, "too many frames");
  s->glen = navg >= 1 ? navg : s->T;
  s->Tu = s->G * s->glen;
  s->ncg = (s->glen + SPECENH_SPECTRAL_CHUNK - 1) / SPECENH_SPECTRAL_CHUNK;
  return SPECENH_OK;
}

// The distinct signals of a bispectrum or wavenumber-spectrum call: shot b of signal s at
// p[s] + b * stride[s].
struct FrameSignals {
  const float* p[3];
  long long stride[3];
};
// Detrends, windows and transforms frames [0, Tu) of every signal of every shot, once, into
// `workspace` as float2 [batch][nsig][Tu][F] holding 2 X / sqrt(plan->scale) (defined in
// bispectrum.hip beside its kernel). SPECENH_OK or a negative error.
int transform_frames(const specenh_stft_plan* plan, const FrameSignals& sig, int nsig,
                     long long batch, long long Tu, void* workspace, hipStream_t stream);

}  // namespace specenh
