// stft_plan.hpp — the STFT plan object: stft_psd.hip creates and destroys it, stft_complex.hip
// runs the complex forward / inverse transforms on it, and the averaging operators read it
// through averaging.hpp.
#pragma once

#include <hip/hip_runtime.h>

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
