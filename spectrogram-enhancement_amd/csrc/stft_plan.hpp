// stft_plan.hpp — the STFT plan object shared by stft_psd.hip (which creates and destroys
// it) and stft_complex.hip (complex forward / inverse transforms on the same plan).
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
};
