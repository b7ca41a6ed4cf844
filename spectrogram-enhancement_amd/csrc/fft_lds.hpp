// fft_lds.hpp — the device code every LDS-transform kernel opens with: the mixed-radix
// Stockham FFT in two LDS ping-pong buffers (stft_complex.hip, cross_spectrum.hip,
// spectral_mean.hip, spectral_matrix.hip, bispectrum.hip) and, for the three kernels that
// carry one real frame per N/2-point transform, the frame front end (load, detrend, window)
// and the unpack of the one-sided bins. The kernels differ in how many transforms a workgroup
// runs side by side, in where a sample comes from and in what they do with the bins.
#pragma once

#include <hip/hip_runtime.h>

#include "specenh.h"
#include "wave.hpp"  // wave_sum

namespace specenh {
namespace fft_lds {

__device__ __forceinline__ float2 c_mul(float2 a, float2 w) {
  return make_float2(fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x));
}

// P forward FFTs of length Lf (transform p at [p * Lf, (p + 1) * Lf)), natural order in and
// out, by a workgroup of CT threads: one radix-2 pass when log2 Lf is odd, then radix-4. tw is
// a natural-order table W_tlen^n of tlen = Lf or 2 Lf entries (a real frame's half-length
// transform reads the frame-length table at stride 2). Returns the buffer that holds the
// result; ends on a barrier.
template <int CT>
__device__ __forceinline__ float2* stockham(float2* src, float2* dst, int Lf, int log2l, int P,
                                            const float2* __restrict__ tw, int tlen, int tid) {
  const int total = P * Lf;
  int Ns = 1;
  if (log2l & 1) {
    for (int idx = tid; idx < total / 2; idx += CT) {
      const int base = (idx >> (log2l - 1)) << log2l, j = idx & (Lf / 2 - 1);
      const float2 v0 = src[base + j], v1 = src[base + j + Lf / 2];
      dst[base + 2 * j] = make_float2(v0.x + v1.x, v0.y + v1.y);
      dst[base + 2 * j + 1] = make_float2(v0.x - v1.x, v0.y - v1.y);
    }
    float2* tmp = src; src = dst; dst = tmp;
    Ns = 2;
    __syncthreads();
  }
  const int q = Lf / 4;
  for (; Ns < Lf; Ns *= 4) {
    // unsigned: both are positive, and a signed scalar division (the sign of 4 Ns is not known
    // to the compiler) sits on every pass's critical path when a workgroup runs alone
    const int tstep = (unsigned)tlen / (4u * Ns);
    for (int idx = tid; idx < total / 4; idx += CT) {
      const int base = (idx >> (log2l - 2)) << log2l, j = idx & (q - 1);
      const int jm = j & (Ns - 1);
      const float2* s = src + base;
      float2 v0 = s[j], v1 = s[j + q], v2 = s[j + 2 * q], v3 = s[j + 3 * q];
      if (jm) {
        const int e = jm * tstep;
        v1 = c_mul(v1, tw[e]);
        v2 = c_mul(v2, tw[2 * e]);
        v3 = c_mul(v3, tw[3 * e]);  // 3 e < 3 tlen / 4
      }
      const float2 s02 = make_float2(v0.x + v2.x, v0.y + v2.y);
      const float2 d02 = make_float2(v0.x - v2.x, v0.y - v2.y);
      const float2 s13 = make_float2(v1.x + v3.x, v1.y + v3.y);
      const float2 d13 = make_float2(v1.x - v3.x, v1.y - v3.y);  // -i * d13 = (d13.y, -d13.x)
      float2* d = dst + base + (j - jm) * 4 + jm;
      d[0] = make_float2(s02.x + s13.x, s02.y + s13.y);
      d[Ns] = make_float2(d02.x + d13.y, d02.y - d13.x);
      d[2 * Ns] = make_float2(s02.x - s13.x, s02.y - s13.y);
      d[3 * Ns] = make_float2(d02.x - d13.y, d02.y + d13.x);
    }
    float2* tmp = src; src = dst; dst = tmp;
    __syncthreads();
  }
  return src;
}

// The front end of a one-real-frame-per-transform kernel: S frames of N samples into raw
// (slot s at [s * N, (s + 1) * N)), sample(s, n) giving sample n of slot s or zero for a slot
// with no frame; then the detrend (fp64 sums, one wave per slot; stat is the caller's
// __shared__ [>= S][2]: mean, slope) and the window. Ends on a barrier.
template <int CT, class Sample>
__device__ __forceinline__ void load_frames(float* raw, float (*stat)[2], int N, int log2n, int S,
                                            int detrend, const float* win, int tid,
                                            Sample sample) {
  const float kc = 0.5f * (N - 1);
  for (int idx = tid; idx < S * N; idx += CT) {
    const int s = idx >> log2n, n = idx & (N - 1);
    float v = sample(s, n);
    if (detrend == SPECENH_DETREND_NONE) v *= win[n];
    raw[idx] = v;
  }
  __syncthreads();
  if (detrend != SPECENH_DETREND_NONE) {  // uniform
    for (int s = tid >> 6; s < S; s += CT / 64) {
      double sx = 0.0, skx = 0.0;
      for (int n = tid & 63; n < N; n += 64) {
        const double v = raw[s * N + n];
        sx += v;
        skx += ((double)n - 0.5 * (N - 1)) * v;
      }
      sx = wave_sum(sx);
      skx = wave_sum(skx);
      if ((tid & 63) == 0) {
        const double skk = (double)N * ((double)N * N - 1.0) / 12.0;
        stat[s][0] = (float)(sx / N);
        stat[s][1] = detrend == SPECENH_DETREND_LINEAR ? (float)(skx / skk) : 0.f;
      }
    }
    __syncthreads();
    for (int idx = tid; idx < S * N; idx += CT) {
      const int s = idx >> log2n, n = idx & (N - 1);
      raw[idx] = (raw[idx] - stat[s][0] - stat[s][1] * ((float)n - kc)) * win[n];
    }
    __syncthreads();
  }
}

// 2 X_k of the real frame whose packed transform is z[0 .. M), k in [0, M); w = W_N^k.
__device__ __forceinline__ float2 unpack2(const float2* z, int k, int M, float2 w) {
  const float2 a = z[k], m = z[(M - k) & (M - 1)];
  const float2 r = c_mul(make_float2(a.y + m.y, m.x - a.x), w);  // W_N^k * 2 O_k
  return make_float2(a.x + m.x + r.x, a.y - m.y + r.y);
}

// 2 X_{N/2} of the same frame: 2 (Re Z_0 - Im Z_0), real.
__device__ __forceinline__ float nyquist2(const float2* z) { return 2.f * (z[0].x - z[0].y); }

}  // namespace fft_lds
}  // namespace specenh
