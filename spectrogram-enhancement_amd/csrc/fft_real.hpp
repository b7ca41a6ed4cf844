// fft_real.hpp — the passes that turn real frames in LDS into their one-sided spectra, one
// real frame per N/2-point complex transform: shared by spectral_mean.hip,
// spectral_matrix.hip and bispectrum.hip, which differ only in how many frames a workgroup
// transforms side by side and in what they do with the bins.
#pragma once

#include <hip/hip_runtime.h>

namespace specenh {
namespace fft_real {

__device__ __forceinline__ float2 c_mul(float2 a, float2 w) {
  return make_float2(fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x));
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// S forward FFTs of length M = N/2 (transform s at [s * M, (s + 1) * M)), natural order in
// and out, by a workgroup of CT threads; tw is the N-point table, W_M^e = tw[2 e]. Returns
// the buffer that holds the result; ends on a barrier.
template <int CT>
__device__ __forceinline__ float2* fft_half(float2* src, float2* dst, int M, int log2m, int S,
                                            const float2* __restrict__ tw, int tid) {
  const int total = S * M;
  int Ns = 1;
  if (log2m & 1) {
    for (int idx = tid; idx < total / 2; idx += CT) {
      const int base = (idx >> (log2m - 1)) << log2m, j = idx & (M / 2 - 1);
      const float2 v0 = src[base + j], v1 = src[base + j + M / 2];
      dst[base + 2 * j] = make_float2(v0.x + v1.x, v0.y + v1.y);
      dst[base + 2 * j + 1] = make_float2(v0.x - v1.x, v0.y - v1.y);
    }
    float2* tmp = src; src = dst; dst = tmp;
    Ns = 2;
    __syncthreads();
  }
  const int q = M / 4;
  for (; Ns < M; Ns *= 4) {
    const int tstep = M / (2 * Ns);  // 2 * M / (4 Ns): the stride-2 index into the N-point table
    for (int idx = tid; idx < total / 4; idx += CT) {
      const int base = (idx >> (log2m - 2)) << log2m, j = idx & (q - 1);
      const int jm = j & (Ns - 1);
      const float2* s = src + base;
      float2 v0 = s[j], v1 = s[j + q], v2 = s[j + 2 * q], v3 = s[j + 3 * q];
      if (jm) {
        const int e = jm * tstep;
        v1 = c_mul(v1, tw[e]);
        v2 = c_mul(v2, tw[2 * e]);
        v3 = c_mul(v3, tw[3 * e]);  // 3 e < 3 N / 4
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

// 2 X_k of the real frame whose packed transform is z[0 .. M), k in [0, M); w = W_N^k.
__device__ __forceinline__ float2 unpack2(const float2* z, int k, int M, float2 w) {
  const float2 a = z[k], m = z[(M - k) & (M - 1)];
  const float2 r = c_mul(make_float2(a.y + m.y, m.x - a.x), w);  // W_N^k * 2 O_k
  return make_float2(a.x + m.x + r.x, a.y - m.y + r.y);
}

}  // namespace fft_real
}  // namespace specenh
