// block_fft.hpp — the forward transform of a workgroup that runs many transforms of one length
// nfft = 256 NI on one block of samples: the overlap-save filter-bank kernels (filterbank.hip,
// filterbank_cross.hip). 256 threads; natural order in and out; two LDS buffers of nfft float2.
#pragma once
#include <hip/hip_runtime.h>

#include "fft_lds.hpp"

namespace specenh {
namespace block_fft {

constexpr int CT = 256;  // threads per workgroup

using fft_lds::c_mul;
using fft_lds::stockham;

// The transform of the filter loop for nfft = 256 NI >= 1024: fft_lds::stockham's passes (one
// radix-2 pass when log2 nfft is odd, then radix-4, natural order in and out) for one transform
// a workgroup, with what a workgroup that runs SC + 1 transforms of one length can afford: every
// thread runs the same NI / 4 butterflies in every pass, so their twiddles are loaded from the
// table once into registers (a twiddle load from global memory inside a pass sits on the
// critical path of a workgroup that has two waves a SIMD), and a pass issues all its LDS reads
// before its first store.
template <int NI>
struct BlockFft {
  static constexpr int N = CT * NI, Q = N / 4, NB = NI / 4;
  static constexpr int LOG = NI == 4 ? 10 : NI == 8 ? 11 : 12;
  static constexpr int NS0 = (LOG & 1) ? 2 : 1;  // Ns of the first radix-4 pass
  static constexpr int NP = LOG / 2;             // radix-4 passes
  float2 w[NP][NB][3];

  __device__ __forceinline__ void init(const float2* __restrict__ tw, int tid) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int Ns = NS0 << (2 * p);
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int e = ((tid + CT * i) & (Ns - 1)) * (N / (4 * Ns));  // 3 e < 3 N / 4
        w[p][i][0] = tw[e];
        w[p][i][1] = tw[2 * e];
        w[p][i][2] = tw[3 * e];
      }
    }
  }

  // src -> the returned buffer; src is read after the caller's barrier; ends on a barrier
  __device__ __forceinline__ float2* run(float2* src, float2* dst, int tid) const {
    if constexpr (LOG & 1) {
      float2 v[NI / 2][2];
#pragma unroll
      for (int i = 0; i < NI / 2; ++i) {
        v[i][0] = src[tid + CT * i];
        v[i][1] = src[tid + CT * i + N / 2];
      }
#pragma unroll
      for (int i = 0; i < NI / 2; ++i) {
        const int j = tid + CT * i;
        dst[2 * j] = make_float2(v[i][0].x + v[i][1].x, v[i][0].y + v[i][1].y);
        dst[2 * j + 1] = make_float2(v[i][0].x - v[i][1].x, v[i][0].y - v[i][1].y);
      }
      float2* tmp = src; src = dst; dst = tmp;
      __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int Ns = NS0 << (2 * p);
      float2 v[NB][4];
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) v[i][r] = src[tid + CT * i + r * Q];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int j = tid + CT * i, jm = j & (Ns - 1);
        const float2 v0 = v[i][0];
        float2 v1 = v[i][1], v2 = v[i][2], v3 = v[i][3];
        if (Ns > 1) {  // compile time; W^0 = (1, 0) multiplies exactly
          v1 = c_mul(v1, w[p][i][0]);
          v2 = c_mul(v2, w[p][i][1]);
          v3 = c_mul(v3, w[p][i][2]);
        }
        const float2 s02 = make_float2(v0.x + v2.x, v0.y + v2.y);
        const float2 d02 = make_float2(v0.x - v2.x, v0.y - v2.y);
        const float2 s13 = make_float2(v1.x + v3.x, v1.y + v3.y);
        const float2 d13 = make_float2(v1.x - v3.x, v1.y - v3.y);  // -i * d13 = (d13.y, -d13.x)
        float2* d = dst + (j - jm) * 4 + jm;
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
};
template <>
struct BlockFft<1> {};
template <>
struct BlockFft<2> {};

// one forward transform of the workgroup's nfft = 2^log2n points: src -> the returned buffer
// (src or dst); tw: exp(-2 pi i k / nfft)
template <int NI>
__device__ __forceinline__ float2* transform(const BlockFft<NI>& f, float2* src, float2* dst,
                                             int nfft, int log2n, const float2* tw, int tid) {
  if constexpr (NI >= 4) return f.run(src, dst, tid);
  else return stockham<CT>(src, dst, nfft, log2n, 1, tw, nfft, tid);
}

}  // namespace block_fft
}  // namespace specenh
