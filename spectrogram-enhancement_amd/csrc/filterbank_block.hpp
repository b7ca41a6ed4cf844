// filterbank_block.hpp — what the overlap-save filter-bank kernels (filterbank.hip,
// filterbank_cross.hip) share around the transform of block_fft.hpp. Host: the shape checks, the
// plan of a call (block length, outputs, filters per workgroup) and the slicing of a batch.
// Device: the zero-extended block load, the table-row load, the product store and the hop
// epilogue, whose fixed summation order both kernels' results depend on.
#pragma once
#include <hip/hip_runtime.h>

#include "specenh_wavelet.h"  // SPECENH_FB_MAX_HALF
#include "runtime.hpp"
#include "averaging.hpp"  // launch, launched
#include "block_fft.hpp"

namespace specenh {
namespace filterbank_block {

using block_fft::CT;  // threads per workgroup
using block_fft::c_mul;

constexpr int RUN = 16;     // values a thread sums in a row for the hop mean
constexpr int MAX_SC = 16;  // filters per workgroup at most: the block's own transform is 1/17 of the work
constexpr int MIN_SC = 4;

// ---------------------------------------------------------------- host
// The plan of a call; each kernel's Args holds one beside its pointers, strides, mode and scale.
struct Plan {
  long long length;
  long long To;  // outputs per (shot, filter)
  int S, nfft, log2n, lmax, hop;
  int V, Vh;     // outputs of W per block, stored outputs per block (V / hop)
  int SC, nchunk;
  int P;         // runs per hop window (mean mode): ceil(hop / RUN)
};

inline bool allowed_nfft(int nfft) {
  return nfft == 256 || nfft == 512 || nfft == 1024 || nfft == 2048 || nfft == 4096;
}

constexpr const char* NFFT_MSG = "nfft must be 256, 512, 1024, 2048 or 4096";

// The checks of an entry that do not look at a pointer. mode_ok, mode_msg: whether the entry
// knows the mode, and its message if not; mean: the mode is a mean over hop windows.
inline int check_shape(int nscales, int nfft, int lmax, long long batch, long long length,
                       long long hop, bool mode_ok, const char* mode_msg, bool mean) {
  if (nscales < 1) return set_error(SPECENH_EINVAL, "nscales must be >= 1");
  if (!allowed_nfft(nfft)) return set_error(SPECENH_EINVAL, NFFT_MSG);
  if (lmax < 0 || lmax > SPECENH_FB_MAX_HALF)
    return set_error(SPECENH_EINVAL, "lmax must be in [0, 1024]");
  if (batch < 0) return set_error(SPECENH_EINVAL, "batch must be >= 0");
  if (hop < 1) return set_error(SPECENH_EINVAL, "hop must be >= 1");
  if (2LL * lmax + hop > nfft)
    return set_error(SPECENH_EINVAL, "2 lmax + hop must not exceed nfft");
  if (!mode_ok) return set_error(SPECENH_EINVAL, mode_msg);
  if (length < 1) return set_error(SPECENH_EINVAL, "length must be >= 1");
  if (mean && length < hop) return set_error(SPECENH_EINVAL, "signal shorter than hop");
  return SPECENH_OK;
}

// Fills p for a checked shape on a device of `cus` compute units; returns the blocks of a shot.
inline long long plan(Plan& p, int nscales, int nfft, int lmax, long long batch, long long length,
                      long long hop, bool mean, int cus) {
  p.S = nscales; p.nfft = nfft; p.log2n = ilog2i(nfft); p.lmax = lmax; p.hop = (int)hop;
  p.length = length;
  p.Vh = (nfft - 2 * lmax) / (int)hop;  // >= 1
  p.V = p.Vh * (int)hop;
  p.To = mean ? length / hop : (length - 1) / hop + 1;
  p.P = (p.hop + RUN - 1) / RUN;
  const long long nblk = (p.To + p.Vh - 1) / p.Vh;
  // filters per workgroup: as many as leave two workgroups a CU (a single shot fills the chip)
  const long long want = 2LL * cus;
  const long long nb0 = batch < 65535 ? batch : 65535;
  p.SC = MAX_SC;
  while (p.SC > MIN_SC && nblk * ((nscales + p.SC - 1) / p.SC) * nb0 < want) p.SC /= 2;
  p.nchunk = (nscales + p.SC - 1) / p.SC;
  return nblk;
}

// One launch per 65,535 shots (the grid.y limit) of a planned call; at(b0) points a's signals
// and outputs at shot b0. SPECENH_OK or the first launch's error.
template <class Kernel, class Args, class At>
int launch_slices(Kernel kern, Args& a, long long nblk, long long batch, size_t lds, void* stream,
                  const char* name, At at) {
  for (long long b0 = 0; b0 < batch; b0 += 65535) {
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    at(b0);
    launch(kern, dim3((unsigned)(nblk * a.p.nchunk), (unsigned)nb), dim3(CT), lds, stream, a);
    if (int rc = launched(name)) return rc;
  }
  return SPECENH_OK;
}

// ---------------------------------------------------------------- device
__device__ __forceinline__ float power(float2 f) { return fmaf(f.x, f.x, f.y * f.y); }

// one block of a signal into buf as nfft complex numbers with zero imaginary part
template <int NI>
__device__ __forceinline__ void load_block(float2* buf, const float* xb, long long n0,
                                           long long length, int tid) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int k = tid + CT * i;
    const long long t = n0 + k;
    buf[k] = make_float2(t >= 0 && t < length ? xb[t] : 0.f, 0.f);
  }
}

// row s of the table [..][n]: thread t takes H_s[t + 256 i]
template <int NI>
__device__ __forceinline__ void load_row(float2 (&H)[NI], const float2* tab, int s, int n,
                                         int tid) {
#pragma unroll
  for (int i = 0; i < NI; ++i) H[i] = tab[(long long)s * n + tid + CT * i];
}

// conj(X_k H[k]) into dst: its forward transform is conj(W) nfft
template <int NI>
__device__ __forceinline__ void store_product(float2* dst, const float2 (&X)[NI],
                                              const float2 (&H)[NI], int tid) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const float2 p = c_mul(X[i], H[i]);
    dst[tid + CT * i] = make_float2(p.x, -p.y);
  }
}

__device__ __forceinline__ void add(float& a, float b) { a += b; }
__device__ __forceinline__ void add(float4& a, const float4& b) {
  a.x += b.x;
  a.y += b.y;
  a.z += b.z;
  a.w += b.w;
}

// The hop epilogue: the block's cnt stored outputs of one filter. h.term(i) is what position i
// of the block's V outputs contributes (an h.Acc: float or float4), h.store(jj, v) scales and
// stores output jj. sampled: the term at jj hop itself, never 0 + term (-0 stays -0). Otherwise
// the sum of the window's hop terms in a fixed order: runs of RUN ascending, one thread a run,
// then the runs ascending (P = 1: one run); the order depends on hop alone. The runs' sums go
// to `spare`, the transform buffer that the result in `res` leaves free (cnt P <= V / 8 of
// them). Returns the buffer the next product may go to: spare, or after the two-level sum res,
// which every thread is done with past the barrier while spare is still being read.
template <class Hop>
__device__ __forceinline__ float2* hop_epilogue(const Hop& h, bool sampled, int P, int hop,
                                                int cnt, float2* res, float2* spare, int tid) {
  using Acc = typename Hop::Acc;
  float2* next = spare;
  if (sampled) {
    for (int jj = tid; jj < cnt; jj += CT) h.store(jj, h.term(jj * hop));
  } else if (P == 1) {
    for (int jj = tid; jj < cnt; jj += CT) {
      Acc acc{};
      for (int i = 0; i < hop; ++i) add(acc, h.term(jj * hop + i));
      h.store(jj, acc);
    }
  } else {
    Acc* part = reinterpret_cast<Acc*>(spare);
    for (int idx = tid; idx < cnt * P; idx += CT) {
      const int jj = idx / P, p = idx - jj * P;
      const int i1 = (p + 1) * RUN < hop ? (p + 1) * RUN : hop;
      Acc acc{};
      for (int i = p * RUN; i < i1; ++i) add(acc, h.term(jj * hop + i));
      part[idx] = acc;
    }
    __syncthreads();
    for (int jj = tid; jj < cnt; jj += CT) {
      Acc acc{};
      for (int p = 0; p < P; ++p) add(acc, part[jj * P + p]);
      h.store(jj, acc);
    }
    next = res;
  }
  return next;
}

}  // namespace filterbank_block
}  // namespace specenh
