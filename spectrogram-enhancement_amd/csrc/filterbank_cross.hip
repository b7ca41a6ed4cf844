// filterbank_cross.hip — the cross spectrum of two real signals through one bank of S complex
// FIR filters for gfx950 (include/specenh_wavelet_cross.h): with W of specenh_wavelet.h,
//   sxy = conj(Wx) Wy,  sxx = |Wx|^2,  syy = |Wy|^2
// at every hop-th sample, or their means over each whole window of hop samples: the
// cross-wavelet spectrum and the spectra wavelet coherence is formed from.
//
// The decomposition, the tables, the block length V and the zero extension are those of
// filterbank.hip. filterbank_cross_kernel: a workgroup owns one (block, chunk of SC filters,
// pair). It transforms the block of x and the block of y (block_fft.hpp) and keeps both spectra
// in registers, thread t holding X[t + 256 i] and Y[t + 256 i]. Per filter it writes
// conj(X_k H_s[k]) into the free buffer and transforms it, copies the V outputs the block
// yields, [Lmax, Lmax + V) of the result (conj(Wx) nfft, the inverse through the forward
// transform), to a strip of their own, so that they survive Wy's ping-pong transform, and does
// the same with Y in the two transform buffers. The epilogue reads the strip and Wy's result and
// stores the block's V / hop outputs of each of the three arrays as one contiguous run.
//   The mean of a hop window is a fixed-order sum, as in filterbank_kernel: runs of 16
//   consecutive values summed in ascending order, then the runs in ascending order; the four
//   partial sums of a run (re, im, xx, yy) go to the buffer Wy's transform leaves free.
//
// Wx, Wy, their products and the inverse transforms never reach memory; no atomics; an element
// depends on its own pair's samples, the tables, hop and mode only.
//
// LDS: two buffers of nfft float2 and the strip of V <= nfft - 2 Lmax (4 KiB + .. 96 KiB, opted
// in through allow_lds; 80 KiB at nfft 4096 with Lmax 1024: two workgroups a CU); no static LDS,
// so the dynamic base is aligned.
#include <hip/hip_runtime.h>

#include <string>

#include "specenh_wavelet_cross.h"
#include "runtime.hpp"
#include "averaging.hpp"  // check_stride, launch, launched
#include "block_fft.hpp"

namespace specenh {
namespace {

using block_fft::BlockFft;
using block_fft::CT;
using block_fft::c_mul;
using block_fft::transform;

constexpr int RUN = 16;     // values a thread sums in a row for the hop mean
constexpr int MAX_SC = 16;  // filters per workgroup at most: the two forward transforms are 1/17 of its work
constexpr int MIN_SC = 4;
constexpr int MAX_LDS = 96 * 1024;

struct Args {
  const float2* tab;  // [S + 1][nfft]: H_s, then W_nfft^n
  const float* x;
  const float* y;
  long long xs, ys, length;
  long long To;  // outputs per (pair, filter)
  int S, nfft, log2n, lmax, hop;
  int V, Vh;     // outputs of W per block, stored outputs per block (V / hop)
  int SC, nchunk;
  int mode;
  int P;         // runs per hop window (mean mode): ceil(hop / RUN)
  float scale;   // 1 / nfft^2 (point), 1 / (nfft^2 hop) (mean)
  float2* sxy;   // [batch][S][To]
  float* sxx;    // [batch][S][To], or null together with syy
  float* syy;
};

// conj(fx) * fy of the two transforms' results is Wx * conj(Wy) nfft^2; conj(Wx) Wy is its
// conjugate, fx * conj(fy)
__device__ __forceinline__ float2 cross(float2 fx, float2 fy) {
  return make_float2(fmaf(fx.x, fy.x, fx.y * fy.y), fmaf(fx.y, fy.x, -(fx.x * fy.y)));
}
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

template <int NI>
__global__ __launch_bounds__(CT) void filterbank_cross_kernel(Args a) {
  extern __shared__ __align__(16) float2 sm[];  // the partial sums are stored as float4
  const int n = a.nfft, tid = threadIdx.x, S = a.S, hop = a.hop, lmax = a.lmax;
  float2* const strip = sm + 2 * n;  // V float2: Wx's outputs while Wy is transformed
  auto other = [&](const float2* p) { return p == sm ? sm + n : sm; };  // of the two transform buffers
  const int q = blockIdx.x / a.nchunk, c = blockIdx.x - q * a.nchunk;
  const long long b = blockIdx.y;
  const long long n0 = (long long)q * a.V - lmax;  // first sample of the block
  const float2* tw = a.tab + (long long)S * n;
  BlockFft<NI> fft;
  if constexpr (NI >= 4) fft.init(tw, tid);
  float2 X[NI], Y[NI];
  load_block<NI>(sm, a.x + b * a.xs, n0, a.length, tid);
  __syncthreads();
  float2* res = transform(fft, sm, sm + n, n, a.log2n, tw, tid);
#pragma unroll
  for (int i = 0; i < NI; ++i) X[i] = res[tid + CT * i];
  load_block<NI>(other(res), a.y + b * a.ys, n0, a.length, tid);  // X is still being read from res
  __syncthreads();
  res = transform(fft, other(res), res, n, a.log2n, tw, tid);
#pragma unroll
  for (int i = 0; i < NI; ++i) Y[i] = res[tid + CT * i];
  // the buffer the next product of X goes to: one that no thread still reads
  float2* cur = other(res);
  const long long j0 = (long long)q * a.Vh;  // first stored output of the block
  const int cnt = a.To - j0 < a.Vh ? (int)(a.To - j0) : a.Vh;  // >= 1: the grid has ceil(To / Vh) blocks
  const int s1 = (c + 1) * a.SC < S ? (c + 1) * a.SC : S;
  const float sc = a.scale;
  const bool autos = a.sxx != nullptr;  // uniform
  float2 H[NI];  // this filter's row; the next one's is loaded under Wy's transform
#pragma unroll
  for (int i = 0; i < NI; ++i) H[i] = a.tab[(long long)(c * a.SC) * n + tid + CT * i];
  for (int s = c * a.SC; s < s1; ++s) {  // uniform
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float2 p = c_mul(X[i], H[i]);
      cur[tid + CT * i] = make_float2(p.x, -p.y);
    }
    __syncthreads();  // every thread is done with the previous filter's buffers
    float2* rx = transform(fft, cur, other(cur), n, a.log2n, tw, tid);
    // Wx's outputs to the strip (the previous filter's were last read before the barrier
    // above), the product of Y beside them; rx's transform ended on a barrier
    for (int k = tid; k < a.V; k += CT) strip[k] = rx[lmax + k];
    float2* py = other(rx);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float2 p = c_mul(Y[i], H[i]);
      py[tid + CT * i] = make_float2(p.x, -p.y);
    }
    if (s + 1 < s1) {
#pragma unroll
      for (int i = 0; i < NI; ++i) H[i] = a.tab[(long long)(s + 1) * n + tid + CT * i];
    }
    __syncthreads();  // the strip is whole, rx is free
    float2* ry = transform(fft, py, rx, n, a.log2n, tw, tid);
    float2* spare = other(ry);
    const float2* fx = strip;      // conj(Wx) * nfft at outputs q V ..
    const float2* fy = ry + lmax;  // conj(Wy) * nfft
    const long long o = (b * S + s) * a.To + j0;
    cur = spare;
    if (a.mode == SPECENH_XWT_POINT) {
      for (int jj = tid; jj < cnt; jj += CT) {
        const float2 u = fx[jj * hop], v = fy[jj * hop];
        const float2 p = cross(u, v);
        a.sxy[o + jj] = make_float2(p.x * sc, p.y * sc);
        if (autos) {
          a.sxx[o + jj] = power(u) * sc;
          a.syy[o + jj] = power(v) * sc;
        }
      }
    } else if (a.P == 1) {  // mean over a window of at most RUN values: one thread, ascending
      for (int jj = tid; jj < cnt; jj += CT) {
        float re = 0.f, im = 0.f, xx = 0.f, yy = 0.f;
        for (int i = 0; i < hop; ++i) {
          const float2 u = fx[jj * hop + i], v = fy[jj * hop + i];
          const float2 p = cross(u, v);
          re += p.x;
          im += p.y;
          xx += power(u);
          yy += power(v);
        }
        a.sxy[o + jj] = make_float2(re * sc, im * sc);
        if (autos) {
          a.sxx[o + jj] = xx * sc;
          a.syy[o + jj] = yy * sc;
        }
      }
    } else {  // runs of RUN values into the free buffer, then the runs of a window, ascending
      float4* part = reinterpret_cast<float4*>(spare);  // cnt * P <= V / 8 float4 <= nfft / 2
      const int P = a.P;
      for (int idx = tid; idx < cnt * P; idx += CT) {
        const int jj = idx / P, p = idx - jj * P;
        const int i1 = (p + 1) * RUN < hop ? (p + 1) * RUN : hop;
        float re = 0.f, im = 0.f, xx = 0.f, yy = 0.f;
        for (int i = p * RUN; i < i1; ++i) {
          const float2 u = fx[jj * hop + i], v = fy[jj * hop + i];
          const float2 pr = cross(u, v);
          re += pr.x;
          im += pr.y;
          xx += power(u);
          yy += power(v);
        }
        part[idx] = make_float4(re, im, xx, yy);
      }
      __syncthreads();
      for (int jj = tid; jj < cnt; jj += CT) {
        float re = 0.f, im = 0.f, xx = 0.f, yy = 0.f;
        for (int p = 0; p < P; ++p) {
          const float4 v = part[jj * P + p];
          re += v.x;
          im += v.y;
          xx += v.z;
          yy += v.w;
        }
        a.sxy[o + jj] = make_float2(re * sc, im * sc);
        if (autos) {
          a.sxx[o + jj] = xx * sc;
          a.syy[o + jj] = yy * sc;
        }
      }
      cur = ry;  // the partials are still being read; every thread is past the barrier, done with ry
    }
  }
}

using Kernel = void (*)(Args);
Kernel kernel_for(int nfft) {
  switch (nfft) {
    case 256: return filterbank_cross_kernel<1>;
    case 512: return filterbank_cross_kernel<2>;
    case 1024: return filterbank_cross_kernel<4>;
    case 2048: return filterbank_cross_kernel<8>;
    default: return filterbank_cross_kernel<16>;
  }
}

LdsOptIn g_lds;

bool allowed_nfft(int nfft) {
  return nfft == 256 || nfft == 512 || nfft == 1024 || nfft == 2048 || nfft == 4096;
}

// the checks of specenh_filterbank that do not look at a pointer, with its messages
int check_shape(int nscales, int nfft, int lmax, long long batch, long long length, long long hop,
                int mode) {
  if (nscales < 1) return set_error(SPECENH_EINVAL, "nscales must be >= 1");
  if (!allowed_nfft(nfft))
    return set_error(SPECENH_EINVAL, "nfft must be 256, 512, 1024, 2048 or 4096");
  if (lmax < 0 || lmax > SPECENH_FB_MAX_HALF) return set_error(SPECENH_EINVAL, "lmax must be in [0, 1024]");
  if (batch < 0) return set_error(SPECENH_EINVAL, "batch must be >= 0");
  if (hop < 1) return set_error(SPECENH_EINVAL, "hop must be >= 1");
  if (2LL * lmax + hop > nfft)
    return set_error(SPECENH_EINVAL, "2 lmax + hop must not exceed nfft");
  if (mode != SPECENH_XWT_POINT && mode != SPECENH_XWT_MEAN)
    return set_error(SPECENH_EINVAL, "mode must be SPECENH_XWT_POINT or SPECENH_XWT_MEAN");
  if (length < 1) return set_error(SPECENH_EINVAL, "length must be >= 1");
  if (mode == SPECENH_XWT_MEAN && length < hop)
    return set_error(SPECENH_EINVAL, "signal shorter than hop");
  return SPECENH_OK;
}

// Vh, V, To, P and the split of the filters over workgroups, for a device of `cus` compute units
long long plan(Args& a, int nscales, int nfft, int lmax, long long batch, long long length,
               long long hop, int mode, int cus) {
  a.S = nscales; a.nfft = nfft; a.log2n = ilog2i(nfft); a.lmax = lmax; a.hop = (int)hop;
  a.length = length;
  a.Vh = (nfft - 2 * lmax) / (int)hop;  // >= 1
  a.V = a.Vh * (int)hop;
  a.mode = mode;
  a.To = mode == SPECENH_XWT_MEAN ? length / hop : (length - 1) / hop + 1;
  a.P = (a.hop + RUN - 1) / RUN;
  const long long nblk = (a.To + a.Vh - 1) / a.Vh;
  // filters per workgroup: as many as leave two workgroups a CU, the rule of specenh_filterbank
  const long long want = 2LL * cus;
  const long long nb0 = batch < 65535 ? batch : 65535;
  a.SC = MAX_SC;
  while (a.SC > MIN_SC && nblk * ((nscales + a.SC - 1) / a.SC) * nb0 < want) a.SC /= 2;
  a.nchunk = (nscales + a.SC - 1) / a.SC;
  return nblk;
}

}  // namespace
}  // namespace specenh

extern "C" {

int specenh_filterbank_cross_chunk(int nscales, int nfft, int lmax, long long batch,
                                   long long length, long long hop, int mode, int cus) {
  using namespace specenh;
  if (int rc = check_shape(nscales, nfft, lmax, batch, length, hop, mode)) return rc;
  if (cus < 0) return set_error(SPECENH_EINVAL, "cus must be >= 0");
  Args a{};
  plan(a, nscales, nfft, lmax, batch, length, hop, mode, cus > 0 ? cus : device_cus());
  return a.SC;
}

int specenh_filterbank_cross(const void* tables, int nscales, int nfft, int lmax, const float* x,
                             const float* y, long long batch, long long length,
                             long long x_stride, long long y_stride, long long hop, int mode,
                             void* sxy, float* sxx, float* syy, void* stream) {
  using namespace specenh;
  if (!tables) return set_error(SPECENH_EINVAL, "null tables");
  if (!x) return set_error(SPECENH_EINVAL, "null x");
  if (!y) return set_error(SPECENH_EINVAL, "null y");
  if (reinterpret_cast<size_t>(tables) % 8)
    return set_error(SPECENH_EINVAL, "tables must be 8-byte aligned");
  if (int rc = check_shape(nscales, nfft, lmax, batch, length, hop, mode)) return rc;
  if (int rc = check_stride(x_stride, length, "x_stride < length")) return rc;
  if (int rc = check_stride(y_stride, length, "y_stride < length")) return rc;
  if (!sxy) return set_error(SPECENH_EINVAL, "null sxy");
  if (!sxx != !syy) return set_error(SPECENH_EINVAL, "sxx and syy must be both given or both null");
  if (batch == 0) return SPECENH_OK;
  Args a{};
  a.tab = reinterpret_cast<const float2*>(tables);
  a.xs = x_stride; a.ys = y_stride;
  const long long nblk = plan(a, nscales, nfft, lmax, batch, length, hop, mode, device_cus());
  const double inv = 1.0 / nfft;
  a.scale = (float)(mode == SPECENH_XWT_POINT ? inv * inv : inv * inv / (double)hop);
  if (nblk * a.nchunk > 2147483647LL) return set_error(SPECENH_EUNSUPPORTED, "too many blocks");
  hipError_t e = allow_lds(g_lds,
                           {(const void*)kernel_for(2048), (const void*)kernel_for(4096)}, MAX_LDS);
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("filterbank_cross: ") + hipGetErrorString(e));
  const size_t lds = ((size_t)2 * nfft + a.V) * sizeof(float2);
  const Kernel kern = kernel_for(nfft);
  for (long long b0 = 0; b0 < batch; b0 += 65535) {  // grid.y limit
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    const size_t at = (size_t)b0 * nscales * a.To;
    a.x = x + b0 * x_stride;
    a.y = y + b0 * y_stride;
    a.sxy = reinterpret_cast<float2*>(sxy) + at;
    a.sxx = sxx ? sxx + at : nullptr;
    a.syy = syy ? syy + at : nullptr;
    launch(kern, dim3((unsigned)(nblk * a.nchunk), (unsigned)nb), dim3(CT), lds, stream, a);
    if (int rc = launched("filterbank_cross")) return rc;
  }
  return SPECENH_OK;
}

}  // extern "C"
