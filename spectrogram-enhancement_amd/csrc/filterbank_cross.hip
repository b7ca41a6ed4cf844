// filterbank_cross.hip — the cross spectrum of two real signals through one bank of S complex
// FIR filters for gfx950 (include/specenh_wavelet_cross.h): with W of specenh_wavelet.h,
//   sxy = conj(Wx) Wy,  sxx = |Wx|^2,  syy = |Wy|^2
// at every hop-th sample, or their means over each whole window of hop samples: the
// cross-wavelet spectrum and the spectra wavelet coherence is formed from.
//
// The decomposition, the tables, the block length V and the zero extension are those of
// filterbank.hip, taken from filterbank_block.hpp. filterbank_cross_kernel: a workgroup owns one
// (block, chunk of SC filters, pair). It transforms the block of x and the block of y
// (block_fft.hpp) and keeps both spectra in registers, thread t holding X[t + 256 i] and
// Y[t + 256 i]. Per filter it writes
// conj(X_k H_s[k]) into the free buffer and transforms it, copies the V outputs the block
// yields, [Lmax, Lmax + V) of the result (conj(Wx) nfft, the inverse through the forward
// transform), to a strip of their own, so that they survive Wy's ping-pong transform, and does
// the same with Y in the two transform buffers. The epilogue reads the strip and Wy's result and
// stores the block's V / hop outputs of each of the three arrays as one contiguous run.
//   The mean of a hop window is hop_epilogue's fixed-order sum, as in filterbank_kernel; the
//   four partial sums of a run (re, im, xx, yy) go to the buffer Wy's transform leaves free.
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
#include "averaging.hpp"  // check_stride
#include "filterbank_block.hpp"

namespace specenh {
namespace {

using namespace filterbank_block;  // the plan, the block pieces and the hop epilogue
using block_fft::BlockFft;
using block_fft::transform;

constexpr int MAX_LDS = 96 * 1024;

struct Args {
  const float2* tab;  // [S + 1][nfft]: H_s, then W_nfft^n
  const float* x;
  const float* y;
  long long xs, ys;
  Plan p;
  int mode;
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

// the hop epilogue's view of one filter's results fx = conj(Wx) nfft, fy = conj(Wy) nfft:
// (re, im of conj(Wx) Wy, |Wx|^2, |Wy|^2) nfft^2, stored scaled at o, the block's first output
struct CrossHop {
  using Acc = float4;
  const float2 *fx, *fy;
  float2* sxy;
  float *sxx, *syy;
  long long o;
  float sc;
  bool autos;
  __device__ float4 term(int i) const {
    const float2 u = fx[i], v = fy[i];
    const float2 p = cross(u, v);
    return make_float4(p.x, p.y, power(u), power(v));
  }
  __device__ void store(int jj, const float4& v) const {
    sxy[o + jj] = make_float2(v.x * sc, v.y * sc);
    if (autos) {
      sxx[o + jj] = v.z * sc;
      syy[o + jj] = v.w * sc;
    }
  }
};

template <int NI>
__global__ __launch_bounds__(CT) void filterbank_cross_kernel(Args a) {
  extern __shared__ __align__(16) float2 sm[];  // the partial sums are stored as float4
  const int n = a.p.nfft, tid = threadIdx.x, S = a.p.S, hop = a.p.hop, lmax = a.p.lmax;
  float2* const strip = sm + 2 * n;  // V float2: Wx's outputs while Wy is transformed
  auto other = [&](const float2* p) { return p == sm ? sm + n : sm; };  // of the two transform buffers
  const int q = blockIdx.x / a.p.nchunk, c = blockIdx.x - q * a.p.nchunk;
  const long long b = blockIdx.y;
  const long long n0 = (long long)q * a.p.V - lmax;  // first sample of the block
  const float2* tw = a.tab + (long long)S * n;
  BlockFft<NI> fft;
  if constexpr (NI >= 4) fft.init(tw, tid);
  float2 X[NI], Y[NI];
  load_block<NI>(sm, a.x + b * a.xs, n0, a.p.length, tid);
  __syncthreads();
  float2* res = transform(fft, sm, sm + n, n, a.p.log2n, tw, tid);
#pragma unroll
  for (int i = 0; i < NI; ++i) X[i] = res[tid + CT * i];
  load_block<NI>(other(res), a.y + b * a.ys, n0, a.p.length, tid);  // X is still being read from res
  __syncthreads();
  res = transform(fft, other(res), res, n, a.p.log2n, tw, tid);
#pragma unroll
  for (int i = 0; i < NI; ++i) Y[i] = res[tid + CT * i];
  // the buffer the next product of X goes to: one that no thread still reads
  float2* cur = other(res);
  const long long j0 = (long long)q * a.p.Vh;  // first stored output of the block
  const int cnt = a.p.To - j0 < a.p.Vh ? (int)(a.p.To - j0) : a.p.Vh;  // >= 1: the grid has ceil(To / Vh) blocks
  const int s1 = (c + 1) * a.p.SC < S ? (c + 1) * a.p.SC : S;
  const bool autos = a.sxx != nullptr;  // uniform
  float2 H[NI];  // this filter's row; the next one's is loaded under Wy's transform
  load_row<NI>(H, a.tab, c * a.p.SC, n, tid);
  for (int s = c * a.p.SC; s < s1; ++s) {  // uniform
    store_product<NI>(cur, X, H, tid);
    __syncthreads();  // every thread is done with the previous filter's buffers
    float2* rx = transform(fft, cur, other(cur), n, a.p.log2n, tw, tid);
    // Wx's outputs to the strip (the previous filter's were last read before the barrier
    // above), the product of Y beside them; rx's transform ended on a barrier
    for (int k = tid; k < a.p.V; k += CT) strip[k] = rx[lmax + k];
    float2* py = other(rx);
    store_product<NI>(py, Y, H, tid);
    if (s + 1 < s1) load_row<NI>(H, a.tab, s + 1, n, tid);
    __syncthreads();  // the strip is whole, rx is free
    float2* ry = transform(fft, py, rx, n, a.p.log2n, tw, tid);
    // conj(Wx) * nfft at outputs q V .. in the strip, conj(Wy) * nfft in ry
    const CrossHop h{strip, ry + lmax, a.sxy, a.sxx, a.syy, (b * S + s) * a.p.To + j0, a.scale,
                     autos};
    cur = hop_epilogue(h, a.mode == SPECENH_XWT_POINT, a.p.P, hop, cnt, ry, other(ry), tid);
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

// check_shape with this entry's modes
int check_cross(int nscales, int nfft, int lmax, long long batch, long long length, long long hop,
                int mode) {
  return check_shape(nscales, nfft, lmax, batch, length, hop,
                     mode == SPECENH_XWT_POINT || mode == SPECENH_XWT_MEAN,
                     "mode must be SPECENH_XWT_POINT or SPECENH_XWT_MEAN", mode == SPECENH_XWT_MEAN);
}

}  // namespace
}  // namespace specenh

extern "C" {

int specenh_filterbank_cross_chunk(int nscales, int nfft, int lmax, long long batch,
                                   long long length, long long hop, int mode, int cus) {
  using namespace specenh;
  if (int rc = check_cross(nscales, nfft, lmax, batch, length, hop, mode)) return rc;
  if (cus < 0) return set_error(SPECENH_EINVAL, "cus must be >= 0");
  Plan p{};
  plan(p, nscales, nfft, lmax, batch, length, hop, mode == SPECENH_XWT_MEAN,
       cus > 0 ? cus : device_cus());
  return p.SC;
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
  if (int rc = check_cross(nscales, nfft, lmax, batch, length, hop, mode)) return rc;
  if (int rc = check_stride(x_stride, length, "x_stride < length")) return rc;
  if (int rc = check_stride(y_stride, length, "y_stride < length")) return rc;
  if (!sxy) return set_error(SPECENH_EINVAL, "null sxy");
  if (!sxx != !syy) return set_error(SPECENH_EINVAL, "sxx and syy must be both given or both null");
  if (batch == 0) return SPECENH_OK;
  Args a{};
  a.tab = reinterpret_cast<const float2*>(tables);
  a.xs = x_stride; a.ys = y_stride;
  a.mode = mode;
  const long long nblk = plan(a.p, nscales, nfft, lmax, batch, length, hop,
                              mode == SPECENH_XWT_MEAN, device_cus());
  const double inv = 1.0 / nfft;
  a.scale = (float)(mode == SPECENH_XWT_POINT ? inv * inv : inv * inv / (double)hop);
  if (nblk * a.p.nchunk > 2147483647LL) return set_error(SPECENH_EUNSUPPORTED, "too many blocks");
  hipError_t e = allow_lds(g_lds,
                           {(const void*)kernel_for(2048), (const void*)kernel_for(4096)}, MAX_LDS);
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("filterbank_cross: ") + hipGetErrorString(e));
  const size_t lds = ((size_t)2 * nfft + a.p.V) * sizeof(float2);
  return launch_slices(kernel_for(nfft), a, nblk, batch, lds, stream, "filterbank_cross",
                       [&](long long b0) {
                         const size_t at = (size_t)b0 * nscales * a.p.To;
                         a.x = x + b0 * x_stride;
                         a.y = y + b0 * y_stride;
                         a.sxy = reinterpret_cast<float2*>(sxy) + at;
                         a.sxx = sxx ? sxx + at : nullptr;
                         a.syy = syy ? syy + at : nullptr;
                       });
}

}  // extern "C"
