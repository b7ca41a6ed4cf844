// filterbank.hip — a bank of S complex FIR filters applied to real signals for gfx950
// (include/specenh_wavelet.h): the Morlet wavelet transform and FIR band-pass filtering,
//   W[b][s][n] = sum_{m = -L_s .. L_s} h_s[m] x_b[n - m]   (np.convolve(x, h_s), 'same'),
// decimated by hop as complex values, as power, or as the mean power of each hop window.
//
// Overlap-save on one transform length nfft = 256 NI: block q of a shot reads samples
// [q V - Lmax, q V - Lmax + nfft) (zeros outside the shot) and yields outputs
// [q V, q V + V), V = nfft - 2 Lmax rounded down to a multiple of hop; they sit at
// [Lmax, Lmax + V) of the circular convolution, out of the wrap's reach.
//
// filterbank_kernel: a workgroup owns one (block, chunk of SC filters, shot). It loads the
//   block once as nfft complex numbers with zero imaginary part and transforms it (the LDS
//   passes of fft_lds.hpp with the table's twiddle row; from nfft = 1024 up BlockFft, the same
//   passes with the twiddles held in registers); thread t keeps X[t + 256 i] in NI float2
//   registers across the filter loop. Per filter it writes conj(X_k H_s[k]) into the free
//   buffer (H_s was loaded under the previous filter's transform), runs the same forward
//   transform and reads y[i] = conj(F[i]) / nfft (the inverse through the forward transform,
//   as correlation.hip's invert_store), and the mode's epilogue stores the block's V / hop
//   outputs as one contiguous run. The plan, the block load, the row load, the product and the
//   hop epilogue (the fixed-order mean of a hop window) are filterbank_block.hpp's, shared with
//   filterbank_cross.hip.
//
// The products and the inverse transforms never reach memory; no atomics; an element depends
// on its own shot's samples, the tables, hop and mode only.
//
// LDS: two buffers of nfft float2 (4 KiB .. 64 KiB, opted in through allow_lds); no static
// LDS, so the dynamic base is aligned.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "specenh_wavelet.h"
#include "runtime.hpp"
#include "averaging.hpp"  // check_stride
#include "filterbank_block.hpp"

namespace specenh {
namespace {

using namespace filterbank_block;  // the plan, the block pieces and the hop epilogue
using block_fft::BlockFft;
using block_fft::transform;

constexpr int MAX_LDS = 64 * 1024;

struct Args {
  const float2* tab;  // [S + 1][nfft]: H_s, then W_nfft^n
  const float* x;
  long long xs;
  Plan p;
  int mode;
  float scale;   // 1 / nfft (complex), 1 / nfft^2 (power), 1 / (nfft^2 hop) (mean)
  void* out;     // [batch][S][To]
};

// the hop epilogue's view of one filter's result y = conj(W) nfft: |y|^2, stored scaled
struct PowerHop {
  using Acc = float;
  const float2* y;
  float* out;  // at the block's first output
  float sc;
  __device__ float term(int i) const { return power(y[i]); }
  __device__ void store(int jj, float v) const { out[jj] = v * sc; }
};

template <int NI>
__global__ __launch_bounds__(CT) void filterbank_kernel(Args a) {
  extern __shared__ float2 sm[];
  const int n = a.p.nfft, tid = threadIdx.x, S = a.p.S, hop = a.p.hop, lmax = a.p.lmax;
  float2* bufA = sm;
  float2* bufB = sm + n;
  const int q = blockIdx.x / a.p.nchunk, c = blockIdx.x - q * a.p.nchunk;
  const long long b = blockIdx.y;
  load_block<NI>(bufA, a.x + b * a.xs, (long long)q * a.p.V - lmax, a.p.length, tid);
  const float2* tw = a.tab + (long long)S * n;
  BlockFft<NI> fft;
  if constexpr (NI >= 4) fft.init(tw, tid);
  __syncthreads();
  float2* res = transform(fft, bufA, bufB, n, a.p.log2n, tw, tid);
  float2 X[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) X[i] = res[tid + CT * i];
  // the buffer the next product goes to: one that no thread still reads
  float2* cur = res == bufA ? bufB : bufA;
  const long long j0 = (long long)q * a.p.Vh;  // first stored output of the block
  const int cnt = a.p.To - j0 < a.p.Vh ? (int)(a.p.To - j0) : a.p.Vh;  // >= 1: the grid has ceil(To / Vh) blocks
  const int s1 = (c + 1) * a.p.SC < S ? (c + 1) * a.p.SC : S;
  const float sc = a.scale;
  float2 H[NI];  // this filter's row; the next one's is loaded under this filter's transform
  load_row<NI>(H, a.tab, c * a.p.SC, n, tid);
  for (int s = c * a.p.SC; s < s1; ++s) {  // uniform
    store_product<NI>(cur, X, H, tid);
    if (s + 1 < s1) load_row<NI>(H, a.tab, s + 1, n, tid);
    __syncthreads();
    res = transform(fft, cur, cur == bufA ? bufB : bufA, n, a.p.log2n, tw, tid);
    float2* other = res == bufA ? bufB : bufA;
    const float2* y = res + lmax;  // conj(y) * nfft at outputs q V ..
    const long long o = (b * S + s) * a.p.To + j0;
    if (a.mode == SPECENH_FB_COMPLEX) {  // not a sum
      float2* out = reinterpret_cast<float2*>(a.out) + o;
      for (int jj = tid; jj < cnt; jj += CT) {
        const float2 f = y[jj * hop];
        out[jj] = make_float2(f.x * sc, -f.y * sc);
      }
      cur = other;
    } else {
      cur = hop_epilogue(PowerHop{y, reinterpret_cast<float*>(a.out) + o, sc},
                         a.mode == SPECENH_FB_POWER, a.p.P, hop, cnt, res, other, tid);
    }
  }
}

using Kernel = void (*)(Args);
Kernel kernel_for(int nfft) {
  switch (nfft) {
    case 256: return filterbank_kernel<1>;
    case 512: return filterbank_kernel<2>;
    case 1024: return filterbank_kernel<4>;
    case 2048: return filterbank_kernel<8>;
    default: return filterbank_kernel<16>;
  }
}

LdsOptIn g_lds;

// in-place radix-2 fp64 FFT of v[0 .. n), forward; w: exp(-2 pi i k / n), k < n / 2
void fft64(std::vector<double>& re, std::vector<double>& im, const std::vector<double>& wr,
           const std::vector<double>& wi) {
  const int n = (int)re.size();
  for (int i = 1, j = 0; i < n; ++i) {
    int bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) {
      std::swap(re[i], re[j]);
      std::swap(im[i], im[j]);
    }
  }
  for (int len = 2; len <= n; len <<= 1) {
    const int half = len / 2, step = n / len;
    for (int base = 0; base < n; base += len)
      for (int k = 0; k < half; ++k) {
        const double cr = wr[k * step], ci = wi[k * step];
        const int u = base + k, v = u + half;
        const double tr = re[v] * cr - im[v] * ci, ti = re[v] * ci + im[v] * cr;
        re[v] = re[u] - tr;
        im[v] = im[u] - ti;
        re[u] += tr;
        im[u] += ti;
      }
  }
}

}  // namespace
}  // namespace specenh

extern "C" {

int specenh_filterbank_nfft(int lmax, int nfft) {
  using namespace specenh;
  if (lmax < 0 || lmax > SPECENH_FB_MAX_HALF)
    return set_error(SPECENH_EINVAL, "lmax must be in [0, 1024]");
  if (nfft == 0) {
    nfft = 1024;
    while (nfft < 4 * lmax) nfft *= 2;
  }
  if (!allowed_nfft(nfft)) return set_error(SPECENH_EINVAL, NFFT_MSG);
  if (2 * lmax + 1 > nfft) return set_error(SPECENH_EINVAL, "2 lmax + hop must not exceed nfft");
  return nfft;
}

size_t specenh_filterbank_tables_bytes(int nscales, int nfft) {
  using namespace specenh;
  if (nscales < 1) {
    set_error(SPECENH_EINVAL, "nscales must be >= 1");
    return 0;
  }
  if (!allowed_nfft(nfft)) {
    set_error(SPECENH_EINVAL, NFFT_MSG);
    return 0;
  }
  return ((size_t)nscales + 1) * (size_t)nfft * sizeof(float2);
}

int specenh_filterbank_tables(int nscales, const int* half_lengths, const double* taps, int nfft,
                              float* tables_host) {
  using namespace specenh;
  if (!half_lengths) return set_error(SPECENH_EINVAL, "null half_lengths");
  if (!taps) return set_error(SPECENH_EINVAL, "null taps");
  if (!tables_host) return set_error(SPECENH_EINVAL, "null tables");
  if (nscales < 1) return set_error(SPECENH_EINVAL, "nscales must be >= 1");
  if (!allowed_nfft(nfft)) return set_error(SPECENH_EINVAL, NFFT_MSG);
  for (int s = 0; s < nscales; ++s) {
    if (half_lengths[s] < 0 || half_lengths[s] > SPECENH_FB_MAX_HALF)
      return set_error(SPECENH_EINVAL, "half length must be in [0, 1024]");
    if (2 * half_lengths[s] + 1 > nfft)
      return set_error(SPECENH_EINVAL, "filter longer than nfft");
  }
  const double step = -2.0 * M_PI / nfft;
  std::vector<double> wr(nfft), wi(nfft), re(nfft), im(nfft);
  for (int k = 0; k < nfft; ++k) {
    wr[k] = std::cos(step * k);
    wi[k] = std::sin(step * k);
  }
  const double* h = taps;
  for (int s = 0; s < nscales; ++s) {
    const int L = half_lengths[s];
    std::fill(re.begin(), re.end(), 0.0);
    std::fill(im.begin(), im.end(), 0.0);
    for (int m = -L; m <= L; ++m) {
      const int at = (m + nfft) & (nfft - 1);
      re[at] = h[2 * (m + L)];
      im[at] = h[2 * (m + L) + 1];
    }
    h += 2 * (2 * (size_t)L + 1);
    fft64(re, im, wr, wi);
    float* row = tables_host + 2 * (size_t)s * nfft;
    for (int k = 0; k < nfft; ++k) {
      row[2 * k] = (float)re[k];
      row[2 * k + 1] = (float)im[k];
    }
  }
  float* row = tables_host + 2 * (size_t)nscales * nfft;
  for (int k = 0; k < nfft; ++k) {
    row[2 * k] = (float)wr[k];
    row[2 * k + 1] = (float)wi[k];
  }
  return SPECENH_OK;
}

int specenh_filterbank(const void* tables, int nscales, int nfft, int lmax, const float* x,
                       long long batch, long long length, long long x_stride, long long hop,
                       int mode, void* out, void* stream) {
  using namespace specenh;
  if (!tables) return set_error(SPECENH_EINVAL, "null tables");
  if (!x) return set_error(SPECENH_EINVAL, "null x");
  if (reinterpret_cast<size_t>(tables) % 8)
    return set_error(SPECENH_EINVAL, "tables must be 8-byte aligned");
  const bool mean = mode == SPECENH_FB_POWER_MEAN;
  if (int rc = check_shape(
          nscales, nfft, lmax, batch, length, hop,
          mode == SPECENH_FB_COMPLEX || mode == SPECENH_FB_POWER || mean,
          "mode must be SPECENH_FB_COMPLEX, SPECENH_FB_POWER or SPECENH_FB_POWER_MEAN", mean))
    return rc;
  if (int rc = check_stride(x_stride, length, "x_stride < length")) return rc;
  if (!out) return set_error(SPECENH_EINVAL, "null out");
  if (batch == 0) return SPECENH_OK;
  Args a{};
  a.tab = reinterpret_cast<const float2*>(tables);
  a.xs = x_stride;
  a.mode = mode;
  const long long nblk = plan(a.p, nscales, nfft, lmax, batch, length, hop, mean, device_cus());
  const double inv = 1.0 / nfft;
  a.scale = (float)(mode == SPECENH_FB_COMPLEX ? inv
                    : mode == SPECENH_FB_POWER ? inv * inv : inv * inv / (double)hop);
  if (nblk * a.p.nchunk > 2147483647LL) return set_error(SPECENH_EUNSUPPORTED, "too many blocks");
  hipError_t e = allow_lds(g_lds,
                           {(const void*)kernel_for(2048), (const void*)kernel_for(4096)}, MAX_LDS);
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("filterbank: ") + hipGetErrorString(e));
  const size_t lds = (size_t)2 * nfft * sizeof(float2);
  const size_t esize = mode == SPECENH_FB_COMPLEX ? sizeof(float2) : sizeof(float);
  return launch_slices(kernel_for(nfft), a, nblk, batch, lds, stream, "filterbank",
                       [&](long long b0) {
                         a.x = x + b0 * x_stride;
                         a.out = reinterpret_cast<char*>(out) + (size_t)b0 * nscales * a.p.To * esize;
                       });
}

}  // extern "C"
