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
//   outputs as one contiguous run.
//   The mean of a hop window is a fixed-order sum: runs of 16 consecutive |y|^2 are summed
//   in ascending order, then the runs in ascending order; the order depends on hop alone.
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
#include "averaging.hpp"  // check_stride, launch, launched
#include "block_fft.hpp"  // BlockFft, transform

namespace specenh {
namespace {

using block_fft::BlockFft;
using block_fft::CT;  // threads per workgroup
using block_fft::c_mul;
using block_fft::transform;

constexpr int RUN = 16;   // |y|^2 values a thread sums in a row for the hop mean
constexpr int MAX_SC = 16;  // filters per workgroup at most: the block's transform is 1/17 of its work
constexpr int MIN_SC = 4;
constexpr int MAX_LDS = 64 * 1024;

struct Args {
  const float2* tab;  // [S + 1][nfft]: H_s, then W_nfft^n
  const float* x;
  long long xs, length;
  long long To;  // outputs per (shot, filter)
  int S, nfft, log2n, lmax, hop;
  int V, Vh;     // outputs of W per block, stored outputs per block (V / hop)
  int SC, nchunk;
  int mode;
  int P;         // runs per hop window (mean mode): ceil(hop / RUN)
  float scale;   // 1 / nfft (complex), 1 / nfft^2 (power), 1 / (nfft^2 hop) (mean)
  void* out;     // [batch][S][To]
};

template <int NI>
__global__ __launch_bounds__(CT) void filterbank_kernel(Args a) {
  extern __shared__ float2 sm[];
  const int n = a.nfft, tid = threadIdx.x, S = a.S, hop = a.hop, lmax = a.lmax;
  float2* bufA = sm;
  float2* bufB = sm + n;
  const int q = blockIdx.x / a.nchunk, c = blockIdx.x - q * a.nchunk;
  const long long b = blockIdx.y;
  const float* xb = a.x + b * a.xs;
  const long long n0 = (long long)q * a.V - lmax;  // first sample of the block
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int k = tid + CT * i;
    const long long t = n0 + k;
    bufA[k] = make_float2(t >= 0 && t < a.length ? xb[t] : 0.f, 0.f);
  }
  const float2* tw = a.tab + (long long)S * n;
  BlockFft<NI> fft;
  if constexpr (NI >= 4) fft.init(tw, tid);
  __syncthreads();
  float2* res = transform(fft, bufA, bufB, n, a.log2n, tw, tid);
  float2 X[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) X[i] = res[tid + CT * i];
  // the buffer the next product goes to: one that no thread still reads
  float2* cur = res == bufA ? bufB : bufA;
  const long long j0 = (long long)q * a.Vh;  // first stored output of the block
  const int cnt = a.To - j0 < a.Vh ? (int)(a.To - j0) : a.Vh;  // >= 1: the grid has ceil(To / Vh) blocks
  const int s1 = (c + 1) * a.SC < S ? (c + 1) * a.SC : S;
  const float sc = a.scale;
  float2 H[NI];  // this filter's row; the next one's is loaded under this filter's transform
#pragma unroll
  for (int i = 0; i < NI; ++i) H[i] = a.tab[(long long)(c * a.SC) * n + tid + CT * i];
  for (int s = c * a.SC; s < s1; ++s) {  // uniform
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const float2 p = c_mul(X[i], H[i]);
      cur[tid + CT * i] = make_float2(p.x, -p.y);
    }
    if (s + 1 < s1) {
#pragma unroll
      for (int i = 0; i < NI; ++i) H[i] = a.tab[(long long)(s + 1) * n + tid + CT * i];
    }
    __syncthreads();
    res = transform(fft, cur, cur == bufA ? bufB : bufA, n, a.log2n, tw, tid);
    float2* other = res == bufA ? bufB : bufA;
    const float2* y = res + lmax;  // conj(y) * nfft at outputs q V ..
    const long long o = (b * S + s) * a.To + j0;
    cur = other;
    if (a.mode == SPECENH_FB_COMPLEX) {
      float2* out = reinterpret_cast<float2*>(a.out) + o;
      for (int jj = tid; jj < cnt; jj += CT) {
        const float2 f = y[jj * hop];
        out[jj] = make_float2(f.x * sc, -f.y * sc);
      }
    } else if (a.mode == SPECENH_FB_POWER) {
      float* out = reinterpret_cast<float*>(a.out) + o;
      for (int jj = tid; jj < cnt; jj += CT) {
        const float2 f = y[jj * hop];
        out[jj] = fmaf(f.x, f.x, f.y * f.y) * sc;
      }
    } else if (a.P == 1) {  // mean over a window of at most RUN values: one thread, ascending
      float* out = reinterpret_cast<float*>(a.out) + o;
      for (int jj = tid; jj < cnt; jj += CT) {
        float acc = 0.f;
        for (int i = 0; i < hop; ++i) {
          const float2 f = y[jj * hop + i];
          acc += fmaf(f.x, f.x, f.y * f.y);
        }
        out[jj] = acc * sc;
      }
    } else {  // runs of RUN values into the free buffer, then the runs of a window, ascending
      float* part = reinterpret_cast<float*>(other);  // cnt * P <= V / 8 floats
      const int P = a.P;
      for (int idx = tid; idx < cnt * P; idx += CT) {
        const int jj = idx / P, p = idx - jj * P;
        const int i1 = (p + 1) * RUN < hop ? (p + 1) * RUN : hop;
        float acc = 0.f;
        for (int i = p * RUN; i < i1; ++i) {
          const float2 f = y[jj * hop + i];
          acc += fmaf(f.x, f.x, f.y * f.y);
        }
        part[idx] = acc;
      }
      __syncthreads();
      float* out = reinterpret_cast<float*>(a.out) + o;
      for (int jj = tid; jj < cnt; jj += CT) {
        float acc = 0.f;
        for (int p = 0; p < P; ++p) acc += part[jj * P + p];
        out[jj] = acc * sc;
      }
      cur = res;  // `other` is still being read; every thread is past the barrier, done with res
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

bool allowed_nfft(int nfft) {
  return nfft == 256 || nfft == 512 || nfft == 1024 || nfft == 2048 || nfft == 4096;
}

const char* const NFFT_MSG = "nfft must be 256, 512, 1024, 2048 or 4096";

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
  if (nscales < 1) return set_error(SPECENH_EINVAL, "nscales must be >= 1");
  if (!allowed_nfft(nfft)) return set_error(SPECENH_EINVAL, NFFT_MSG);
  if (lmax < 0 || lmax > SPECENH_FB_MAX_HALF)
    return set_error(SPECENH_EINVAL, "lmax must be in [0, 1024]");
  if (batch < 0) return set_error(SPECENH_EINVAL, "batch must be >= 0");
  if (hop < 1) return set_error(SPECENH_EINVAL, "hop must be >= 1");
  if (2LL * lmax + hop > nfft)
    return set_error(SPECENH_EINVAL, "2 lmax + hop must not exceed nfft");
  if (mode != SPECENH_FB_COMPLEX && mode != SPECENH_FB_POWER && mode != SPECENH_FB_POWER_MEAN)
    return set_error(SPECENH_EINVAL,
                     "mode must be SPECENH_FB_COMPLEX, SPECENH_FB_POWER or SPECENH_FB_POWER_MEAN");
  if (length < 1) return set_error(SPECENH_EINVAL, "length must be >= 1");
  if (mode == SPECENH_FB_POWER_MEAN && length < hop)
    return set_error(SPECENH_EINVAL, "signal shorter than hop");
  if (int rc = check_stride(x_stride, length, "x_stride < length")) return rc;
  if (!out) return set_error(SPECENH_EINVAL, "null out");
  if (batch == 0) return SPECENH_OK;
  Args a{};
  a.tab = reinterpret_cast<const float2*>(tables);
  a.xs = x_stride; a.length = length;
  a.S = nscales; a.nfft = nfft; a.log2n = ilog2i(nfft); a.lmax = lmax; a.hop = (int)hop;
  a.Vh = (nfft - 2 * lmax) / (int)hop;  // >= 1
  a.V = a.Vh * (int)hop;
  a.mode = mode;
  a.To = mode == SPECENH_FB_POWER_MEAN ? length / hop : (length - 1) / hop + 1;
  a.P = (a.hop + RUN - 1) / RUN;
  const double inv = 1.0 / nfft;
  a.scale = (float)(mode == SPECENH_FB_COMPLEX ? inv
                    : mode == SPECENH_FB_POWER ? inv * inv : inv * inv / (double)hop);
  const long long nblk = (a.To + a.Vh - 1) / a.Vh;
  // filters per workgroup: as many as leave two workgroups a CU (a single shot fills the chip)
  const long long want = 2LL * device_cus();
  const long long nb0 = batch < 65535 ? batch : 65535;
  a.SC = MAX_SC;
  while (a.SC > MIN_SC && nblk * ((nscales + a.SC - 1) / a.SC) * nb0 < want) a.SC /= 2;
  a.nchunk = (nscales + a.SC - 1) / a.SC;
  if (nblk * a.nchunk > 2147483647LL) return set_error(SPECENH_EUNSUPPORTED, "too many blocks");
  hipError_t e = allow_lds(g_lds,
                           {(const void*)kernel_for(2048), (const void*)kernel_for(4096)}, MAX_LDS);
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("filterbank: ") + hipGetErrorString(e));
  const size_t lds = (size_t)2 * nfft * sizeof(float2);
  const size_t esize = mode == SPECENH_FB_COMPLEX ? sizeof(float2) : sizeof(float);
  const Kernel kern = kernel_for(nfft);
  for (long long b0 = 0; b0 < batch; b0 += 65535) {  // grid.y limit
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    a.x = x + b0 * x_stride;
    a.out = reinterpret_cast<char*>(out) + (size_t)b0 * nscales * a.To * esize;
    launch(kern, dim3((unsigned)(nblk * a.nchunk), (unsigned)nb), dim3(CT), lds, stream, a);
    if (int rc = launched("filterbank")) return rc;
  }
  return SPECENH_OK;
}

}  // extern "C"
