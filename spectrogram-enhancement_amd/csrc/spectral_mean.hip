// spectral_mean.hip — time-averaged spectra for gfx950: Welch PSD, averaged cross-spectral
// density and magnitude-squared coherence of signal pairs, over the whole shot or over
// blocks of navg frames (scipy.signal.welch / csd / coherence, average='mean').
//
// A workgroup owns one shot and one chunk: a run of at most SPECENH_SPECTRAL_CHUNK
// consecutive frames of one averaging group. Round by round it loads FR frames of x (and the
// same FR frames of y) into LDS, detrends (fp64 sums) and windows them, transforms them side
// by side and adds |X|^2, |Y|^2 and conj(X) Y per bin to fp32 registers. No per-frame
// spectrum goes to memory.
//
// One real frame per transform, nothing shared between two frames or two signals: a frame of
// N reals is read as N/2 complex numbers z_j = v_2j + i v_2j+1, transformed by an N/2-point
// Stockham FFT (the LDS ping-pong passes of fft_lds.hpp with the plan's natural-order
// twiddles at stride 2, after that header's frame front end) and unpacked,
//   X_k = E_k + W_N^k O_k,  2 E_k = Z_k + conj Z_{N/2-k},  2 O_k = -i (Z_k - conj Z_{N/2-k}).
// That is the butterfly count of carrying two real frames in one N-point transform, without
// x's rounding reaching y (or frame 2q's reaching 2q+1): the coherence inherits the pointwise
// error of Pxx where |X_k| << |Y_k|.
//
// Slot p of a round accumulates frames p, p + FR, ... of the chunk in ascending order; the
// slots are then added in ascending p. A group that is one chunk is scaled and stored by the
// same workgroup; otherwise the chunk's fp32 partials go to the workspace and
// spectral_finalize_kernel adds them in fp64 in ascending chunk order. No atomics.
#include <hip/hip_runtime.h>

#include <string>

#include "specenh_spectral.h"
#include "runtime.hpp"
#include "averaging.hpp"
#include "fft_lds.hpp"

namespace specenh {
namespace {

constexpr int CT = 256;  // threads per workgroup
// Frames per chunk. A sequential fp32 sum of C non-negative terms is off by at most C u
// (u = 2^-24) relatively, about sqrt(C) u in practice: 1.9e-6 and 3e-7 at C = 32, below the
// 2e-6 floor of the coherence bound and a fifth of the 1e-5 PSD contract. The price of a
// short chunk is the partial it writes: 16 (N/2 + 1) bytes against 8 C hop bytes of samples
// read, an eighth at hop = N/4.
constexpr int CHUNK = SPECENH_SPECTRAL_CHUNK;
constexpr int MAX_LDS = 64 * 1024;

using namespace fft_lds;  // load_frames, stockham, unpack2, nyquist2

struct Outputs {
  float* pxx;
  float* pyy;
  float2* pxy;
  float* coh;
};

struct Args {
  const float* x;
  const float* y;
  long long xs, ys;  // row strides
  int N, log2n, hop, slots, detrend;
  int glen;  // frames per group
  int ncg;   // chunks per group
  int G;     // groups
  Outputs o;    // [batch][F][G]
  void* ws;     // [batch][G][ncg][F] float4 (pair) or float (x alone); used when ncg > 1
  double m;     // scale / (4 glen): the sums are of |2 X|^2
  const float* win;
  const float2* tw;
};

// One bin of one group from its sums (of |2X|^2, |2Y|^2, conj(2X) 2Y): mean, scale, one-sided
// doubling, coherence. The only place outputs are stored.
__device__ __forceinline__ void store_bin(const Outputs& o, long long at, bool dbl, double m,
                                          double sxx, double syy, double sre, double sim) {
  if (dbl) m *= 2.0;
  if (o.pxx) o.pxx[at] = (float)(sxx * m);
  if (o.pyy) o.pyy[at] = (float)(syy * m);
  if (o.pxy) o.pxy[at] = make_float2((float)(sre * m), (float)(sim * m));
  if (o.coh) o.coh[at] = (float)((sre * sre + sim * sim) / (sxx * syy));
}

// NI = FR * (N/2) / CT bins per thread, FR = frames per round (slots, or slots / 2 with y).
template <int NI, bool PAIR>
__global__ __launch_bounds__(CT) void spectral_mean_kernel(Args a) {
  extern __shared__ float2 sm[];
  __shared__ float stat[32][2];  // per slot: mean, slope
  constexpr int NA = PAIR ? 4 : 1;
  const int N = a.N, M = N / 2, F = M + 1, log2m = a.log2n - 1, tid = threadIdx.x;
  const int S = a.slots, FR = PAIR ? S / 2 : S;
  float2* bufA = sm;
  float2* bufB = sm + S * M;
  float* raw = reinterpret_cast<float*>(bufA);  // slot s: samples [s * N, (s + 1) * N)
  const long long b = blockIdx.y;
  const int g = blockIdx.x / a.ncg, c = blockIdx.x - g * a.ncg;
  const long long f0 = (long long)g * a.glen + (long long)c * CHUNK;  // first frame
  const int left = a.glen - c * CHUNK;
  const int cnt = left < CHUNK ? left : CHUNK;  // >= 1
  const float* xb = a.x + b * a.xs;
  const float* yb = PAIR ? a.y + b * a.ys : nullptr;
  // bins 0 .. M-1 of this thread's slots; the Nyquist bin of all of them (k = 0 threads only)
  float acc[NI][NA], accn[NA];
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    accn[j] = 0.f;
#pragma unroll
    for (int i = 0; i < NI; ++i) acc[i][j] = 0.f;
  }
  for (int r0 = 0; r0 < cnt; r0 += FR) {
    load_frames<CT>(raw, stat, N, a.log2n, S, a.detrend, a.win, tid, [&](int s, int n) {
      const int p = s & (FR - 1);
      const float* src = (PAIR && s >= FR) ? yb : xb;
      // slots past the chunk's end stay zero and add nothing
      return r0 + p < cnt ? src[(f0 + r0 + p) * a.hop + n] : 0.f;
    });
    const float2* res = stockham<CT>(bufA, bufB, M, log2m, S, a.tw, N, tid);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int idx = tid + CT * i, p = idx >> log2m, k = idx & (M - 1);
      const float2 w = a.tw[k];
      const float2* zx = res + p * M;
      const float2 X = unpack2(zx, k, M, w);
      acc[i][0] = fmaf(X.x, X.x, fmaf(X.y, X.y, acc[i][0]));
      if constexpr (PAIR) {
        const float2* zy = res + (FR + p) * M;
        const float2 Y = unpack2(zy, k, M, w);
        acc[i][1] = fmaf(Y.x, Y.x, fmaf(Y.y, Y.y, acc[i][1]));
        acc[i][2] += fmaf(X.x, Y.x, X.y * Y.y);
        acc[i][3] += fmaf(X.x, Y.y, -X.y * Y.x);
        if (k == 0) {
          const float xn = nyquist2(zx), yn = nyquist2(zy);
          accn[0] = fmaf(xn, xn, accn[0]);
          accn[1] = fmaf(yn, yn, accn[1]);
          accn[2] = fmaf(xn, yn, accn[2]);
        }
      } else if (k == 0) {
        const float xn = nyquist2(zx);
        accn[0] = fmaf(xn, xn, accn[0]);
      }
    }
    __syncthreads();  // the next round's loads overwrite the buffers
  }
  float* red = reinterpret_cast<float*>(sm);  // [FR][F][NA] <= the two FFT buffers
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int idx = tid + CT * i, p = idx >> log2m, k = idx & (M - 1);
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      red[(p * F + k) * NA + j] = acc[i][j];
      // a k = 0 thread folds the Nyquist bins of all its slots into one accn: stored once
      if (k == 0) red[(p * F + M) * NA + j] = i == 0 ? accn[j] : 0.f;
    }
  }
  __syncthreads();
  const long long bg = b * a.G + g;
  for (int k = tid; k < F; k += CT) {
    float s[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) s[j] = 0.f;
    for (int p = 0; p < FR; ++p)
#pragma unroll
      for (int j = 0; j < NA; ++j) s[j] += red[(p * F + k) * NA + j];
    if (a.ncg > 1) {  // uniform
      const long long at = (bg * a.ncg + c) * F + k;
      if constexpr (PAIR) reinterpret_cast<float4*>(a.ws)[at] = make_float4(s[0], s[1], s[2], s[3]);
      else reinterpret_cast<float*>(a.ws)[at] = s[0];
    } else {
      double v[4] = {s[0], 0.0, 0.0, 0.0};
      if constexpr (PAIR) { v[1] = s[1]; v[2] = s[2]; v[3] = s[3]; }
      store_bin(a.o, (b * F + k) * a.G + g, k > 0 && k < M, a.m, v[0], v[1], v[2], v[3]);
    }
  }
}

struct FinArgs {
  const void* ws;  // [nb][G][ncg][F]
  long long total;  // nb * G * F
  int F, G, ncg;
  Outputs o;
  double m;
};

// One thread per (shot, group, bin), bins fastest: the chunk partials in fp64, ascending.
template <bool PAIR>
__global__ __launch_bounds__(CT) void spectral_finalize_kernel(FinArgs a) {
  const long long idx = (long long)blockIdx.x * CT + threadIdx.x;
  if (idx >= a.total) return;
  const int k = (int)(idx % a.F);
  const long long bg = idx / a.F;
  const int g = (int)(bg % a.G);
  const long long b = bg / a.G;
  const long long base = bg * a.ncg * a.F + k;
  double sxx = 0.0, syy = 0.0, sre = 0.0, sim = 0.0;
  for (int c = 0; c < a.ncg; ++c) {
    const long long at = base + (long long)c * a.F;
    if (PAIR) {
      const float4 v = reinterpret_cast<const float4*>(a.ws)[at];
      sxx += v.x; syy += v.y; sre += v.z; sim += v.w;
    } else {
      sxx += reinterpret_cast<const float*>(a.ws)[at];
    }
  }
  store_bin(a.o, (b * a.F + k) * a.G + g, k > 0 && k < a.F - 1, a.m, sxx, syy, sre, sim);
}

using MeanKernel = void (*)(Args);
// NI = slots N / (PAIR ? 1024 : 512)
MeanKernel mean_kernel(int N, bool pair) {
  if (pair) return N <= 1024 ? spectral_mean_kernel<2, true>
                 : N == 2048 ? spectral_mean_kernel<4, true> : spectral_mean_kernel<8, true>;
  return N <= 1024 ? spectral_mean_kernel<4, false>
       : N == 2048 ? spectral_mean_kernel<8, false> : spectral_mean_kernel<16, false>;
}

// N = 4096 takes 64 KiB of dynamic LDS next to the static stat[]: the attribute on every kernel
LdsOptIn g_lds;
hipError_t allow_mean_lds() {
  return allow_lds(g_lds,
                   {(const void*)mean_kernel(1024, false), (const void*)mean_kernel(1024, true),
                    (const void*)mean_kernel(2048, false), (const void*)mean_kernel(2048, true),
                    (const void*)mean_kernel(4096, false), (const void*)mean_kernel(4096, true)},
                   MAX_LDS);
}

}  // namespace
}  // namespace specenh

extern "C" {

long long specenh_spectral_groups(long long frames, long long navg) {
  using specenh::set_error;
  if (frames < 1) return set_error(SPECENH_EINVAL, "at least one frame is needed");
  if (navg <= 0) return 1;
  if (navg > frames) return set_error(SPECENH_EINVAL, "navg exceeds the number of frames");
  return frames / navg;
}

size_t specenh_spectral_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                        long long length, long long navg) {
  using namespace specenh;
  FrameSplit s;
  if (check_call(plan, batch, length, navg, false, &s) != SPECENH_OK || s.ncg == 1) return 0;
  return (size_t)batch * s.G * s.ncg * (plan->nperseg / 2 + 1) * sizeof(float4);
}

int specenh_spectral_mean(const specenh_stft_plan* plan, const float* x, const float* y,
                          long long batch, long long length, long long x_stride,
                          long long y_stride, long long navg, float* pxx, float* pyy, void* pxy,
                          float* coh, void* workspace, void* stream) {
  using namespace specenh;
  if (!x) return set_error(SPECENH_EINVAL, "null x");
  FrameSplit s;
  if (int rc = check_call(plan, batch, length, navg, false, &s)) return rc;
  const SignalArg in[] = {{x, x_stride, "x_stride < length"}, {y, y_stride, "y_stride < length"}};
  if (int rc = check_strides(in, 2, length)) return rc;
  const int N = plan->nperseg;
  if (!y && (pyy || pxy || coh))
    return set_error(SPECENH_EINVAL, "pyy, pxy and coh need a second signal y");
  if (!pxx && !pyy && !pxy && !coh) return set_error(SPECENH_EINVAL, "no output requested");
  if (batch == 0) return SPECENH_OK;
  if (s.ncg > 1 && !workspace) return set_error(SPECENH_EINVAL, "null workspace");
  if (s.G * s.ncg > 2147483647LL) return set_error(SPECENH_EUNSUPPORTED, "too many chunks");
  if (s.ncg > 1 && (65535 * s.G * (N / 2 + 1) + CT - 1) / CT > 2147483647LL)
    return set_error(SPECENH_EUNSUPPORTED, "too many groups");
  const long long F = N / 2 + 1;
  const bool pair = y != nullptr;
  hipError_t e = allow_mean_lds();
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("spectral_mean: ") + hipGetErrorString(e));
  Args a{};
  a.xs = x_stride; a.ys = y_stride;
  a.N = N; a.log2n = ilog2i(N); a.hop = plan->hop; a.slots = slots_for(N);
  a.detrend = plan->detrend;
  a.glen = (int)s.glen; a.ncg = (int)s.ncg; a.G = (int)s.G;
  a.m = plan->scale / (4.0 * (double)s.glen);
  a.win = plan->d_window; a.tw = plan->d_tw_nat;
  const size_t lds = (size_t)a.slots * N * sizeof(float2);  // two buffers of slots * N/2
  const size_t ws_elem = pair ? sizeof(float4) : sizeof(float);
  const MeanKernel kern = mean_kernel(N, pair);
  for (long long b0 = 0; b0 < batch; b0 += 65535) {  // grid.y limit
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    a.x = x + b0 * x_stride;
    a.y = pair ? y + b0 * y_stride : nullptr;
    const long long o0 = b0 * F * s.G;
    a.o.pxx = pxx ? pxx + o0 : nullptr;
    a.o.pyy = pyy ? pyy + o0 : nullptr;
    a.o.pxy = pxy ? reinterpret_cast<float2*>(pxy) + o0 : nullptr;
    a.o.coh = coh ? coh + o0 : nullptr;
    a.ws = s.ncg > 1 ? (char*)workspace + (size_t)(b0 * s.G * s.ncg * F) * ws_elem : nullptr;
    launch(kern, dim3((unsigned)(s.G * s.ncg), (unsigned)nb), dim3(CT), lds, stream, a);
    if (int rc = launched("spectral_mean")) return rc;
    if (s.ncg == 1) continue;
    FinArgs f{};
    f.ws = a.ws; f.total = nb * s.G * F; f.F = (int)F; f.G = (int)s.G; f.ncg = (int)s.ncg;
    f.o = a.o; f.m = a.m;
    const long long blocks = (f.total + CT - 1) / CT;
    if (pair)
      SPECENH_LAUNCH(spectral_finalize_kernel<true>, dim3((unsigned)blocks), dim3(CT), 0,
                     (hipStream_t)stream, f);
    else
      SPECENH_LAUNCH(spectral_finalize_kernel<false>, dim3((unsigned)blocks), dim3(CT), 0,
                     (hipStream_t)stream, f);
    if (int rc = launched("spectral_finalize")) return rc;
  }
  return SPECENH_OK;
}

}  // extern "C"
