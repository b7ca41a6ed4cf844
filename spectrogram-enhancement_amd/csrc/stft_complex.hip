// stft_complex.hip — batched complex STFT and inverse STFT (overlap-add) for gfx950.
//
// The return path from a denoised spectrogram to a denoised signal: scipy.signal.stft and
// scipy.signal.istft semantics (scipy/signal/_spectral_py.py) for power-of-two nperseg in
// [64, 4096], fp32 samples, complex64 spectra [batch][F][T] frequency-major, F = N/2 + 1.
//
// Both directions run the mixed-radix Stockham FFT of fft_lds.hpp (one radix-2 pass when
// log2 N is odd, then radix-4, in LDS ping-pong buffers) with the plan's natural-order
// twiddles W_N^n, P transforms side by side per workgroup, and carry two real frames per
// complex transform:
//   forward  z = a + i b,  A_k = (Z_k + conj Z_{N-k}) / 2,  B_k = (Z_k - conj Z_{N-k}) / 2i;
//   inverse  X = Afull + i Bfull over all N bins (Hermitian extensions),
//            a + i b = conj(FFT(conj X)) / N  — the forward passes again.
// Frames are paired (2q, 2q + 1) and tiled from multiples of TF whatever the workgroup, so
// a frame's bits do not depend on how the work was split.
//
// Forward: a workgroup owns TF consecutive frames of one shot. Samples are loaded coalesced
// with the zero-extension predicate (boundary / padding are never materialised), detrended
// per frame after the zeros are in place, windowed, transformed, separated into a
// (bins x frames) LDS tile and stored as whole frequency-row segments.
//
// Inverse: a workgroup owns SPAN consecutive output samples, 16 per thread in registers. It
// stages the bins of every frame that touches the span (gain multiplied on the load),
// inverts them pair by pair and each thread GATHERS its samples' contributions in ascending
// frame order, together with norm = sum w^2 over the frames that exist. No atomics; every
// output sample is written once; the edge frames are recomputed by both neighbours. The few
// samples whose norm is tiny but above scipy's 1e-10 cut are recomputed in fp64 (edge_sample).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "specenh_stft_complex.h"
#include "runtime.hpp"
#include "stft_plan.hpp"
#include "fft_lds.hpp"

namespace specenh {
namespace {

using namespace fft_lds;  // stockham

constexpr int CT = 256;            // threads per workgroup
constexpr int SPT = 16;            // inverse: output samples per thread
constexpr int SPAN = CT * SPT;     // inverse: output samples per workgroup
constexpr int MAX_LDS = 136 * 1024;

// P transforms side by side (P * N / 4 radix-4 butterflies per pass >= 256 where LDS
// allows), TF frames per tile (TF / 2P rounds of P frame pairs).
struct Cfg {
  int P, TF;
};
inline Cfg cfg_for(int N) {
  switch (N) {
    case 64: return {16, 32};
    case 128: return {8, 16};
    case 256: return {4, 16};
    case 512: return {2, 8};
    case 1024: return {1, 8};
    case 2048: return {1, 4};
    default: return {1, 2};
  }
}
inline size_t fft_tile_bytes(int N, Cfg c) {
  return ((size_t)2 * c.P * N + (size_t)(N / 2 + 1) * (c.TF + 1)) * sizeof(float2);
}

// ------------------------------------------------------------------------- forward
struct FwdArgs {
  const float* x;
  long long xs, L, T;  // row stride, samples per shot, frames
  float2* out;         // [batch][F][T]
  int N, log2n, hop, pad, P, TF, log2tf, detrend;
  float rs;  // sqrt(scale) / 2 (the 1/2 of the pair separation folded in)
  const float* win;
  const float2* tw;
};

__global__ __launch_bounds__(CT) void stft_complex_kernel(FwdArgs a) {
  extern __shared__ float2 sm[];
  __shared__ float stat[32][2];  // per frame of the round: mean, slope
  const int N = a.N, P = a.P, TF = a.TF, F = N / 2 + 1, tid = threadIdx.x;
  float2* bufA = sm;
  float2* bufB = sm + P * N;
  float2* tile = sm + 2 * P * N;  // [F][TF + 1]
  const long long b = blockIdx.y, t0 = (long long)blockIdx.x * TF;
  const float* xb = a.x + b * a.xs;
  const float kc = 0.5f * (N - 1);
  const int rounds = TF / (2 * P);
  for (int r = 0; r < rounds; ++r) {
    const long long tr = t0 + (long long)r * 2 * P;
    if (tr >= a.T) break;  // uniform
    for (int idx = tid; idx < P * N; idx += CT) {
      const int p = idx >> a.log2n, n = idx & (N - 1);
      const long long ta = tr + 2 * p;
      const long long ia = ta * a.hop + n - a.pad, ib = ia + a.hop;
      const float va = (ta < a.T && ia >= 0 && ia < a.L) ? xb[ia] : 0.f;
      const float vb = (ta + 1 < a.T && ib >= 0 && ib < a.L) ? xb[ib] : 0.f;
      const float w = a.detrend == SPECENH_DETREND_NONE ? a.win[n] : 1.f;  // no detrend: window now
      bufA[idx] = make_float2(va * w, vb * w);
    }
    __syncthreads();
    if (a.detrend != SPECENH_DETREND_NONE) {  // uniform; fp64 sums, one wave per pair
      for (int p = tid >> 6; p < P; p += CT / 64) {
        double sx = 0.0, skx = 0.0, sy = 0.0, sky = 0.0;
        for (int n = tid & 63; n < N; n += 64) {
          const float2 v = bufA[p * N + n];
          const double k = (double)n - 0.5 * (N - 1);
          sx += v.x; skx += k * v.x; sy += v.y; sky += k * v.y;
        }
        sx = wave_sum(sx); skx = wave_sum(skx); sy = wave_sum(sy); sky = wave_sum(sky);
        if ((tid & 63) == 0) {
          const double skk = (double)N * ((double)N * N - 1.0) / 12.0;
          const bool lin = a.detrend == SPECENH_DETREND_LINEAR;
          stat[2 * p][0] = (float)(sx / N);
          stat[2 * p][1] = lin ? (float)(skx / skk) : 0.f;
          stat[2 * p + 1][0] = (float)(sy / N);
          stat[2 * p + 1][1] = lin ? (float)(sky / skk) : 0.f;
        }
      }
      __syncthreads();
      for (int idx = tid; idx < P * N; idx += CT) {
        const int p = idx >> a.log2n, n = idx & (N - 1);
        const float k = (float)n - kc, w = a.win[n];
        const float2 v = bufA[idx];
        bufA[idx] = make_float2((v.x - stat[2 * p][0] - stat[2 * p][1] * k) * w,
                                (v.y - stat[2 * p + 1][0] - stat[2 * p + 1][1] * k) * w);
      }
      __syncthreads();
    }
    const float2* res = stockham<CT>(bufA, bufB, N, a.log2n, P, a.tw, N, tid);
    for (int idx = tid; idx < P * F; idx += CT) {
      const int p = idx / F, k = idx - p * F;
      const float2 z = res[p * N + k], zc = res[p * N + ((N - k) & (N - 1))];
      float2* o = tile + k * (TF + 1) + r * 2 * P + 2 * p;
      o[0] = make_float2(a.rs * (z.x + zc.x), a.rs * (z.y - zc.y));
      o[1] = make_float2(a.rs * (z.y + zc.y), a.rs * (zc.x - z.x));
    }
    __syncthreads();
  }
  const long long left = a.T - t0;
  const int nv = left < TF ? (int)left : TF;
  float2* ob = a.out + b * F * a.T + t0;
  for (int idx = tid; idx < F * TF; idx += CT) {
    const int tl = idx & (TF - 1), k = idx >> a.log2tf;
    if (tl < nv) ob[(long long)k * a.T + tl] = tile[k * (TF + 1) + tl];
  }
}

// ------------------------------------------------------------------------- inverse
struct InvArgs {
  const float2* Z;    // [batch][F][T]
  const float* gain;  // [batch][gain_rows][T] or null
  int gain_rows;
  int T;              // frames
  float* out;         // [batch][n_out], row stride os
  long long os, n_out;
  int N, log2n, hop, trim, P, TF, log2tf;
  float c;    // sum(w) or sqrt(fs sum(w^2)), over N
  double cd;  // the same in fp64 (edge_sample)
  const float* win;
  const float2* tw;
};

// Below this norm a sample is recomputed in fp64 (edge_sample). The fp32 transform leaves an
// error of about 1e-7 of the frame's largest sample on every y_t[n]; the division by norm
// turns it into 1e-7 / sqrt(norm) of the output where one frame covers the sample, so a
// norm under 4e-3 would cost more than 2e-6 of the 1e-5 contract. Only the first and last
// samples of a boundary=False inverse under a window that falls to zero (hann) get here,
// or a window / hop pair on the brink of failing NOLA.
constexpr float EDGE_NRM = 4e-3f;

// One output sample straight from the definition in fp64: the inverse DFT of every frame
// lo..hi at this sample (exact sincospi twiddles), window, norm, scale.
__device__ __forceinline__ float edge_sample(const InvArgs& a, const float2* __restrict__ Zb,
                                          const float* __restrict__ gb, long long e, int lo,
                                          int hi) {
  const int N = a.N;
  double acc = 0.0, nrm = 0.0;
  for (int t = lo; t <= hi; ++t) {
    const int n = (int)(e - (long long)t * a.hop);
    const double w = (double)a.win[n];
    double s = 0.0;
    for (int k = 0; k <= N / 2; ++k) {
      const float2 z = Zb[(long long)k * a.T + t];
      double g = 1.0;
      if (gb) g = k < a.gain_rows ? (double)gb[(long long)k * a.T + t] : 0.0;
      double sn, cs;
      sincospi(2.0 * (double)((k * n) & (N - 1)) / (double)N, &sn, &cs);
      if (k == 0 || k == N / 2) s += g * (double)z.x * cs;  // imaginary parts ignored
      else s += 2.0 * g * ((double)z.x * cs - (double)z.y * sn);
    }
    acc += s * w;
    nrm += w * w;
  }
  return (float)(acc * a.cd / nrm);
}

__global__ __launch_bounds__(CT) void istft_kernel(InvArgs a) {
  extern __shared__ float2 sm[];
  const int N = a.N, P = a.P, TF = a.TF, F = N / 2 + 1, tid = threadIdx.x, hop = a.hop;
  float2* bufA = sm;
  float2* bufB = sm + P * N;
  float2* tile = sm + 2 * P * N;  // [F][TF + 1]
  float* sW = reinterpret_cast<float*>(tile + F * (TF + 1));
  const long long b = blockIdx.y, o0 = (long long)blockIdx.x * SPAN;
  const long long olast = (o0 + SPAN < a.n_out ? o0 + SPAN : a.n_out) - 1;
  const long long e0 = o0 + a.trim, e1 = olast + a.trim;  // span in overlap-add coordinates
  // frames that touch the span: ceil((e0 - N + 1) / hop) .. floor(e1 / hop), clipped
  const int tlo = e0 >= N ? (int)((e0 - N + hop) / hop) : 0;
  const long long th = e1 / hop;
  const int thi = th < a.T - 1 ? (int)th : a.T - 1;
  const int tlo_pair = tlo & ~1;  // the pair partner is loaded too: same bits as the neighbour
  for (int n = tid; n < N; n += CT) sW[n] = a.win[n];
  float acc[SPT], nrm[SPT];
  int lo[SPT], hi[SPT];
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const long long e = e0 + tid + CT * i;
    acc[i] = 0.f;
    nrm[i] = 0.f;
    lo[i] = e >= N ? (int)((e - N + hop) / hop) : 0;
    const long long h = e / hop;
    hi[i] = h < a.T - 1 ? (int)h : a.T - 1;
  }
  const float2* Zb = a.Z + b * F * (long long)a.T;
  const float* gb = a.gain ? a.gain + b * a.gain_rows * (long long)a.T : nullptr;
  const int rounds = TF / (2 * P);
  for (int tt = (tlo / TF) * TF; tt <= thi; tt += TF) {
    __syncthreads();  // the previous tile's readers are done (and sW is written)
    for (int idx = tid; idx < F * TF; idx += CT) {
      const int tl = idx & (TF - 1), k = idx >> a.log2tf;
      const int t = tt + tl;
      float2 v = make_float2(0.f, 0.f);
      if (t < a.T && t >= tlo_pair) {
        v = Zb[(long long)k * a.T + t];
        if (gb) {
          const float g = k < a.gain_rows ? gb[(long long)k * a.T + t] : 0.f;
          v.x *= g;
          v.y *= g;
        }
      }
      if (k == 0 || k == N / 2) v.y = 0.f;  // c2r ignores these imaginary parts
      tile[k * (TF + 1) + tl] = v;
    }
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
      const int tr = tt + r * 2 * P;  // first frame of the round
      if (tr > thi || tr + 2 * P <= tlo_pair) continue;  // uniform
      for (int idx = tid; idx < P * N; idx += CT) {
        const int p = idx >> a.log2n, n = idx & (N - 1);
        const int k = n <= N / 2 ? n : N - n;
        const float2* s = tile + k * (TF + 1) + r * 2 * P + 2 * p;
        const float2 A = s[0], B = s[1];
        bufA[idx] = n <= N / 2 ? make_float2(A.x - B.y, -(A.y + B.x))
                               : make_float2(A.x + B.y, A.y - B.x);
      }
      __syncthreads();
      const float2* res = stockham<CT>(bufA, bufB, N, a.log2n, P, a.tw, N, tid);
      // res[p N + n] = N (a_n - i b_n) of the frames tr + 2p (a) and tr + 2p + 1 (b)
#pragma unroll
      for (int i = 0; i < SPT; ++i) {
        const long long e = e0 + tid + CT * i;
        const int f0 = lo[i] > tr ? lo[i] : tr;
        const int f1 = hi[i] < tr + 2 * P - 1 ? hi[i] : tr + 2 * P - 1;
        for (int t = f0; t <= f1; ++t) {
          const int n = (int)(e - (long long)t * hop), f = t - tr;
          const float2 v = res[(f >> 1) * N + n];
          const float w = sW[n];
          acc[i] = fmaf((f & 1) ? -v.y : v.x, w, acc[i]);
          nrm[i] = fmaf(w, w, nrm[i]);
        }
      }
      __syncthreads();
    }
  }
  float* ob = a.out + b * a.os;
  unsigned edge = 0;  // samples left to edge_sample
#pragma unroll
  for (int i = 0; i < SPT; ++i) {
    const long long o = o0 + tid + CT * i;
    if (o >= a.n_out) continue;
    if (nrm[i] > 1e-10f && nrm[i] < EDGE_NRM) edge |= 1u << i;
    else ob[o] = acc[i] * a.c / (nrm[i] > 1e-10f ? nrm[i] : 1.f);
  }
  while (edge) {  // after the register arrays are dead: rare, and heavy in fp64
    const int i = __ffs(edge) - 1;
    edge &= edge - 1;
    const long long e = e0 + tid + CT * i;
    const int l = e >= N ? (int)((e - N + hop) / hop) : 0;
    const long long h = e / hop;
    ob[o0 + tid + CT * i] = edge_sample(a, Zb, gb, e, l, h < a.T - 1 ? (int)h : a.T - 1);
  }
}

// dynamic LDS above 64 KiB needs the attribute on both kernels
LdsOptIn g_lds;
hipError_t allow_tile_lds() {
  return allow_lds(g_lds, {(const void*)stft_complex_kernel, (const void*)istft_kernel}, MAX_LDS);
}

}  // namespace
}  // namespace specenh

extern "C" {

long long specenh_stft_complex_frames(long long length, int nperseg, int noverlap, int boundary,
                                      int padded) {
  using specenh::set_error;
  if (nperseg <= 0 || noverlap < 0 || noverlap >= nperseg)
    return set_error(SPECENH_EINVAL, "noverlap must be less than nperseg.");
  if (boundary != SPECENH_BOUNDARY_NONE && boundary != SPECENH_BOUNDARY_ZEROS)
    return set_error(SPECENH_EUNSUPPORTED, "boundary must be None or 'zeros' on the GPU path");
  if (length < nperseg) return set_error(SPECENH_EINVAL, "signal shorter than nperseg");
  const long long hop = nperseg - noverlap;
  const long long ext = length + (boundary == SPECENH_BOUNDARY_ZEROS ? 2 * (nperseg / 2) : 0);
  long long nadd = 0;
  if (padded) nadd = ((hop - (ext - nperseg) % hop) % hop) % nperseg;
  return (ext + nadd - nperseg) / hop + 1;
}

long long specenh_istft_length(long long frames, int nperseg, int noverlap, int boundary) {
  using specenh::set_error;
  if (nperseg <= 0 || noverlap < 0 || noverlap >= nperseg)
    return set_error(SPECENH_EINVAL, "noverlap must be less than nperseg.");
  if (frames < 1) return set_error(SPECENH_EINVAL, "at least one frame is needed");
  const long long hop = nperseg - noverlap;
  return hop * (frames - 1) + nperseg - (boundary ? 2 * (nperseg / 2) : 0);
}

int specenh_stft_complex(const specenh_stft_plan* plan, const float* x, long long batch,
                         long long length, long long x_stride, void* out, int boundary, int padded,
                         void* stream) {
  using namespace specenh;
  if (!plan) return set_error(SPECENH_EINVAL, "null plan");
  if (batch < 0) return set_error(SPECENH_EINVAL, "batch must be >= 0");
  const int N = plan->nperseg;
  const long long T = specenh_stft_complex_frames(length, N, plan->noverlap, boundary, padded);
  if (T < 0) return (int)T;
  if (batch == 0) return SPECENH_OK;
  if (!x || !out) return set_error(SPECENH_EINVAL, "null x/out");
  if (x_stride < length) return set_error(SPECENH_EINVAL, "x_stride < length");
  const Cfg c = cfg_for(N);
  const long long tiles = (T + c.TF - 1) / c.TF;
  if (tiles > 2147483647LL) return set_error(SPECENH_EUNSUPPORTED, "too many frames");
  hipError_t e = allow_tile_lds();
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("stft_complex: ") + hipGetErrorString(e));
  FwdArgs a{};
  a.xs = x_stride; a.L = length; a.T = T;
  a.N = N; a.log2n = ilog2i(N); a.hop = plan->hop;
  a.pad = boundary == SPECENH_BOUNDARY_ZEROS ? N / 2 : 0;
  a.P = c.P; a.TF = c.TF; a.log2tf = ilog2i(c.TF); a.detrend = plan->detrend;
  a.rs = (float)(0.5 * std::sqrt(plan->scale));
  a.win = plan->d_window; a.tw = plan->d_tw_nat;
  const size_t lds = fft_tile_bytes(N, c);
  const long long F = N / 2 + 1;
  for (long long b0 = 0; b0 < batch; b0 += 65535) {  // grid.y limit
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    a.x = x + b0 * x_stride;
    a.out = reinterpret_cast<float2*>(out) + b0 * F * T;
    SPECENH_LAUNCH(stft_complex_kernel, dim3((unsigned)tiles, (unsigned)nb), dim3(CT), lds,
                   (hipStream_t)stream, a);
    e = hipGetLastError();
    if (e != hipSuccess)
      return set_error(SPECENH_EHIP, std::string("stft_complex launch: ") + hipGetErrorString(e));
  }
  return SPECENH_OK;
}

int specenh_istft(const specenh_stft_plan* plan, const void* Z, const float* gain, int gain_rows,
                  long long batch, long long frames, float* out, long long out_stride, int boundary,
                  void* stream) {
  using namespace specenh;
  if (!plan) return set_error(SPECENH_EINVAL, "null plan");
  if (batch < 0) return set_error(SPECENH_EINVAL, "batch must be >= 0");
  const int N = plan->nperseg, F = N / 2 + 1;
  const long long n_out = specenh_istft_length(frames, N, plan->noverlap, boundary);
  if (n_out < 0) return (int)n_out;
  if (gain ? (gain_rows != F && gain_rows != F - 1) : gain_rows != 0)
    return set_error(SPECENH_EINVAL, "gain must have F or F - 1 rows (0 without a gain)");
  if (batch == 0 || n_out == 0) return SPECENH_OK;
  if (!Z || !out) return set_error(SPECENH_EINVAL, "null Z/out");
  if (out_stride < n_out) return set_error(SPECENH_EINVAL, "out_stride < output length");
  const long long spans = (n_out + SPAN - 1) / SPAN;
  if (frames > 2147483647LL - 64 || spans > 2147483647LL)
    return set_error(SPECENH_EUNSUPPORTED, "too many frames");
  hipError_t e = allow_tile_lds();
  if (e != hipSuccess) return set_error(SPECENH_EHIP, std::string("istft: ") + hipGetErrorString(e));
  const Cfg c = cfg_for(N);
  InvArgs a{};
  a.gain_rows = gain_rows; a.T = (int)frames; a.os = out_stride; a.n_out = n_out;
  a.N = N; a.log2n = ilog2i(N); a.hop = plan->hop; a.trim = boundary ? N / 2 : 0;
  a.P = c.P; a.TF = c.TF; a.log2tf = ilog2i(c.TF);
  const double s = plan->scaling == SPECENH_SCALING_SPECTRUM ? plan->win_sum
                                                             : std::sqrt(plan->fs * plan->win_sumsq);
  a.c = (float)(s / N);
  a.cd = s / N;
  a.win = plan->d_window; a.tw = plan->d_tw_nat;
  const size_t lds = fft_tile_bytes(N, c) + (size_t)N * sizeof(float);
  for (long long b0 = 0; b0 < batch; b0 += 65535) {  // grid.y limit
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    a.Z = reinterpret_cast<const float2*>(Z) + b0 * F * frames;
    a.gain = gain ? gain + b0 * gain_rows * frames : nullptr;
    a.out = out + b0 * out_stride;
    SPECENH_LAUNCH(istft_kernel, dim3((unsigned)spans, (unsigned)nb), dim3(CT), lds,
                   (hipStream_t)stream, a);
    e = hipGetLastError();
    if (e != hipSuccess)
      return set_error(SPECENH_EHIP, std::string("istft launch: ") + hipGetErrorString(e));
  }
  return SPECENH_OK;
}

}  // extern "C"
