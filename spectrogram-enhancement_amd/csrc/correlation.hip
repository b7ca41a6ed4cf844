// correlation.hip — block-averaged linear cross-correlation of signal pairs for gfx950
// (include/specenh_correlation.h): per averaging group the mean over its frames of
//   r_t[m] = sum_n x_t[n] y_t[n + m],  m = -M .. M,
// x_t, y_t the detrended, windowed frames of spectral_mean.hip, and the mean frame energies
// sum_n x_t[n]^2, sum_n y_t[n]^2 that normalise it to a coefficient
// (scipy.signal.correlate(y_t, x_t, 'full')[N - 1 + m], averaged).
//
// The correlation is linear, so the cross-spectra of a group's frames are summed first and
// inverted once. A frame of N reals, zero-padded to 2N, is read as N complex numbers
// z_j = v_2j + i v_2j+1 (the upper half zero), transformed by an N-point Stockham FFT (the LDS
// passes of fft_lds.hpp with the plan's natural-order twiddles) and unpacked to the N + 1 bins
// of the 2N-point real transform with the plan's W_2N table (d_tw_pad). No per-frame spectrum
// goes to memory.
//
// correlation_chunk_kernel: a workgroup owns one shot and one chunk, a run of at most
//   SPECENH_SPECTRAL_CHUNK consecutive frames of one group. Round by round it loads FR frames
//   of x (and of y) into LDS, detrends and windows them (load_frames), takes their energies in
//   the time domain (fp64, wave_sum), pads, transforms them side by side and adds
//   conj(X) Y per bin to fp32 registers. Slot p accumulates frames p, p + FR, ... in ascending
//   order; the slots are then added in ascending p. A group that is one chunk is inverted and
//   stored by the same workgroup; otherwise the chunk's record (N + 1 float2 bins, two fp64
//   energies) goes to the workspace.
// correlation_fold_kernel: a workgroup per (shot, group) adds the chunk records in fp64 in
//   ascending chunk order and inverts.
//
// The inverse: C_k, k = 0 .. N, Hermitian, is packed to
//   Z_k = (C_k + conj C_{N-k}) + i conj(W_2N^k) (C_k - conj C_{N-k}),   k = 0 .. N-1,
// conj(Z) goes through the same forward transform, and r[2j] = Re F_j, r[2j+1] = -Im F_j, times
// 1 / (8 N) (the bins are those of 2X and 2Y, Z is twice the packed spectrum). Lag m < 0 is
// r[2N + m]. No atomics; an element depends on its own pair's samples, the plan, navg, maxlag
// and mode only.
//
// LDS: two buffers of slots * N float2 (32 KiB; 64 KiB at N = 2048, opted in through
// allow_lds beside 0.5 KiB static); the fold kernel (2 N + 1) float2.
#include <hip/hip_runtime.h>

#include <string>

#include "specenh_correlation.h"
#include "runtime.hpp"
#include "averaging.hpp"
#include "fft_lds.hpp"

namespace specenh {
namespace {

constexpr int CT = 256;  // threads per workgroup
constexpr int CHUNK = SPECENH_SPECTRAL_CHUNK;
constexpr int MAX_LDS = 64 * 1024;
constexpr int MAX_N = 2048;  // the padded transform is at most the 4096 points of the LDS FFT

using namespace fft_lds;  // load_frames, stockham, unpack2, nyquist2, c_mul

struct Args {
  const float* x;
  const float* y;
  long long xs, ys;  // row strides
  int N, log2n, hop, slots, detrend;
  int glen;  // frames per group
  int ncg;   // chunks per group
  int G;     // groups
  int M;     // maximum lag
  int mode;
  float* out;       // [batch][G][2 M + 1]
  float* energies;  // [batch][G][2] or null
  float2* ws;       // [batch][G][ncg] records of N + 3 float2; used when ncg > 1
  const float* win;
  const float2* tw;   // W_N^n
  const float2* tw2;  // W_2N^n
};

// The lags of one group from its summed cross-spectrum cb[0 .. N] (of 2X and 2Y) and its
// summed frame energies; zb and cb are the transform's two buffers (zb: N, cb: N + 1 float2).
// The only place outputs are stored. Every thread of the workgroup calls it.
__device__ __forceinline__ void invert_store(const Args& a, float2* zb, float2* cb, double ex,
                                             double ey, long long bg, int tid) {
  const int N = a.N, M = a.M;
  for (int k = tid; k < N; k += CT) {
    const float2 c = cb[k], m = cb[N - k], w = a.tw2[k];
    const float2 s = make_float2(c.x + m.x, c.y - m.y);  // C_k + conj C_{N-k}
    const float2 d = make_float2(c.x - m.x, c.y + m.y);  // C_k - conj C_{N-k}
    const float2 p = c_mul(d, make_float2(w.x, -w.y));
    zb[k] = make_float2(s.x - p.y, -(s.y + p.x));  // conj(s + i p)
  }
  __syncthreads();
  const float2* res = stockham<CT>(zb, cb, N, a.log2n, 1, a.tw, N, tid);
  double sc = 1.0 / (8.0 * N);
  if (a.mode == SPECENH_CORR_COEFF) sc = (ex > 0.0 && ey > 0.0) ? sc / (sqrt(ex) * sqrt(ey)) : 0.0;
  else sc /= (double)a.glen;
  float* out = a.out + bg * (2 * M + 1);
  for (int i = tid; i < 2 * M + 1; i += CT) {
    const int n = i < M ? 2 * N + i - M : i - M;  // lag i - M
    const float2 f = res[n >> 1];
    out[i] = (float)(((n & 1) ? -f.y : f.x) * sc);
  }
  if (a.energies && tid < 2) a.energies[bg * 2 + tid] = (float)((tid ? ey : ex) / (double)a.glen);
}

// NI = FR * N / CT bins per thread, FR = frames per round (slots, or slots / 2 with y).
template <int NI, bool PAIR>
__global__ __launch_bounds__(CT) void correlation_chunk_kernel(Args a) {
  extern __shared__ float2 sm[];
  __shared__ float stat[32][2];  // per slot: mean, slope
  __shared__ double esum[32];    // per slot: the energies of its frames so far
  constexpr int NA = PAIR ? 2 : 1;
  const int N = a.N, H = N / 2, F = N + 1, log2n = a.log2n, tid = threadIdx.x;
  const int S = a.slots, FR = PAIR ? S / 2 : S;
  float2* bufA = sm;
  float2* bufB = sm + S * N;
  float* raw = reinterpret_cast<float*>(bufB);  // slot s: samples [s * N, (s + 1) * N)
  const long long b = blockIdx.y;
  const int g = blockIdx.x / a.ncg, c = blockIdx.x - g * a.ncg;
  const long long f0 = (long long)g * a.glen + (long long)c * CHUNK;  // first frame
  const int left = a.glen - c * CHUNK;
  const int cnt = left < CHUNK ? left : CHUNK;  // >= 1
  const float* xb = a.x + b * a.xs;
  const float* yb = PAIR ? a.y + b * a.ys : nullptr;
  if (tid < 32) esum[tid] = 0.0;  // load_frames' barriers come before the first use
  // bins 0 .. N-1 of this thread's slots; bin N (real) of all of them (k = 0 threads only)
  float acc[NI][NA], accn = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < NA; ++j) acc[i][j] = 0.f;
  for (int r0 = 0; r0 < cnt; r0 += FR) {
    load_frames<CT>(raw, stat, N, log2n, S, a.detrend, a.win, tid, [&](int s, int n) {
      const int p = PAIR ? s & (FR - 1) : s;
      const float* src = (PAIR && s >= FR) ? yb : xb;
      // slots past the chunk's end stay zero and add nothing
      return r0 + p < cnt ? src[(f0 + r0 + p) * a.hop + n] : 0.f;
    });
    for (int s = tid >> 6; s < S; s += CT / 64) {  // a slot belongs to one wave, round after round
      double e = 0.0;
      for (int n = tid & 63; n < N; n += 64) {
        const double v = raw[s * N + n];
        e = fma(v, v, e);
      }
      e = wave_sum(e);
      if ((tid & 63) == 0) esum[s] += e;
    }
    for (int idx = tid; idx < S * N; idx += CT) {  // z_j = v_2j + i v_2j+1, the upper half zero
      const int s = idx >> log2n, j = idx & (N - 1);
      bufA[idx] = j < H ? reinterpret_cast<const float2*>(raw)[s * H + j] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    const float2* res = stockham<CT>(bufA, bufB, N, log2n, S, a.tw, N, tid);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int idx = tid + CT * i, p = idx >> log2n, k = idx & (N - 1);
      const float2 w = a.tw2[k];
      const float2* zx = res + p * N;
      const float2 X = unpack2(zx, k, N, w);
      if constexpr (PAIR) {
        const float2* zy = res + (FR + p) * N;
        const float2 Y = unpack2(zy, k, N, w);
        acc[i][0] += fmaf(X.x, Y.x, X.y * Y.y);  // conj(X) Y
        acc[i][1] += fmaf(X.x, Y.y, -X.y * Y.x);
        if (k == 0) accn = fmaf(nyquist2(zx), nyquist2(zy), accn);
      } else {
        acc[i][0] = fmaf(X.x, X.x, fmaf(X.y, X.y, acc[i][0]));
        if (k == 0) {
          const float xn = nyquist2(zx);
          accn = fmaf(xn, xn, accn);
        }
      }
    }
    __syncthreads();  // the next round's loads overwrite the buffers
  }
  float* red = reinterpret_cast<float*>(sm);  // [FR][F][NA] <= bufA
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int idx = tid + CT * i, p = idx >> log2n, k = idx & (N - 1);
#pragma unroll
    for (int j = 0; j < NA; ++j) red[(p * F + k) * NA + j] = acc[i][j];
    // a k = 0 thread folds bin N of all its slots into one accn: stored once
    if (k == 0) {
      red[(p * F + N) * NA] = i == 0 ? accn : 0.f;
      if constexpr (PAIR) red[(p * F + N) * NA + 1] = 0.f;
    }
  }
  __syncthreads();
  const long long bg = b * a.G + g;
  float2* rec = a.ws + (bg * a.ncg + c) * (N + 3);
  for (int k = tid; k < F; k += CT) {
    float s[2] = {0.f, 0.f};
    for (int p = 0; p < FR; ++p)
#pragma unroll
      for (int j = 0; j < NA; ++j) s[j] += red[(p * F + k) * NA + j];
    const float2 v = make_float2(s[0], s[1]);
    if (a.ncg > 1) rec[k] = v;  // uniform
    else bufB[k] = v;
  }
  double ex = 0.0, ey = 0.0;
  for (int p = 0; p < FR; ++p) {
    ex += esum[p];
    if constexpr (PAIR) ey += esum[FR + p];
  }
  if constexpr (!PAIR) ey = ex;
  if (a.ncg > 1) {
    if (tid < 2) reinterpret_cast<double*>(rec + F)[tid] = tid ? ey : ex;
    return;
  }
  __syncthreads();  // red is read, the bins are in bufB
  invert_store(a, bufA, bufB, ex, ey, bg, tid);
}

// grid (G, nb): the chunk records of one group in fp64, ascending, then the inverse
__global__ __launch_bounds__(CT) void correlation_fold_kernel(Args a) {
  extern __shared__ float2 sm[];  // zb [N], cb [N + 1]
  const int N = a.N, F = N + 1, tid = threadIdx.x;
  float2* zb = sm;
  float2* cb = sm + N;
  const long long bg = (long long)blockIdx.y * a.G + blockIdx.x;
  const float2* rec = a.ws + bg * a.ncg * (N + 3);
  for (int k = tid; k < F; k += CT) {
    double re = 0.0, im = 0.0;
    for (int c = 0; c < a.ncg; ++c) {
      const float2 v = rec[(long long)c * (N + 3) + k];
      re += v.x;
      im += v.y;
    }
    cb[k] = make_float2((float)re, (float)im);
  }
  double ex = 0.0, ey = 0.0;
  for (int c = 0; c < a.ncg; ++c) {
    const double* e = reinterpret_cast<const double*>(rec + (long long)c * (N + 3) + F);
    ex += e[0];
    ey += e[1];
  }
  __syncthreads();
  invert_store(a, zb, cb, ex, ey, bg, tid);
}

using ChunkKernel = void (*)(Args);
// NI = FR N / CT
ChunkKernel chunk_kernel(int N, bool pair) {
  if (pair) return N <= 1024 ? correlation_chunk_kernel<4, true> : correlation_chunk_kernel<8, true>;
  return N <= 1024 ? correlation_chunk_kernel<8, false> : correlation_chunk_kernel<16, false>;
}

// N = 2048 takes 64 KiB of dynamic LDS next to the static stat[] and esum[]
LdsOptIn g_lds;

// plan, batch, nperseg, the frame split and maxlag of a call; SPECENH_OK or a negative error
int check_lags(const specenh_stft_plan* plan, long long batch, long long length, long long navg,
               long long maxlag, FrameSplit* s) {
  const int N = plan ? plan->nperseg : 64;  // its own nperseg range, ahead of frame_split's
  if (N == 4096)
    return set_error(SPECENH_EUNSUPPORTED,
                     "correlation: nperseg = 4096 is not supported (the padded transform would "
                     "be 8192 points); nperseg must be a power of two in [64, 2048]");
  if (N < 64 || N > MAX_N || (N & (N - 1)))
    return set_error(SPECENH_EUNSUPPORTED,
                     "correlation: nperseg must be a power of two in [64, 2048]");
  if (int rc = check_call(plan, batch, length, navg, true, s)) return rc;
  if (maxlag < 0 || maxlag >= N)
    return set_error(SPECENH_EINVAL, "maxlag must be in [0, nperseg - 1]");
  return SPECENH_OK;
}

size_t record_bytes(int N) { return (size_t)(N + 3) * sizeof(float2); }

}  // namespace
}  // namespace specenh

extern "C" {

size_t specenh_correlation_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                           long long length, long long navg, long long maxlag) {
  using namespace specenh;
  FrameSplit s;
  if (check_lags(plan, batch, length, navg, maxlag, &s) != SPECENH_OK || s.ncg == 1) return 0;
  return (size_t)batch * s.G * s.ncg * record_bytes(plan->nperseg);
}

int specenh_correlation(const specenh_stft_plan* plan, const float* x, const float* y,
                        long long batch, long long length, long long x_stride,
                        long long y_stride, long long navg, long long maxlag, int mode,
                        float* out, float* energies, void* workspace, size_t workspace_bytes,
                        void* stream) {
  using namespace specenh;
  if (!x) return set_error(SPECENH_EINVAL, "null x");
  if (!y) return set_error(SPECENH_EINVAL, "null y");
  FrameSplit s;
  if (int rc = check_lags(plan, batch, length, navg, maxlag, &s)) return rc;
  const SignalArg in[] = {{x, x_stride, "x_stride < length"}, {y, y_stride, "y_stride < length"}};
  if (int rc = check_strides(in, 2, length)) return rc;
  if (mode != SPECENH_CORR_RAW && mode != SPECENH_CORR_COEFF)
    return set_error(SPECENH_EINVAL, "mode must be SPECENH_CORR_RAW or SPECENH_CORR_COEFF");
  if (!out) return set_error(SPECENH_EINVAL, "null out");
  if (batch == 0) return SPECENH_OK;
  const int N = plan->nperseg;
  if (s.G * s.ncg > 2147483647LL) return set_error(SPECENH_EUNSUPPORTED, "too many chunks");
  if (s.ncg > 1)
    if (int rc = check_workspace(workspace, workspace_bytes,
                                 (size_t)batch * s.G * s.ncg * record_bytes(N)))
      return rc;
  FrameSignals sig{};
  int which[2];
  const bool pair = collect_signals(in, 2, &sig, which) == 2;  // y given as x: loaded once
  hipError_t e = allow_lds(g_lds,
                           {(const void*)chunk_kernel(1024, false), (const void*)chunk_kernel(1024, true),
                            (const void*)chunk_kernel(2048, false), (const void*)chunk_kernel(2048, true)},
                           MAX_LDS);
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("correlation: ") + hipGetErrorString(e));
  Args a{};
  a.xs = x_stride; a.ys = y_stride;
  a.N = N; a.log2n = ilog2i(N); a.hop = plan->hop; a.slots = slots_for(N);
  a.detrend = plan->detrend;
  a.glen = (int)s.glen; a.ncg = (int)s.ncg; a.G = (int)s.G;
  a.M = (int)maxlag; a.mode = mode;
  a.win = plan->d_window; a.tw = plan->d_tw_nat; a.tw2 = plan->d_tw_pad;
  const size_t lds = (size_t)2 * a.slots * N * sizeof(float2);
  const ChunkKernel kern = chunk_kernel(N, pair);
  for (long long b0 = 0; b0 < batch; b0 += 65535) {  // grid.y limit
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    a.x = x + b0 * x_stride;
    a.y = pair ? y + b0 * y_stride : nullptr;
    a.out = out + b0 * s.G * (2 * maxlag + 1);
    a.energies = energies ? energies + b0 * s.G * 2 : nullptr;
    a.ws = s.ncg > 1 ? reinterpret_cast<float2*>(workspace) + b0 * s.G * s.ncg * (N + 3) : nullptr;
    launch(kern, dim3((unsigned)(s.G * s.ncg), (unsigned)nb), dim3(CT), lds, stream, a);
    if (int rc = launched("correlation_chunk")) return rc;
    if (s.ncg == 1) continue;
    SPECENH_LAUNCH(correlation_fold_kernel, dim3((unsigned)s.G, (unsigned)nb), dim3(CT),
                   (size_t)(2 * N + 1) * sizeof(float2), (hipStream_t)stream, a);
    if (int rc = launched("correlation_fold")) return rc;
  }
  return SPECENH_OK;
}

}  // extern "C"
