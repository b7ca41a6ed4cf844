// wavenumber.hip — the two-point wavenumber-frequency spectrum S(k, f) for gfx950 (Beall, Kim &
// Powers 1982; include/specenh_wavenumber.h): per averaging group and bin f, the histogram of
// the per-frame cross-phase theta = arg(conj(X_t[f]) Y_t[f]) over K centred bins, each frame
// weighted by its power o[f] (|X_t[f]|^2 + |Y_t[f]|^2) / 2. Two kernels on one stream:
//
// the transform of bispectrum.hip (transform_frames(), averaging.hpp): every frame of x and y
//   that enters a group, detrended, windowed and transformed once into the workspace as
//   float2 [shot][signal][frame][F] holding 2 X / sqrt(scale);
//
// wavenumber_accumulate_kernel: a one-wave workgroup owns one (shot, group, 64 consecutive
//   bins f), lane = bin, so a frame is two coalesced 512-byte row reads (loaded FS frames
//   ahead of their use). Lane l keeps its K accumulators in LDS as fp64 at H[j * 64 + l] and
//   walks the group's frames in ascending order with a plain read-add-write: the cell is
//   private to the lane, so there is no atomic, and whatever j each lane picks the 64 lanes
//   touch 64 consecutive doubles of row j_l — one double per lane and bank pair, two full
//   rows of the 64 x 4 B banks, no conflict. The sums are fp64 from the first frame, so there
//   is no chunk to fold. The epilogue scales in fp64 (scale, o[f], 1 / frames), rounds once to
//   fp32 and writes every element of [F][K], zeros included: JB bins j at a time through a
//   padded LDS tile, so a store instruction covers whole 128-byte lines.
//
// Bitwise structure. A lane's chain depends on its own bin's samples, K and the group length
// only; the tile grid is anchored at bin 0. An element therefore does not depend on the
// batch, on the shot's position or on strides. LDS: K * 512 B dynamic (32 KiB at K = 64,
// 128 KiB at K = 256, opted in through allow_lds) + 8.25 KiB static for the store tile.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "specenh_wavenumber.h"
#include "runtime.hpp"
#include "averaging.hpp"

namespace specenh {
namespace {

constexpr int WL = 64;   // lanes of the workgroup = bins f it owns
constexpr int FS = 8;    // frames in flight ahead of their use
constexpr int JB = 32;   // bins j the epilogue stores at once: 128 bytes a bin f
constexpr int MIN_K = 4, MAX_K = 256;
constexpr int MAX_LDS = MAX_K * WL * (int)sizeof(double);

struct AccumulateArgs {
  const float2* X;  // frame t of shot b at X + b * bs + t * F, likewise Y
  const float2* Y;
  long long bs;
  float* S;         // [nb][G][F][K]
  int F, K, G, glen;
  int nt;           // tiles along f: ceil(F / WL)
  int onesided;     // o[f] = 2 for 0 < f < F - 1
  float kscale;     // K / (2 pi)
  double scale;     // of the sum of |X|^2 + |Y|^2, before o[f] and the division by glen
};

// grid (G * nt, nb): the tiles of one group run side by side
__global__ __launch_bounds__(WL) void wavenumber_accumulate_kernel(AccumulateArgs a) {
  extern __shared__ double H[];            // [K][WL]
  __shared__ float st[WL * (JB + 1)];      // the epilogue's [f][j] tile, rows padded by one
  const int lane = threadIdx.x;
  const int g = blockIdx.x / a.nt, tile = blockIdx.x - g * a.nt;
  const long long b = blockIdx.y;
  const int F = a.F, K = a.K, half = K >> 1;
  const int f = tile * WL + lane;
  const bool ok = f < F;  // lanes past the spectrum add zeros to their own cells, never read a row
  for (int j = 0; j < K; ++j) H[j * WL + lane] = 0.0;
  const long long first = b * a.bs + (long long)g * a.glen * F + (ok ? f : 0);
  const float2* sx = a.X + first;
  const float2* sy = a.Y + first;
  float2 vx[FS], vy[FS];  // this lane's bin of the frames of a step, in flight a step ahead
  auto fetch = [&](int f0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < FS; ++q) {
      vx[q] = vy[q] = make_float2(0.f, 0.f);
      if (ok && f0 + q < a.glen) {
        vx[q] = sx[(long long)(f0 + q) * F];
        vy[q] = sy[(long long)(f0 + q) * F];
      }
    }
  };
  fetch(0);
  for (int f0 = 0; f0 < a.glen; f0 += FS) {
    float2 cx[FS], cy[FS];
#pragma unroll
    for (int q = 0; q < FS; ++q) {
      cx[q] = vx[q];
      cy[q] = vy[q];
    }
    if (f0 + FS < a.glen) fetch(f0 + FS);  // the next step's loads run under this step's sums
    const int nf = a.glen - f0 < FS ? a.glen - f0 : FS;
#pragma unroll
    for (int q = 0; q < FS; ++q) {
      if (q >= nf) break;
      const float2 x = cx[q], y = cy[q];
      const float re = fmaf(x.x, y.x, x.y * y.y);   // conj(X) Y
      const float im = fmaf(x.x, y.y, -(x.y * y.x));
      const float theta = (re == 0.f && im == 0.f) ? 0.f : atan2f(im, re);
      int j = (int)rintf(theta * a.kscale) + half;  // 0 .. K, K wraps onto 0: +pi and -pi
      if (j >= K) j -= K;
      j = j < 0 ? 0 : (j >= K ? K - 1 : j);  // NaN or Inf samples: still this lane's own cell
      const float w = fmaf(x.x, x.x, fmaf(x.y, x.y, fmaf(y.x, y.x, y.y * y.y)));
      H[j * WL + lane] += (double)w;
    }
  }
  // scale and o[f] = 2 for 0 < f < F - 1 (a power of two: the product rounds as the factors)
  const double so = (a.onesided && f > 0 && f < F - 1) ? 2.0 * a.scale : a.scale;
  const double glen = (double)a.glen;
  const int rows = F - tile * WL < WL ? F - tile * WL : WL;  // bins f of this tile
  float* out = a.S + (((b * a.G + g) * F) + (long long)tile * WL) * K;
  const int jj = lane % JB;
  for (int j0 = 0; j0 < K; j0 += JB) {
    const int nj = K - j0 < JB ? K - j0 : JB;
    __syncthreads();  // the reads of the block before are done
    for (int c = 0; c < nj; ++c)
      st[lane * (JB + 1) + c] = (float)(H[(j0 + c) * WL + lane] * so / glen);
    __syncthreads();
    if (jj < nj)  // WL / JB bins f an instruction, JB consecutive floats of each
      for (int r = lane / JB; r < rows; r += WL / JB)
        out[(long long)r * K + j0 + jj] = st[r * (JB + 1) + jj];
  }
}

LdsOptIn g_lds;  // K > 128 takes more than 64 KiB of dynamic LDS

int check_nk(long long nk) {
  if (nk < MIN_K || nk > MAX_K || (nk & 1))
    return set_error(SPECENH_EINVAL, "nk must be even and in [4, 256]");
  return SPECENH_OK;
}

// the accumulate launches of a call: shots [0, batch) in steps of grid.y
int accumulate(AccumulateArgs g, long long batch, float* skf, void* stream) {
  const long long per_shot = (long long)g.G * g.nt;
  if (per_shot > 2147483647LL) return set_error(SPECENH_EUNSUPPORTED, "too many groups");
  hipError_t e = allow_lds(g_lds, {(const void*)wavenumber_accumulate_kernel}, MAX_LDS);
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("wavenumber: ") + hipGetErrorString(e));
  g.kscale = (float)(g.K / (2.0 * M_PI));
  const size_t lds = (size_t)g.K * WL * sizeof(double);
  const long long out_shot = (long long)g.G * g.F * g.K;
  const float2 *X = g.X, *Y = g.Y;
  for (long long b0 = 0; b0 < batch; b0 += 65535) {
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    g.X = X + b0 * g.bs;
    g.Y = Y + b0 * g.bs;
    g.S = skf + b0 * out_shot;
    SPECENH_LAUNCH(wavenumber_accumulate_kernel, dim3((unsigned)per_shot, (unsigned)nb), dim3(WL),
                   lds, (hipStream_t)stream, g);
    if (int rc = launched("wavenumber_accumulate")) return rc;
  }
  return SPECENH_OK;
}

}  // namespace
}  // namespace specenh

extern "C" {

size_t specenh_wavenumber_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                          long long nsignals, long long length,
                                          long long navg) {
  using namespace specenh;
  FrameSplit s;
  if (check_call(plan, batch, length, navg, true, &s) != SPECENH_OK) return 0;
  if (nsignals < 1 || nsignals > 2) {
    set_error(SPECENH_EINVAL, "nsignals must be in [1, 2]");
    return 0;
  }
  return frames_workspace_bytes(plan, batch, nsignals, s.Tu);
}

int specenh_wavenumber_spectrum(const specenh_stft_plan* plan, const float* x, const float* y,
                                long long batch, long long length, long long x_stride,
                                long long y_stride, long long navg, long long nk, float* skf,
                                void* workspace, size_t workspace_bytes, void* stream) {
  using namespace specenh;
  if (!x) return set_error(SPECENH_EINVAL, "null x");
  if (!y) return set_error(SPECENH_EINVAL, "null y");
  FrameSplit s;
  if (int rc = check_call(plan, batch, length, navg, true, &s)) return rc;
  const SignalArg in[] = {{x, x_stride, "x_stride < length"}, {y, y_stride, "y_stride < length"}};
  if (int rc = check_strides(in, 2, length)) return rc;
  if (int rc = check_nk(nk)) return rc;
  if (!skf) return set_error(SPECENH_EINVAL, "null skf");
  if (batch == 0) return SPECENH_OK;
  FrameSignals sig{};
  int which[2];
  const int nsig = collect_signals(in, 2, &sig, which);  // y given as x: transformed once
  if (int rc = check_workspace(workspace, workspace_bytes,
                               frames_workspace_bytes(plan, batch, nsig, s.Tu)))
    return rc;
  if (int rc = transform_frames(plan, sig, nsig, batch, s.Tu, workspace, (hipStream_t)stream))
    return rc;
  const long long F = plan->nperseg / 2 + 1;
  AccumulateArgs g{};
  g.X = reinterpret_cast<const float2*>(workspace);
  g.Y = g.X + which[1] * s.Tu * F;
  g.bs = (long long)nsig * s.Tu * F;
  g.F = (int)F; g.K = (int)nk; g.G = (int)s.G; g.glen = (int)s.glen;
  g.nt = (int)((F + WL - 1) / WL);
  g.onesided = 1;
  g.scale = plan->scale / 8;  // the workspace holds 2 X / sqrt(scale); (|X|^2 + |Y|^2) / 2
  return accumulate(g, batch, skf, stream);
}

int specenh_wavenumber_spectra(const void* X, const void* Y, long long batch, long long frames,
                               long long nfreq, long long navg, long long nk, float* skf,
                               void* stream) {
  using namespace specenh;
  if (!X) return set_error(SPECENH_EINVAL, "null X");
  if (!Y) return set_error(SPECENH_EINVAL, "null Y");
  long long G;
  if (int rc = check_spectra(batch, frames, nfreq, navg, &G)) return rc;
  if (int rc = check_nk(nk)) return rc;
  if (!skf) return set_error(SPECENH_EINVAL, "null skf");
  if (batch == 0) return SPECENH_OK;
  AccumulateArgs g{};
  g.X = reinterpret_cast<const float2*>(X);
  g.Y = reinterpret_cast<const float2*>(Y);
  g.bs = frames * nfreq;
  g.F = (int)nfreq; g.K = (int)nk; g.G = (int)G; g.glen = (int)(navg >= 1 ? navg : frames);
  g.nt = (int)((nfreq + WL - 1) / WL);
  g.onesided = 0;
  g.scale = 0.5;
  return accumulate(g, batch, skf, stream);
}

}  // extern "C"
