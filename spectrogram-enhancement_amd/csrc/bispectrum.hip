// bispectrum.hip — the bispectrum and squared bicoherence for gfx950: per averaging group
//   B[k][l] = mean_t X_t[k] Y_t[l] conj(Z_t[k+l]),  b2 = |B|^2 / (mean|X Y|^2 mean|Z_{k+l}|^2)
// on the (k, l) plane k + l <= N/2 (include/specenh_bispectrum.h; X_t is
// scipy.signal.spectrogram(mode='complex'), the slice and detrend rules of spectral_mean.hip).
//
// The work is quadratic in the bins and indexed by k + l (a Hankel structure), so it is no
// Gram product and the matrix cores do not apply: a VALU kernel fed from LDS. Two kernels on
// one stream:
//
// bispectrum_transform_kernel: a workgroup owns S consecutive frames of one signal of one
//   shot. It loads them into LDS, detrends (fp64 sums) and windows them, transforms them side
//   by side (all of it fft_lds.hpp, one real frame per N/2-point FFT) and writes 2 X,
//   unscaled, to the workspace as float2 [shot][signal][frame][F]: frame-major with the bins
//   contiguous, what the second kernel streams. Every frame of every distinct signal is
//   transformed exactly once; y or z that alias another signal share its spectra. Its launch
//   is transform_frames() (averaging.hpp), which wavenumber.hip calls too.
//
// bispectrum_accumulate_kernel: a workgroup owns one (shot, group, 64 x 64 tile of the plane),
//   a wave a 32 x 32 quarter of it. Per step of FS frames the workgroup stages the three bin
//   ranges it needs into LDS: 64 of X, 64 of Y and the 127 of Z that k + l reaches (one
//   element a thread and frame, loaded into registers a step ahead of its use). Lane
//   (i, j) of a wave keeps the 4 x 4 micro-tile k = kw + i + 8 a, l = lw + j + 8 b strided
//   across the wave: the 32 lanes an LDS read serves at once then touch 8 consecutive
//   float2 of X, 4 of Y and 11 of Z (ds_read_b64, no bank conflict), and a lane needs only
//   4 + 4 + 7 reads a frame for its 16 pairs (k + l = kw + lw + i + j + 8 (a + b)). It walks
//   the group's frames in ascending order: P = X_k Y_l, B += P conj(Z_{k+l}), D += |P|^2,
//   E_{k+l} += |Z_{k+l}|^2, in fp32 for at most SPECENH_SPECTRAL_CHUNK frames; then the
//   partials are added to fp64 accumulators in registers and cleared. b2 is formed in fp64
//   from the unrounded sums; the bispectrum's scale (sqrt(scale) / 2)^3 / frames is applied in
//   fp64 to the sum. No partial sum goes to memory, no atomics.
//
// Bitwise structure. Every lane runs the same chain on the same operands for a given (k, l),
// and the tile grid is anchored at bin 0, so an element does not depend on the batch, on
// nbins or on where its tile sits. In the auto case (y and z alias x) only l <= k is
// computed and stored to [k][l] and [l][k]: tiles above the diagonal leave at once, the wave
// of a diagonal tile that lies wholly above it idles.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "specenh_bispectrum.h"
#include "runtime.hpp"
#include "averaging.hpp"
#include "fft_lds.hpp"

namespace specenh {
namespace {

using namespace fft_lds;  // load_frames, stockham, unpack2, nyquist2

constexpr int CT = 256;  // threads per workgroup (both kernels)
constexpr int CHUNK = SPECENH_SPECTRAL_CHUNK;
constexpr int MAX_LDS = 64 * 1024;
constexpr int TILE = 64;  // bins of k and of l a workgroup owns
constexpr int WT = 32;    // ... a wave owns
constexpr int FS = 8;     // frames staged at once
constexpr int ROW = 256;  // float2 a staged frame takes: X 64 | Y 64 | Z 127 (+ 1 unused)
static_assert(CHUNK % FS == 0, "a chunk is a whole number of staging steps");
static_assert(2 * TILE + 2 * TILE - 1 <= ROW && ROW == CT, "one staged element per thread");

struct TransformArgs {
  FrameSignals sig;
  int nsig;
  float2* ws;  // [nb][nsig][Tu][F]
  int N, log2n, hop, S, detrend;
  int Tu;      // frames that enter a group
  const float* win;
  const float2* tw;
};

// grid (ceil(Tu / S), nsig, nb)
__global__ __launch_bounds__(CT) void bispectrum_transform_kernel(TransformArgs a) {
  extern __shared__ float2 sm[];
  __shared__ float stat[8][2];  // per slot: mean, slope
  const int N = a.N, M = N / 2, log2m = a.log2n - 1, tid = threadIdx.x;
  const int S = a.S;
  float2* bufA = sm;
  float2* bufB = sm + S * M;
  float* raw = reinterpret_cast<float*>(bufA);  // slot s: samples [s * N, (s + 1) * N)
  const int t0 = blockIdx.x * S, sg = blockIdx.y;
  const long long b = blockIdx.z;
  const float* xb = a.sig.p[sg] + b * a.sig.stride[sg];
  load_frames<CT>(raw, stat, N, a.log2n, S, a.detrend, a.win, tid, [&](int s, int n) {
    // slots past the last frame stay zero and are not stored
    return t0 + s < a.Tu ? xb[(long long)(t0 + s) * a.hop + n] : 0.f;
  });
  const float2* res = stockham<CT>(bufA, bufB, M, log2m, S, a.tw, N, tid);
  // bins fastest: consecutive lanes store consecutive float2 of a frame's row
  const long long F = M + 1;
  float2* wb = a.ws + ((b * a.nsig + sg) * a.Tu + t0) * F;  // slot s, bin k at wb + s * F + k
  for (int idx = tid; idx < S * M; idx += CT) {
    const int s = idx >> log2m, k = idx & (M - 1);
    if (t0 + s >= a.Tu) continue;
    wb[s * F + k] = unpack2(res + s * M, k, M, a.tw[k]);
  }
  if (tid < S && t0 + tid < a.Tu) wb[tid * F + M] = make_float2(nyquist2(res + tid * M), 0.f);
}

struct AccumulateArgs {
  const float2* X;  // frame t of shot b at X + b * bs + t * F, likewise Y and Z
  const float2* Y;
  const float2* Z;
  long long bs;
  float2* bis;      // [nb][G][K][K], may be null
  float* coh;       // [nb][G][K][K], may be null
  int F, K, G, glen;
  int nt;           // tiles along k and along l: ceil(K / TILE)
  int autoc;        // Y and Z are X: compute l <= k, store both
  double scale;     // of the bispectrum's sum, before the division by glen
};

// grid (G * nt * nt, nb): the tiles of one group run side by side and read the same rows
__global__ __launch_bounds__(CT) void bispectrum_accumulate_kernel(AccumulateArgs a) {
  __shared__ float2 st[FS * ROW];
  const int tid = threadIdx.x;
  const int ntt = a.nt * a.nt;
  const int g = blockIdx.x / ntt, tile = blockIdx.x - g * ntt;
  const int tk = tile / a.nt, tl = tile - tk * a.nt;
  if (a.autoc && tl > tk) return;  // uniform: the mirror of tile (tl, tk)
  const long long b = blockIdx.y;
  const int F = a.F, K = a.K, top = F - 1;  // the domain is k + l <= top
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int i = lane & 7, j = lane >> 3;
  const int kw = (wave & 1) * WT, lw = (wave >> 1) * WT;
  const int k0 = tk * TILE, l0 = tl * TILE;
  const bool live = k0 + l0 <= top;  // uniform: part of the tile is inside the domain
  // wave-uniform: some pair of this wave is stored with a value
  const bool active = live && k0 + kw < K && l0 + lw < K && k0 + kw + l0 + lw <= top &&
                      !(a.autoc && l0 + lw >= k0 + kw + WT);
  float br[16], bi[16], d[16], e[7];
  double Br[16], Bi[16], D[16], E[7];
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    br[p] = bi[p] = d[p] = 0.f;
    Br[p] = Bi[p] = D[p] = 0.0;
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    e[c] = 0.f;
    E[c] = 0.0;
  }
  if (live) {
    // this thread's element of a staged row: X[k0 ..], Y[l0 ..] or Z[k0 + l0 ..]
    const long long first = b * a.bs + (long long)g * a.glen * F;
    const float2* src;
    int bin;
    if (tid < TILE) {
      src = a.X;
      bin = k0 + tid;
    } else if (tid < 2 * TILE) {
      src = a.Y;
      bin = l0 + tid - TILE;
    } else {
      src = a.Z;
      bin = k0 + l0 + tid - 2 * TILE;
    }
    const bool ok = bin < F;  // bins past the spectrum are zero operands, never a read past a row
    src += first + (ok ? bin : 0);
    const float2* rx = st + kw + i;
    const float2* ry = st + TILE + lw + j;
    const float2* rz = st + 2 * TILE + kw + lw + i + j;
    float2 v[FS];  // this thread's element of the frames of a step, in flight a step ahead
    auto fetch = [&](int f0) __attribute__((always_inline)) {
#pragma unroll
      for (int f = 0; f < FS; ++f) {
        v[f] = make_float2(0.f, 0.f);
        if (ok && f0 + f < a.glen) v[f] = src[(long long)(f0 + f) * F];
      }
    };
    fetch(0);
    for (int f0 = 0; f0 < a.glen; f0 += FS) {
      __syncthreads();  // the reads of the step before are done
#pragma unroll
      for (int f = 0; f < FS; ++f) st[f * ROW + tid] = v[f];
      __syncthreads();
      if (f0 + FS < a.glen) fetch(f0 + FS);  // the next step's loads run under this step's sums
      if (active) {
        const int nf = a.glen - f0 < FS ? a.glen - f0 : FS;
        for (int f = 0; f < nf; ++f) {
          float2 x[4], y[4], z[7];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            x[q] = rx[f * ROW + 8 * q];
            y[q] = ry[f * ROW + 8 * q];
          }
#pragma unroll
          for (int c = 0; c < 7; ++c) {
            z[c] = rz[f * ROW + 8 * c];
            e[c] = fmaf(z[c].x, z[c].x, fmaf(z[c].y, z[c].y, e[c]));
          }
#pragma unroll
          for (int qa = 0; qa < 4; ++qa) {
#pragma unroll
            for (int qb = 0; qb < 4; ++qb) {
              const int p = qa * 4 + qb;
              const float2 X = x[qa], Y = y[qb], Zc = z[qa + qb];
              const float pr = fmaf(X.x, Y.x, -(X.y * Y.y));
              const float pi = fmaf(X.x, Y.y, X.y * Y.x);
              br[p] = fmaf(pr, Zc.x, fmaf(pi, Zc.y, br[p]));   // Re P conj(Z)
              bi[p] = fmaf(pi, Zc.x, fmaf(-pr, Zc.y, bi[p]));  // Im P conj(Z)
              d[p] = fmaf(pr, pr, fmaf(pi, pi, d[p]));
            }
          }
        }
        if ((f0 + FS) % CHUNK == 0 || f0 + FS >= a.glen) {  // a chunk is summed: fp64 takes over
#pragma unroll
          for (int p = 0; p < 16; ++p) {
            Br[p] += (double)br[p];
            Bi[p] += (double)bi[p];
            D[p] += (double)d[p];
            br[p] = bi[p] = d[p] = 0.f;
          }
#pragma unroll
          for (int c = 0; c < 7; ++c) {
            E[c] += (double)e[c];
            e[c] = 0.f;
          }
        }
      }
    }
  }
  const long long o = (b * a.G + g) * (long long)K * K;
  const double glen = (double)a.glen;
#pragma unroll
  for (int qa = 0; qa < 4; ++qa) {
#pragma unroll
    for (int qb = 0; qb < 4; ++qb) {
      const int p = qa * 4 + qb;
      const int k = k0 + kw + i + 8 * qa, l = l0 + lw + j + 8 * qb;
      if (k >= K || l >= K || (a.autoc && l > k)) continue;
      float2 bv = make_float2(0.f, 0.f);
      float cv = 0.f;
      if (k + l <= top) {  // inside the domain: this wave was active
        bv = make_float2((float)(Br[p] * a.scale / glen), (float)(Bi[p] * a.scale / glen));
        cv = (float)((Br[p] * Br[p] + Bi[p] * Bi[p]) / (D[p] * E[qa + qb]));
      }
      const long long at = o + (long long)k * K + l, mir = o + (long long)l * K + k;
      if (a.bis) {
        a.bis[at] = bv;
        if (a.autoc && l < k) a.bis[mir] = bv;
      }
      if (a.coh) {
        a.coh[at] = cv;
        if (a.autoc && l < k) a.coh[mir] = cv;
      }
    }
  }
}

LdsOptIn g_lds;  // N >= 1024 takes 64 KiB of dynamic LDS next to the static stat[]

// the accumulate launches of a call: shots [0, batch) in steps of grid.y
int accumulate(AccumulateArgs g, long long batch, void* bispec, float* bicoh, void* stream) {
  const long long per_shot = (long long)g.G * g.nt * g.nt;
  if (per_shot > 2147483647LL) return set_error(SPECENH_EUNSUPPORTED, "too many groups");
  const long long out_shot = (long long)g.G * g.K * g.K;
  const float2 *X = g.X, *Y = g.Y, *Z = g.Z;
  for (long long b0 = 0; b0 < batch; b0 += 65535) {
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    g.X = X + b0 * g.bs;
    g.Y = Y + b0 * g.bs;
    g.Z = Z + b0 * g.bs;
    g.bis = bispec ? reinterpret_cast<float2*>(bispec) + b0 * out_shot : nullptr;
    g.coh = bicoh ? bicoh + b0 * out_shot : nullptr;
    SPECENH_LAUNCH(bispectrum_accumulate_kernel, dim3((unsigned)per_shot, (unsigned)nb),
                   dim3(CT), 0, (hipStream_t)stream, g);
    if (int rc = launched("bispectrum_accumulate")) return rc;
  }
  return SPECENH_OK;
}

}  // namespace

// averaging.hpp: the transform launches of a call, shots [0, batch) in steps of grid.z
int transform_frames(const specenh_stft_plan* plan, const FrameSignals& sig, int nsig,
                     long long batch, long long Tu, void* workspace, hipStream_t stream) {
  hipError_t e = allow_lds(g_lds, {(const void*)bispectrum_transform_kernel}, MAX_LDS);
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("bispectrum: ") + hipGetErrorString(e));
  const int N = plan->nperseg;
  const long long F = N / 2 + 1;
  TransformArgs t{};
  t.sig = sig;
  t.nsig = nsig;
  t.N = N; t.log2n = ilog2i(N); t.hop = plan->hop;
  t.S = slots8_for(N); t.detrend = plan->detrend;
  t.Tu = (int)Tu;
  t.win = plan->d_window; t.tw = plan->d_tw_nat;
  const size_t lds = (size_t)t.S * N * sizeof(float2);  // two buffers of S * N/2
  const long long ws_shot = (long long)nsig * Tu * F;
  const long long blocks = (Tu + t.S - 1) / t.S;
  for (long long b0 = 0; b0 < batch; b0 += 65535) {  // grid.z
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    for (int u = 0; u < nsig; ++u) t.sig.p[u] = sig.p[u] + b0 * sig.stride[u];
    t.ws = reinterpret_cast<float2*>(workspace) + b0 * ws_shot;
    SPECENH_LAUNCH(bispectrum_transform_kernel, dim3((unsigned)blocks, (unsigned)nsig, (unsigned)nb),
                   dim3(CT), lds, stream, t);
    if (int rc = launched("bispectrum_transform")) return rc;
  }
  return SPECENH_OK;
}

}  // namespace specenh

extern "C" {

size_t specenh_bispectrum_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                          long long nsignals, long long length,
                                          long long navg) {
  using namespace specenh;
  FrameSplit s;
  if (check_call(plan, batch, length, navg, true, &s) != SPECENH_OK) return 0;
  if (nsignals < 1 || nsignals > 3) {
    set_error(SPECENH_EINVAL, "nsignals must be in [1, 3]");
    return 0;
  }
  return frames_workspace_bytes(plan, batch, nsignals, s.Tu);
}

int specenh_bispectrum(const specenh_stft_plan* plan, const float* x, const float* y,
                       const float* z, long long batch, long long length, long long x_stride,
                       long long y_stride, long long z_stride, long long navg, long long nbins,
                       void* bispec, float* bicoh, void* workspace, size_t workspace_bytes,
                       void* stream) {
  using namespace specenh;
  if (!x) return set_error(SPECENH_EINVAL, "null x");
  FrameSplit s;
  if (int rc = check_call(plan, batch, length, navg, true, &s)) return rc;
  const SignalArg in[] = {{x, x_stride, "x_stride < length"}, {y, y_stride, "y_stride < length"},
                          {z, z_stride, "z_stride < length"}};
  if (int rc = check_strides(in, 3, length)) return rc;
  const int N = plan->nperseg;
  const long long F = N / 2 + 1;
  if (nbins <= 0) nbins = F;
  if (nbins > F) return set_error(SPECENH_EINVAL, "nbins must be in [1, nperseg/2 + 1]");
  if (!bispec && !bicoh) return set_error(SPECENH_EINVAL, "no output requested");
  if (batch == 0) return SPECENH_OK;
  // the distinct signals, and which of them y and z are
  FrameSignals sig{};
  int which[3];
  const int nsig = collect_signals(in, 3, &sig, which);
  if (int rc = check_workspace(workspace, workspace_bytes,
                               frames_workspace_bytes(plan, batch, nsig, s.Tu)))
    return rc;
  if (int rc = transform_frames(plan, sig, nsig, batch, s.Tu, workspace, (hipStream_t)stream))
    return rc;
  const long long ws_shot = (long long)nsig * s.Tu * F;
  AccumulateArgs g{};
  const float2* ws = reinterpret_cast<const float2*>(workspace);
  g.X = ws;
  g.Y = ws + which[1] * s.Tu * F;
  g.Z = ws + which[2] * s.Tu * F;
  g.bs = ws_shot;
  g.F = (int)F; g.K = (int)nbins; g.G = (int)s.G; g.glen = (int)s.glen;
  g.nt = (int)((nbins + TILE - 1) / TILE);
  g.autoc = nsig == 1;
  const double h = 0.5 * std::sqrt(plan->scale);  // the workspace holds 2 X / sqrt(scale)
  g.scale = h * h * h;
  return accumulate(g, batch, bispec, bicoh, stream);
}

int specenh_bispectrum_spectra(const void* X, const void* Y, const void* Z, long long batch,
                               long long frames, long long nfreq, long long navg,
                               long long nbins, void* bispec, float* bicoh, void* stream) {
  using namespace specenh;
  if (!X) return set_error(SPECENH_EINVAL, "null X");
  long long G;
  if (int rc = check_spectra(batch, frames, nfreq, navg, &G)) return rc;
  if (nbins <= 0) nbins = nfreq;
  if (nbins > nfreq) return set_error(SPECENH_EINVAL, "nbins must be in [1, nfreq]");
  if (!bispec && !bicoh) return set_error(SPECENH_EINVAL, "no output requested");
  if (batch == 0) return SPECENH_OK;
  AccumulateArgs g{};
  g.X = reinterpret_cast<const float2*>(X);
  g.Y = Y ? reinterpret_cast<const float2*>(Y) : g.X;
  g.Z = Z ? reinterpret_cast<const float2*>(Z) : g.X;
  g.bs = frames * nfreq;
  g.F = (int)nfreq; g.K = (int)nbins; g.G = (int)G; g.glen = (int)(navg >= 1 ? navg : frames);
  g.nt = (int)((nbins + TILE - 1) / TILE);
  g.autoc = g.Y == g.X && g.Z == g.X;
  g.scale = 1.0;
  return accumulate(g, batch, bispec, bicoh, stream);
}

}  // extern "C"
