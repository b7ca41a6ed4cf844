// spectral_matrix.hip — the cross-spectral matrix of a channel array for gfx950: per
// frequency bin and averaging group the Hermitian S[i][j] = mean_t conj(X_i) X_j of all
// channel pairs and the coherence matrix |S_ij|^2 / (S_ii S_jj) (scipy.signal.csd of every
// pair, average='mean'; the slice, scale, doubling and detrend rules of spectral_mean.hip).
//
// The F C (C + 1) / 2 complex sums do not fit one workgroup, and a fused kernel split by bin
// or channel tile would transform every frame once per part. So two kernels on one stream:
//
// csm_transform_kernel: a workgroup owns one frame of one shot and S consecutive channels.
//   It loads the S frames into LDS, detrends (fp64 sums) and windows them, transforms them
//   side by side (all of it fft_lds.hpp: one real frame per N/2-point Stockham FFT, then the
//   unpack, nothing shared between two channels) and writes 2 X to the workspace as float2
//   [shot][bin][frame][C]. The channel blocks of one frame are neighbouring
//   workgroups, so a workspace row is completed within a short time. Every frame of every
//   channel is transformed exactly once.
//
// csm_gram_kernel: a wave owns one (shot, group, bin, pair of 32-channel tiles of the upper
//   triangle). With X = A + iB over the group's frames,
//     Re S_ij = sum A_i A_j + B_i B_j,   Im S_ij = sum A_i B_j - sum B_i A_j,
//   three 32x32 accumulators on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, two frames a
//   step, one operand VGPR per lane; a lane's (A, B) is one 8-byte load straight from a
//   workspace row: lanes 0..31 are 32 consecutive channels of one frame, lanes 32..63 of the
//   next). It walks the frames in ascending order, the operands of the next 8 frames in
//   flight while the MFMAs of these 8 run; after every SPECENH_SPECTRAL_CHUNK frames the
//   fp32 partials are added to fp64 accumulators in registers and cleared. No partial sum
//   goes to memory, no atomics. Channels past C are zero operands (predicated loads, never a
//   read past a row).
//
// Bitwise structure. A product a * b does not depend on which operand is the row, so the
// chain of S_ij's real part is that of S_ji's, and sum A_i B_j - sum B_i A_j is the exact
// negative of the (j, i) value: tiles on the diagonal compute both triangles, tiles off it
// store the conjugate as the mirror, the diagonal's imaginary part is x - x = 0. A value
// depends on its two channels' samples only, not on where the channels sit in the array.
// The coherence takes S_ii from a per-lane fmaf chain over the same operands in the MFMA's
// k order (both lane halves exchange their frame), so every wave has the powers of its rows
// and columns without another wave's results.
#include <hip/hip_runtime.h>

#include <string>

#include "specenh_csm.h"
#include "runtime.hpp"
#include "averaging.hpp"
#include "fft_lds.hpp"

namespace specenh {
namespace {

constexpr int CT = 256;  // threads per workgroup (both kernels)
constexpr int CHUNK = SPECENH_SPECTRAL_CHUNK;
constexpr int TILE = 32;  // channels per MFMA tile
constexpr int MAX_LDS = 64 * 1024;

typedef float f32x16 __attribute__((ext_vector_type(16)));

using namespace fft_lds;  // load_frames, stockham, unpack2, nyquist2

struct TransformArgs {
  const float* x;          // shot b, channel c at x + b * bs + c * cs
  long long bs, cs;
  float2* ws;              // [nb][F][Tu][C]
  int C, N, log2n, hop, S, log2s, detrend;
  int Tu;                  // frames that enter a group
  int nblk;                // channel blocks: ceil(C / S)
  const float* win;
  const float2* tw;
};

// grid (Tu * nblk, 1, nb), the channel block fastest
__global__ __launch_bounds__(CT) void csm_transform_kernel(TransformArgs a) {
  extern __shared__ float2 sm[];
  __shared__ float stat[8][2];  // per slot: mean, slope
  const int N = a.N, M = N / 2, log2m = a.log2n - 1, tid = threadIdx.x;
  const int S = a.S, C = a.C;
  float2* bufA = sm;
  float2* bufB = sm + S * M;
  float* raw = reinterpret_cast<float*>(bufA);  // slot s: samples [s * N, (s + 1) * N)
  const long long tu = blockIdx.x / a.nblk, b = blockIdx.z;
  const int c0 = (int)(blockIdx.x - tu * a.nblk) * S;
  const float* xb = a.x + b * a.bs + tu * a.hop;
  load_frames<CT>(raw, stat, N, a.log2n, S, a.detrend, a.win, tid, [&](int s, int n) {
    // slots past the last channel stay zero and are not stored
    return c0 + s < C ? xb[(long long)(c0 + s) * a.cs + n] : 0.f;
  });
  const float2* res = stockham<CT>(bufA, bufB, M, log2m, S, a.tw, N, tid);
  // channels fastest: S consecutive lanes store S consecutive float2 of a workspace row
  const long long F = M + 1;
  float2* wb = a.ws + (b * F * a.Tu + tu) * C;  // bin k at wb + k * Tu * C
  const long long kstep = (long long)a.Tu * C;
  for (int idx = tid; idx < S * M; idx += CT) {
    const int s = idx & (S - 1), k = idx >> a.log2s;
    if (c0 + s >= C) continue;
    const float2 X = unpack2(res + s * M, k, M, a.tw[k]);
    wb[k * kstep + c0 + s] = X;
  }
  if (tid < S && c0 + tid < C)
    wb[M * kstep + c0 + tid] = make_float2(nyquist2(res + tid * M), 0.f);
}

struct GramArgs {
  const float2* ws;  // [nb][F][Tu][C]
  float2* csm;       // [nb][F][G][C][C], may be null
  float* coh;        // [nb][F][G][C][C], may be null
  int C, F, G, glen, Tu;
  int ntp;           // tile pairs of the upper triangle: 1 (C <= 32) or 3
  long long waves;   // nb * G * F * ntp
  double m;          // scale / (4 glen): the sums are of conj(2 X_i) 2 X_j
};

// Wave w = ((b * G + g) * F + f) * ntp + tp: the tile pairs of one matrix run side by side
// and read the same workspace rows.
__global__ __launch_bounds__(CT) void csm_gram_kernel(GramArgs a) {
  const long long w = (long long)blockIdx.x * (CT / 64) +
                      __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= a.waves) return;  // wave-uniform
  const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  const int C = a.C;
  const int tp = (int)(w % a.ntp);
  long long r = w / a.ntp;
  const int f = (int)(r % a.F);
  r /= a.F;
  const int g = (int)(r % a.G);
  const long long b = r / a.G;
  const int ti = tp == 2 ? 1 : 0, tj = tp == 0 ? 0 : 1;  // (0,0) (0,1) (1,1)
  const int ci = ti * TILE + col, cj = tj * TILE + col;
  const bool iok = ci < C, jok = cj < C;
  const bool diag = ti == tj;  // wave-uniform: the column operands are the row operands
  const float2* base = a.ws + ((b * a.F + f) * a.Tu + (long long)g * a.glen) * C;
  double drr[16], dim[16], di = 0.0, dj = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) drr[i] = dim[i] = 0.0;
  f32x16 rr = {}, p = {}, q = {};
  float pi = 0.f, pj = 0.f;
  // a batch: BS steps of two frames; BPC batches are a chunk
  constexpr int BS = 4, BPC = CHUNK / (2 * BS);
  const int nbatch = (a.glen + 2 * BS - 1) / (2 * BS);
  const int oi = half * C + ci, oj = half * C + cj;  // this lane's operands in a step's rows
  // the operands of batch bi: a lane's (A, B) of its row channel and of its column channel
  typedef float fvec __attribute__((ext_vector_type(2 * BS)));  // (A, B) of BS steps
  struct Operands {
    fvec i, j;
  };
  auto load = [&](int bi) __attribute__((always_inline)) {
    Operands o;
    const float2* fr = base + (long long)bi * (2 * BS) * C;
#pragma unroll
    for (int s = 0; s < BS; ++s) {
      const bool ok = bi * 2 * BS + 2 * s + half < a.glen;  // an odd group's last step: one frame
      float2 vi = make_float2(0.f, 0.f), vj = vi;  // past the group or past C: zero operands
      if (ok && iok) vi = fr[2 * s * C + oi];
      if (diag) vj = vi;
      else if (ok && jok) vj = fr[2 * s * C + oj];
      o.i[2 * s] = vi.x; o.i[2 * s + 1] = vi.y;
      o.j[2 * s] = vj.x; o.j[2 * s + 1] = vj.y;
    }
    return o;
  };
  auto run = [&](int bi, const Operands& o) __attribute__((always_inline)) {
#pragma unroll
    for (int s = 0; s < BS; ++s) {
      if (bi * 2 * BS + 2 * s < a.glen) {  // uniform
        const float ai = o.i[2 * s], bi_ = o.i[2 * s + 1], aj = o.j[2 * s], bj = o.j[2 * s + 1];
        rr = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, aj, rr, 0, 0, 0);
        rr = __builtin_amdgcn_mfma_f32_32x32x2f32(bi_, bj, rr, 0, 0, 0);
        p = __builtin_amdgcn_mfma_f32_32x32x2f32(ai, bj, p, 0, 0, 0);
        q = __builtin_amdgcn_mfma_f32_32x32x2f32(bi_, aj, q, 0, 0, 0);
        // |2 X|^2 of this lane's two channels in the MFMA's order: frame 2s, then 2s + 1
        const float ai2 = __shfl_xor(ai, 32), bi2 = __shfl_xor(bi_, 32);
        const float aj2 = __shfl_xor(aj, 32), bj2 = __shfl_xor(bj, 32);
        const float ai_lo = half ? ai2 : ai, ai_hi = half ? ai : ai2;
        const float bi_lo = half ? bi2 : bi_, bi_hi = half ? bi_ : bi2;
        const float aj_lo = half ? aj2 : aj, aj_hi = half ? aj : aj2;
        const float bj_lo = half ? bj2 : bj, bj_hi = half ? bj : bj2;
        pi = fmaf(ai_hi, ai_hi, fmaf(ai_lo, ai_lo, pi));
        pi = fmaf(bi_hi, bi_hi, fmaf(bi_lo, bi_lo, pi));
        pj = fmaf(aj_hi, aj_hi, fmaf(aj_lo, aj_lo, pj));
        pj = fmaf(bj_hi, bj_hi, fmaf(bj_lo, bj_lo, pj));
      }
    }
    if (bi % BPC == BPC - 1 || bi + 1 == nbatch) {  // a chunk is summed: fp64 takes over
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        drr[i] += (double)rr[i];
        dim[i] += (double)p[i] - (double)q[i];
      }
      rr = p = q = f32x16{};
      di += (double)pi;
      dj += (double)pj;
      pi = pj = 0.f;
    }
  };
  // two operand sets in turn: the next batch's loads are in flight under this batch's MFMAs
  Operands u = load(0), v = u;
  for (int bi = 0; bi < nbatch; bi += 2) {
    if (bi + 1 < nbatch) v = load(bi + 1);
    run(bi, u);
    if (bi + 1 >= nbatch) break;
    if (bi + 2 < nbatch) u = load(bi + 2);
    run(bi + 1, v);
  }
  double m = a.m;
  if (f > 0 && f < a.F - 1) m *= 2.0;
  const long long o = (((b * a.F + f) * a.G + g) * C) * C;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int rw = (i & 3) + 8 * (i >> 2) + 4 * half;  // the accumulator's row
    const double pw = __shfl(di, rw);                  // lane rw holds channel ti * 32 + rw
    const int ch = ti * TILE + rw;
    if (ch >= C || !jok) continue;
    const double re = drr[i], im = dim[i];
    const long long at = o + (long long)ch * C + cj, mir = o + (long long)cj * C + ch;
    if (a.csm) {
      a.csm[at] = make_float2((float)(re * m), (float)(im * m));
      if (ti != tj) a.csm[mir] = make_float2((float)(re * m), (float)(-im * m));
    }
    if (a.coh) {
      const float c = (float)((re * re + im * im) / (pw * dj));
      a.coh[at] = c;
      if (ti != tj) a.coh[mir] = c;
    }
  }
}

LdsOptIn g_lds;  // N >= 1024 takes 64 KiB of dynamic LDS next to the static stat[]

// the split of a call, or a negative error; validates everything but the pointers
int split_for(const specenh_stft_plan* plan, long long batch, long long channels,
              long long length, long long navg, FrameSplit* s) {
  if (int rc = check_call(plan, batch, length, navg, true, s)) return rc;
  if (channels < 2 || channels > SPECENH_CSM_MAX_CHANNELS)
    return set_error(SPECENH_EINVAL, "channels must be in [2, 64]");
  return SPECENH_OK;
}

}  // namespace

int csm_transform(const specenh_stft_plan* plan, const float* x, long long nb, int C,
                  long long channel_stride, long long batch_stride, long long Tu, float2* ws,
                  hipStream_t stream) {
  const int N = plan->nperseg;
  if (Tu * ((C + slots8_for(N) - 1) / slots8_for(N)) > 2147483647LL)
    return set_error(SPECENH_EUNSUPPORTED, "too many frames");
  hipError_t e = allow_lds(g_lds, {(const void*)csm_transform_kernel}, MAX_LDS);
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("csm: ") + hipGetErrorString(e));
  TransformArgs t{};
  t.x = x; t.ws = ws;
  t.bs = batch_stride; t.cs = channel_stride;
  t.C = C; t.N = N; t.log2n = ilog2i(N); t.hop = plan->hop;
  t.S = slots8_for(N); t.log2s = ilog2i(t.S); t.detrend = plan->detrend;
  t.Tu = (int)Tu; t.nblk = (C + t.S - 1) / t.S;
  t.win = plan->d_window; t.tw = plan->d_tw_nat;
  const size_t lds = (size_t)t.S * N * sizeof(float2);  // two buffers of S * N/2
  SPECENH_LAUNCH(csm_transform_kernel, dim3((unsigned)(Tu * t.nblk), 1, (unsigned)nb), dim3(CT),
                 lds, stream, t);
  return launched("csm_transform");
}

}  // namespace specenh

extern "C" {

size_t specenh_csm_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                   long long channels, long long length, long long navg) {
  using namespace specenh;
  FrameSplit s;
  if (split_for(plan, batch, channels, length, navg, &s) != SPECENH_OK) return 0;
  return (size_t)batch * (size_t)(plan->nperseg / 2 + 1) * (size_t)s.Tu * 2 * (size_t)channels *
         sizeof(float);
}

int specenh_csm(const specenh_stft_plan* plan, const float* x, long long batch,
                long long channels, long long length, long long channel_stride,
                long long batch_stride, long long navg, void* csm, float* coh, void* workspace,
                size_t workspace_bytes, void* stream) {
  using namespace specenh;
  if (!x) return set_error(SPECENH_EINVAL, "null x");
  FrameSplit s;
  if (int rc = split_for(plan, batch, channels, length, navg, &s)) return rc;
  if (int rc = check_stride(channel_stride, length, "channel_stride < length")) return rc;
  if (batch_stride < channels * channel_stride)
    return set_error(SPECENH_EINVAL, "batch_stride < channels * channel_stride");
  if (!csm && !coh) return set_error(SPECENH_EINVAL, "no output requested");
  if (batch == 0) return SPECENH_OK;
  const int N = plan->nperseg, C = (int)channels;
  const long long F = N / 2 + 1;
  if (int rc = check_workspace(workspace, workspace_bytes,
                               specenh_csm_workspace_bytes(plan, batch, channels, length, navg)))
    return rc;
  const int ntp = C <= TILE ? 1 : 3;
  const long long per_shot = s.G * F * ntp;  // waves of the Gram kernel
  if (per_shot > (1ll << 31)) return set_error(SPECENH_EUNSUPPORTED, "too many groups");
  GramArgs g{};
  g.C = C; g.F = (int)F; g.G = (int)s.G; g.glen = (int)s.glen; g.Tu = (int)s.Tu; g.ntp = ntp;
  g.m = plan->scale / (4.0 * (double)s.glen);
  // shots per launch: grid.z of the transform, 2^31 - 1 workgroups of the Gram kernel
  long long step = (4ll * 2147483647LL) / per_shot;
  if (step > 65535) step = 65535;
  const long long ws_shot = F * s.Tu * C, out_shot = F * s.G * C * C;
  for (long long b0 = 0; b0 < batch; b0 += step) {
    const long long nb = batch - b0 < step ? batch - b0 : step;
    float2* ws = reinterpret_cast<float2*>(workspace) + b0 * ws_shot;
    if (int rc = csm_transform(plan, x + b0 * batch_stride, nb, C, channel_stride, batch_stride,
                               s.Tu, ws, (hipStream_t)stream))
      return rc;
    g.ws = ws;
    g.csm = csm ? reinterpret_cast<float2*>(csm) + b0 * out_shot : nullptr;
    g.coh = coh ? coh + b0 * out_shot : nullptr;
    g.waves = nb * per_shot;
    const long long blocks = (g.waves + CT / 64 - 1) / (CT / 64);
    SPECENH_LAUNCH(csm_gram_kernel, dim3((unsigned)blocks), dim3(CT), 0, (hipStream_t)stream, g);
    if (int rc = launched("csm_gram")) return rc;
  }
  return SPECENH_OK;
}

}  // extern "C"
