// herm_eig.hip — batched eigendecomposition of small complex Hermitian matrices
// (2 <= n <= 64) for gfx950: the mode decomposition of the cross-spectral matrices of
// spectral_matrix.hip (eigenvalues = mode powers, leading eigenvectors = mode structures).
//
// Cyclic Jacobi in the round-robin (tournament) ordering, one wave per matrix, several
// matrices per workgroup, each wave with a private LDS region holding A and V (P x P complex,
// P = n rounded up to even, rows S = P + 1 .. 4 elements apart, see row_stride): the complex
// form of jacobi_grouped in svd_denoise.hip. A round rotates the P / 2 disjoint pairs at once:
// the lanes are grouped by pair, L = min(64 / (P / 2), P) lanes per pair, lane (pair, sub)
// covering the elements sub, sub + L, ... of rows (p, q) in the row pass and of columns
// (p, q) of A and V in the column pass. For a_pq = r e^{i phi}
//     J = diag(1, e^{-i phi}) [[c, s], [-s, c]],   A <- J^H A J,   V <- V J,
// (c, s) the real symmetric Jacobi angle of [[a_pp, r], [r, a_qq]]; every lane of a pair
// computes it in fp64 from the three entries it reads before the row pass, so a round is two
// read -> write phases and two wave-level LDS syncs; no workgroup barrier anywhere (the waves
// of a workgroup do not share anything). The column pass stores a_pq = a_qp = 0 and the two
// new diagonal entries a_pp - t r, a_qq + t r (t = s / c, fp64, imaginary part 0) in place of
// the products that are those values up to rounding.
//
// A pair is skipped when |a_pq| <= eps max(sqrt|a_pp a_qq|, 16 eps d_max), eps = 2^-24,
// d_max the largest |a_ii| of the input; a matrix stops after a sweep without a rotation.
// The sweep loop is bounded by SPECENH_HERM_EIG_MAX_SWEEPS, so no input (NaN, Inf produced
// by overflow) can make a wave spin; a matrix with a non-finite input element is answered
// with NaN before the iteration.
//
// Odd n: the padded row / column is zero, so every pair with it is skipped (|0| <= anything)
// and it never mixes with the others; the sort runs over the indices < n only, the extra
// eigenvalue 0 does not exist in the output.
//
// Storage: A and V in fp32 at every size, the angles and the new diagonal entries in fp64.
// Measured against numpy.linalg.eigh in complex128 the eigenvalue error, residual and
// orthonormality stay below 1.7e-6 max |lambda| at every n up to 64, a sixth
// of the 1e-5 contract, so no size needs fp64 storage.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "fft_common.hpp"
#include "runtime.hpp"
#include "specenh_modes.h"

namespace specenh {

namespace {

constexpr int MAX_SWEEPS = SPECENH_HERM_EIG_MAX_SWEEPS;
constexpr int MAX_WAVES = 4;         // matrices per workgroup at most
constexpr int WG_LDS = 64 * 1024;    // LDS a workgroup of several matrices stays under
constexpr int MAX_LDS = 160 * 1024;  // one matrix may take the CU's
constexpr int TAIL = 64 * 4 * 2;     // per-matrix LDS after A and V: w[64], order[64]

using T = float;  // storage of A and V
using T2 = float2;

struct EigArgs {
  const float2* a;
  long long count, mstride;
  float* w;
  float2* v;
  int* sweeps;
  int n, P, S, L, k, mpw;
  unsigned lds_per;  // bytes of LDS per matrix
};

// x * z
__device__ __forceinline__ T2 cmul(T2 x, T2 z) {
  T2 r;
  r.x = x.x * z.x - x.y * z.y;
  r.y = x.x * z.y + x.y * z.x;
  return r;
}
// x * conj(z)
__device__ __forceinline__ T2 cmulc(T2 x, T2 z) {
  T2 r;
  r.x = x.x * z.x + x.y * z.y;
  r.y = x.y * z.x - x.x * z.y;
  return r;
}

// U: elements a lane reads before it writes them back (8: 203 VGPRs, two waves per
// SIMD, for the sizes where a lane has more than 4 elements a pass; 4: 123 VGPRs, four waves
// per SIMD, for the small matrices whose LDS footprint lets that many run)
template <int U>
__global__ __launch_bounds__(64 * MAX_WAVES) void herm_eig_kernel(EigArgs g) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * g.mpw + wave;
  if (m >= g.count) return;  // wave-uniform; nothing below is a workgroup barrier
  const int n = g.n, P = g.P, S = g.S;
  unsigned char* base = smem + (size_t)wave * g.lds_per;
  T2* sA = reinterpret_cast<T2*>(base);
  T2* sV = sA + P * S;
  float* sW = reinterpret_cast<float*>(sV + P * S);
  int* sOrd = reinterpret_cast<int*>(sW + 64);

  // ---- load: upper triangle and the diagonal's real part; V = I
  for (int idx = lane; idx < P * S; idx += 64) {
    T2 z;
    z.x = 0; z.y = 0;
    sA[idx] = z;
    z.x = (idx / S == idx % S) ? 1 : 0;
    sV[idx] = z;
  }
  wave_lds_sync();
  const float2* A = g.a + m * g.mstride;
  bool bad = false;
  float dmax = 0.f;
  for (int idx = lane; idx < n * n; idx += 64) {
    const int i = idx / n, j = idx - i * n;
    if (i > j) continue;
    const float2 z = A[idx];
    T2 t;
    t.x = z.x;
    if (i == j) {
      bad |= !isfinite(z.x);
      dmax = fmaxf(dmax, fabsf(z.x));
      t.y = 0;
      sA[i * S + i] = t;
    } else {
      bad |= !(isfinite(z.x) && isfinite(z.y));
      t.y = z.y;
      sA[i * S + j] = t;
      t.y = -z.y;
      sA[j * S + i] = t;
    }
  }
  for (int s = 32; s >= 1; s >>= 1) dmax = fmaxf(dmax, __shfl_xor(dmax, s));
  if (__any(bad)) {  // this matrix alone is answered with NaN
    const float qn = __builtin_nanf("");
    if (lane < n) {
      if (g.w) g.w[m * n + lane] = qn;
      for (int r = 0; r < g.k; ++r) g.v[(m * g.k + r) * n + lane] = make_float2(qn, qn);
    }
    if (g.sweeps && lane == 0) g.sweeps[m] = 0;
    return;
  }
  wave_lds_sync();

  // ---- sweeps
  const int NP = P >> 1, L = g.L;
  const int j = lane / L, sub = lane - j * L;
  const bool live = j < NP;
  // tournament players of pair j: kA = j (player 0 never moves), kB = P - 1 - j; player
  // k > 0 sits at 1 + (k - 1 + round) mod (P - 1)
  const int kA = live ? j : 0, kB = live ? P - 1 - j : P - 1;
  const int ra0 = kA == 0 ? 0 : kA - 1, rb0 = kB - 1;
  const double eps = 5.9604644775390625e-08;  // 2^-24
  const double dfloor = 16.0 * eps * (double)dmax;
  int sweep = 0;
  while (sweep < MAX_SWEEPS) {
    bool rotated = false;
    int ra = ra0, rb = rb0;
    for (int round = 0; round < P - 1; ++round) {
      int a = kA == 0 ? 0 : 1 + ra, b = 1 + rb;
      if (a > b) { const int t = a; a = b; b = t; }
      const double haa = sA[a * S + a].x, hbb = sA[b * S + b].x;
      const T2 hab = sA[a * S + b];
      const double hx = hab.x, hy = hab.y;
      const double r = sqrt(hx * hx + hy * hy);
      const double thr = eps * fmax(sqrt(fabs(haa * hbb)), dfloor);
      const bool rot = live && !(r <= thr);  // (a NaN rotates: the sweep bound ends it)
      T c = 1, s = 0;
      T2 se, ce;  // s e^{i phi}, c e^{i phi}
      se.x = se.y = ce.y = 0; ce.x = 1;
      double dpp = haa, dqq = hbb;
      if (rot) {
        const double tau = (hbb - haa) / (2.0 * r);
        const double tt = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double cd = 1.0 / sqrt(1.0 + tt * tt), sd = tt * cd;
        const double ex = hx / r, ey = hy / r;
        c = (T)cd; s = (T)sd;
        se.x = (T)(sd * ex); se.y = (T)(sd * ey);
        ce.x = (T)(cd * ex); ce.y = (T)(cd * ey);
        dpp = haa - tt * r;
        dqq = hbb + tt * r;
        // row pass: rows p, q of A <- J^H A
        for (int k0 = sub; k0 < P; k0 += L * U) {
          T2 xa[U], xb[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int k = min(k0 + L * u, P - 1);
            xa[u] = sA[a * S + k];
            xb[u] = sA[b * S + k];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int k = k0 + L * u;
            if (k < P) {
              const T2 p1 = cmul(xb[u], se), p2 = cmul(xb[u], ce);
              T2 na, nb;
              na.x = c * xa[u].x - p1.x; na.y = c * xa[u].y - p1.y;
              nb.x = s * xa[u].x + p2.x; nb.y = s * xa[u].y + p2.y;
              sA[a * S + k] = na;
              sA[b * S + k] = nb;
            }
          }
        }
      }
      wave_lds_sync();
      if (rot) {
        // column pass: columns p, q of A <- A J and V <- V J; the pair's 2 x 2 block is known
        for (int k0 = sub; k0 < P; k0 += L * U) {
          T2 xa[U], xb[U], qa[U], qb[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int k = min(k0 + L * u, P - 1);
            xa[u] = sA[k * S + a];
            xb[u] = sA[k * S + b];
            qa[u] = sV[k * S + a];
            qb[u] = sV[k * S + b];
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int k = k0 + L * u;
            if (k < P) {
              T2 p1 = cmulc(xb[u], se), p2 = cmulc(xb[u], ce);
              T2 na, nb;
              na.x = c * xa[u].x - p1.x; na.y = c * xa[u].y - p1.y;
              nb.x = s * xa[u].x + p2.x; nb.y = s * xa[u].y + p2.y;
              if (k == a) { na.x = (T)dpp; na.y = 0; nb.x = 0; nb.y = 0; }
              if (k == b) { na.x = 0; na.y = 0; nb.x = (T)dqq; nb.y = 0; }
              sA[k * S + a] = na;
              sA[k * S + b] = nb;
              p1 = cmulc(qb[u], se); p2 = cmulc(qb[u], ce);
              na.x = c * qa[u].x - p1.x; na.y = c * qa[u].y - p1.y;
              nb.x = s * qa[u].x + p2.x; nb.y = s * qa[u].y + p2.y;
              sV[k * S + a] = na;
              sV[k * S + b] = nb;
            }
          }
        }
      }
      wave_lds_sync();
      rotated |= rot;
      ra = ra + 1 == P - 1 ? 0 : ra + 1;
      rb = rb + 1 == P - 1 ? 0 : rb + 1;
    }
    ++sweep;
    if (!__any(rotated)) break;
  }

  // ---- eigenvalues, descending, stable by index, over the n real indices only
  sW[lane] = lane < n ? (float)sA[lane * S + lane].x : 0.f;
  sOrd[lane] = lane < n ? lane : 0;
  wave_lds_sync();
  float wi = 0.f;
  int rank = 0;
  if (lane < n) {
    wi = sW[lane];
    for (int i = 0; i < n; ++i) {
      const float wj = sW[i];
      rank += (wj > wi || (wj == wi && i < lane)) ? 1 : 0;
    }
  }
  wave_lds_sync();
  if (lane < n) {  // rank < n whatever the values (a NaN from overflow compares false)
    sOrd[rank] = lane;
    if (g.w) g.w[m * n + rank] = wi;
  }
  if (g.sweeps && lane == 0) g.sweeps[m] = sweep;
  wave_lds_sync();

  // ---- eigenvectors: column order[r] of V, one component per lane; unit norm, the
  // component of largest modulus (lowest index on ties) real positive
  for (int r = 0; r < g.k; ++r) {
    const int col = sOrd[r];
    double zx = 0.0, zy = 0.0;
    if (lane < n) {
      const T2 z = sV[lane * S + col];
      zx = z.x; zy = z.y;
    }
    const double m2 = zx * zx + zy * zy;
    double sum = m2, best = m2;
    int bi = lane;
    for (int s = 32; s >= 1; s >>= 1) {
      sum += __shfl_xor(sum, s);
      const double ob = __shfl_xor(best, s);
      const int oi = __shfl_xor(bi, s);
      if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    bi &= 63;
    const double mx = __shfl(zx, bi), my = __shfl(zy, bi);
    const double am = sqrt(best), inv = 1.0 / sqrt(sum);
    const double px = mx / am, py = -my / am;  // conj(z_max) / |z_max|
    float2 o;
    o.x = (float)((zx * px - zy * py) * inv);
    o.y = (float)((zx * py + zy * px) * inv);
    if (lane == bi) { o.x = (float)(am * inv); o.y = 0.f; }
    if (lane < n) g.v[(m * g.k + r) * n + lane] = o;
  }
}

// Row stride of A and V in elements: P plus the pad in 1 .. 4 with the fewest LDS cycles a
// round in the bank model, per P = 2, 4, .. 64 (tools/herm_eig_banks.py --table; without a
// pad the rows of P = 32, 64 start in one bank: 32 cycles per row-pass instruction against
// 3 to 5 padded).
inline int row_stride(int P) {
  static const signed char PAD[32] = {1, 2, 3, 2, 4, 2, 4, 2, 2, 2, 4, 2, 2, 1, 4, 4,
                                      3, 1, 4, 3, 1, 2, 4, 2, 4, 2, 4, 2, 4, 2, 4, 2};
  return P + PAD[P / 2 - 1];
}

LdsOptIn g_lds[2];  // herm_eig_kernel<4>, <8>

}  // namespace
}  // namespace specenh

extern "C" {

int specenh_herm_eig(const void* a, long long count, long long n, long long matrix_stride,
                     long long k, float* w, void* v, int* sweeps, void* stream) {
  using namespace specenh;
  if (!a) return set_error(SPECENH_EINVAL, "null a");
  if (count < 0) return set_error(SPECENH_EINVAL, "count must be >= 0");
  if (n < 2 || n > SPECENH_HERM_EIG_MAX_N) return set_error(SPECENH_EINVAL, "n must be in [2, 64]");
  if (k < 0 || k > n) return set_error(SPECENH_EINVAL, "k must be in [0, n]");
  if (matrix_stride < n * n) return set_error(SPECENH_EINVAL, "matrix_stride < n * n");
  if (count == 0) return SPECENH_OK;
  if (k > 0 && !v) return set_error(SPECENH_EINVAL, "null v with k > 0");
  if (!w && !sweeps && k == 0) return set_error(SPECENH_EINVAL, "no output requested");
  if (reinterpret_cast<size_t>(a) % 8) return set_error(SPECENH_EINVAL, "a must be 8-byte aligned");
  if (k > 0 && reinterpret_cast<size_t>(v) % 8)
    return set_error(SPECENH_EINVAL, "v must be 8-byte aligned");
  if (matrix_stride > (1ll << 40) || count > (1ll << 40))
    return set_error(SPECENH_EUNSUPPORTED, "count or matrix_stride too large");
  EigArgs g{};
  g.n = (int)n; g.P = (int)(n + (n & 1)); g.S = row_stride(g.P); g.k = (int)k;
  const int NP = g.P / 2;
  g.L = 64 / NP < g.P ? 64 / NP : g.P;
  g.lds_per = (unsigned)(((size_t)2 * g.P * g.S * sizeof(T2) + TAIL + 15) / 16 * 16);
  g.mpw = WG_LDS / (int)g.lds_per;
  g.mpw = g.mpw < 1 ? 1 : g.mpw > MAX_WAVES ? MAX_WAVES : g.mpw;
  g.mstride = matrix_stride;
  const size_t lds = (size_t)g.mpw * g.lds_per;
  if (lds > (size_t)MAX_LDS) return set_error(SPECENH_EUNSUPPORTED, "matrix does not fit LDS");
  const bool wide = (g.P + g.L - 1) / g.L > 4;  // elements a lane has in a pass
  hipError_t e = allow_lds(g_lds[wide], {wide ? (const void*)herm_eig_kernel<8>
                                              : (const void*)herm_eig_kernel<4>}, MAX_LDS);
  if (e != hipSuccess)
    return set_error(SPECENH_EHIP, std::string("herm_eig: ") + hipGetErrorString(e));
  const long long step = (1ll << 30);  // matrices per launch (grid.x < 2^31)
  for (long long m0 = 0; m0 < count; m0 += step) {
    const long long nm = count - m0 < step ? count - m0 : step;
    g.count = nm;
    g.a = reinterpret_cast<const float2*>(a) + m0 * matrix_stride;
    g.w = w ? w + m0 * n : nullptr;
    g.v = k > 0 ? reinterpret_cast<float2*>(v) + m0 * k * n : nullptr;
    g.sweeps = sweeps ? sweeps + m0 : nullptr;
    const unsigned blocks = (unsigned)((nm + g.mpw - 1) / g.mpw);
    const dim3 grid(blocks), block(64 * g.mpw);
    if (wide)
      SPECENH_LAUNCH(herm_eig_kernel<8>, grid, block, lds, (hipStream_t)stream, g);
    else
      SPECENH_LAUNCH(herm_eig_kernel<4>, grid, block, lds, (hipStream_t)stream, g);
    e = hipGetLastError();
    if (e != hipSuccess)
      return set_error(SPECENH_EHIP, std::string("herm_eig launch: ") + hipGetErrorString(e));
  }
  return SPECENH_OK;
}

}  // extern "C"
