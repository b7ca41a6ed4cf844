// kmeans.hip — one Lloyd iteration of k-means on the GPU. include/specenh_kmeans.h has the
// arithmetic, its order and the rounding counts c_s, c_u, c_i; tests/kmeans_local.py the numpy
// restatement.
//
// Assignment, s_j = |c_j|^2 - 2 x.c_j. cnorm_kernel: a wave per centre. assign_kernel: a
// workgroup of four waves per tile of 64 points against all k centres. d is walked in chunks of
// 32: the tile's chunk of X (coalesced, 128 bytes a row) and the centres' chunk (transposed, so
// that a B operand is 32 neighbouring dwords) are staged in LDS with zeros past n, k and d.
// Wave w takes the 32 points (w & 1) and the column half (w >> 1) of the centres, at most four
// 32 x 32 blocks: per block a chunk is one v_mfma_f32_32x32x2_f32 chain from zero, then added
// to the block's running product. The epilogue forms the scores in registers, each lane
// reduces its blocks, the (score, index) pairs go through LDS and four threads a point finish
// the argmin; ties go to the lower index at every step, so the order of the reduction does not
// matter. The [n, k] scores never leave the workgroup.
//
// Update. update_kernel: a wave per (slab of points, 32 columns of d), no LDS traffic in its
// loop: the B operand is X itself (32 neighbouring floats of a row, coalesced), the A operand
// the one-hot of the two points' labels, built in registers, so sums = onehot^T X accumulates
// on the matrix cores in point order. The same wave adds (x - c_label)^2 for its columns, and
// the waves of column block 0 count the slab's labels in an LDS histogram (integer adds).
// reduce_kernel adds a batch item's count and inertia partials, finalize_kernel its slab sums
// in slab order and divides. No floating-point atomics.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <string>

#include "specenh_kmeans.h"
#include "runtime.hpp"
#include "wave.hpp"

namespace specenh {
namespace {

constexpr int MAXK = SPECENH_KMEANS_MAX_K;
constexpr int MAXD = SPECENH_KMEANS_MAX_D;
constexpr int TP = SPECENH_KMEANS_TILE;   // points of a workgroup: two MFMA row blocks
constexpr int KC = SPECENH_KMEANS_CHUNK;  // d of a chunk
constexpr int XP = KC + 1;                // pitch of a staged point: odd, A reads hit 32 banks
constexpr int CP = MAXK + 1;              // pitch of a staged d row of the centres
constexpr int EP = TP + 1;                // pitch of the epilogue's candidates of a point
constexpr int STAGE = KC * CP + TP * XP;  // dwords of LDS
static_assert(TP == 64 && KC == 32, "index arithmetic below");
static_assert(2 * TP * EP <= STAGE, "the candidates reuse the staging area");

typedef float f32x16 __attribute__((ext_vector_type(16)));

// v_mfma_f32_32x32x2_f32: D = A (32 x 2) B (2 x 32) + C. Lane l holds A[l % 32][l / 32] and
// B[l / 32][l % 32]; D[(i & 3) + 8 (i >> 2) + 4 (l / 32)][l % 32] is element i of lane l.
__device__ __forceinline__ f32x16 mma(float a, float b, f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ int mma_row(int i, int lane) {
  return (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
}

// slab length of the update: SPECENH_KMEANS_SLAB, doubled while n needs more than 1024 slabs
long long slab_len(long long n) {
  long long L = SPECENH_KMEANS_SLAB;
  while ((n + L - 1) / L > 1024) L *= 2;
  return L;
}

// ---------------------------------------------------------------- |c_j|^2
// grid (k, batch), 64 threads: one wave per centre row
__global__ __launch_bounds__(64) void cnorm_kernel(const float* C, int d, float* cn) {
  const long long row = (long long)blockIdx.y * gridDim.x + blockIdx.x;
  const float* c = C + row * d;
  float v = 0.f;
  for (int i = threadIdx.x; i < d; i += 64) v = __builtin_fmaf(c[i], c[i], v);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  if (threadIdx.x == 0) cn[row] = v;
}

// ---------------------------------------------------------------- assignment
// (score, index) a beats b: lower score, then lower index
__device__ __forceinline__ void take_lower(float& v, int& j, float ov, int oj) {
  if (ov < v || (ov == v && oj < j)) {
    v = ov;
    j = oj;
  }
}

// grid (ceil(n / 64), batch). NBH: 32-centre blocks of a wave (a column half of the centres)
template <int NBH>
__global__ __launch_bounds__(256) void assign_kernel(const float* X, int n, int d, long long ld,
                                                     long long stride, const float* C, int k,
                                                     const float* cn, int* labels) {
  __shared__ float lds[STAGE];
  float* cs = lds;            // [KC][CP]: cs[c][j] = C[j][d0 + c]
  float* xs = lds + KC * CP;  // [TP][XP]: xs[p][c] = X[p0 + p][d0 + c]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long b = blockIdx.y;
  const int p0 = blockIdx.x * TP;  // < n < 2^31
  const float* Xb = X + b * stride;
  const float* Cb = C + b * (long long)k * d;
  const int nb = (k + 31) >> 5;      // 32-centre blocks in all
  const int pb = wave & 1;           // the wave's 32 points
  const int jb0 = (wave >> 1) * NBH; // its first block
  const int col = lane & 31, kk = lane >> 5;

  f32x16 run[NBH];
#pragma unroll
  for (int q = 0; q < NBH; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) run[q][i] = 0.f;

  for (int d0 = 0; d0 < d; d0 += KC) {
    // stage the chunk: zeros past n, k and d (exact zero products)
#pragma unroll
    for (int it = 0; it < TP * KC / 256; ++it) {
      const int idx = tid + 256 * it, p = idx >> 5, c = idx & 31;
      float v = 0.f;
      if (p < n - p0 && d0 + c < d) v = Xb[(long long)(p0 + p) * ld + d0 + c];
      xs[p * XP + c] = v;
    }
    for (int idx = tid; idx < nb * 32 * KC; idx += 256) {
      const int j = idx >> 5, c = idx & 31;
      float v = 0.f;
      if (j < k && d0 + c < d) v = Cb[(long long)j * d + d0 + c];
      cs[c * CP + j] = v;
    }
    __syncthreads();
    const int steps = d - d0 < KC ? (d - d0 + 1) >> 1 : KC / 2;  // k steps that hold data
    float a[KC / 2];
#pragma unroll
    for (int s = 0; s < KC / 2; ++s) a[s] = xs[(pb * 32 + col) * XP + 2 * s + kk];
#pragma unroll
    for (int q = 0; q < NBH; ++q) {
      if (jb0 + q < nb) {  // wave-uniform
        f32x16 t;
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = 0.f;
        const float* bq = cs + kk * CP + (jb0 + q) * 32 + col;
#pragma unroll
        for (int s = 0; s < KC / 2; ++s)
          if (s < steps) t = mma(a[s], bq[2 * s * CP], t);
#pragma unroll
        for (int i = 0; i < 16; ++i) run[q][i] = run[q][i] + t[i];
      }
    }
    __syncthreads();
  }

  // scores and the lane's own candidates: column `col` of each of its blocks, ascending
  float* ev = lds;                                         // [TP][EP]
  int* ej = reinterpret_cast<int*>(lds) + TP * EP;         // [TP][EP]
  float cnj[NBH];
#pragma unroll
  for (int q = 0; q < NBH; ++q) {
    const int j = (jb0 + q) * 32 + col;
    cnj[q] = j < k ? cn[b * k + j] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float best = INFINITY;
    int bj = INT_MAX;
#pragma unroll
    for (int q = 0; q < NBH; ++q) {
      const int j = (jb0 + q) * 32 + col;
      if (j < k) take_lower(best, bj, __builtin_fmaf(-2.f, run[q][i], cnj[q]), j);
    }
    const int e = (pb * 32 + mma_row(i, lane)) * EP + (wave >> 1) * 32 + col;
    ev[e] = best;
    ej[e] = bj;
  }
  __syncthreads();
  // four threads a point, 16 candidates each
  const int p = tid >> 2, part = tid & 3;
  float best = INFINITY;
  int bj = INT_MAX;
#pragma unroll
  for (int c = 0; c < 16; ++c)
    take_lower(best, bj, ev[p * EP + part * 16 + c], ej[p * EP + part * 16 + c]);
#pragma unroll
  for (int m = 1; m <= 2; m <<= 1) {
    const float ov = __shfl_xor(best, m);
    const int oj = __shfl_xor(bj, m);
    take_lower(best, bj, ov, oj);
  }
  // no finite score (overflow, NaN): label 0
  if (part == 0 && p < n - p0) labels[b * n + p0 + p] = bj == INT_MAX ? 0 : bj;
}

// ---------------------------------------------------------------- update: slab partials
struct UpdateArgs {
  const float* X;
  const float* C;
  const int* labels;
  float* psum;    // [batch][S][k][d]
  int* pcount;    // [batch][S][k]
  float* pinert;  // [batch][S][DB]
  long long ld, stride;
  int n, d, k;
  int L, S, DB;   // slab length, slabs, 32-column blocks of d
};

// grid (ceil(S DB / 4), batch): wave u of the grid is slab u / DB, column block u % DB
template <int NB>
__global__ __launch_bounds__(256) void update_kernel(UpdateArgs p) {
  __shared__ int hist[4][MAXK];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long b = blockIdx.y;
  const int u = blockIdx.x * 4 + wave;
  const bool active = u < p.S * p.DB;
  const int slab = u / p.DB, dblk = u - slab * p.DB;
  const int n0 = active ? slab * p.L : 0;  // S L < n + L: no overflow for an active wave
  const int len = active ? (p.n - n0 < p.L ? p.n - n0 : p.L) : 0;  // n0 + r < n for r < len
  const int* lab_b = p.labels + b * p.n + n0;

  // counts of the slab: the waves of column block 0
  const bool counting = active && dblk == 0;
  for (int j = lane; j < MAXK; j += 64) hist[wave][j] = 0;
  __syncthreads();
  if (counting)
    for (int q = lane; q < len; q += 64) {
      const int l = lab_b[q];
      if (l >= 0 && l < p.k) atomicAdd(&hist[wave][l], 1);
    }
  __syncthreads();
  if (counting)
    for (int j = lane; j < p.k; j += 64) p.pcount[(b * p.S + slab) * p.k + j] = hist[wave][j];
  if (!active) return;

  const int col = lane & 31, kk = lane >> 5;
  const int dd = dblk * 32 + col;
  const bool dvalid = dd < p.d;
  const float* Xb = p.X + b * p.stride + (long long)n0 * p.ld + dd;
  const float* Cb = p.C + b * (long long)p.k * p.d + dd;
  f32x16 acc[NB];
#pragma unroll
  for (int q = 0; q < NB; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
  float inert = 0.f;
#pragma unroll 4
  for (int q0 = 0; q0 < len; q0 += 2) {
    const int pt = q0 + kk;  // within the slab
    int l = -1;
    float x = 0.f;
    if (pt < len) {
      l = lab_b[pt];
      l = l < 0 ? 0 : (l >= p.k ? p.k - 1 : l);  // a label is an index whatever the caller wrote
      if (dvalid) {
        x = Xb[(long long)pt * p.ld];
        const float e = x - Cb[(long long)l * p.d];
        inert = __builtin_fmaf(e, e, inert);
      }
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) acc[q] = mma(l == q * 32 + col ? 1.f : 0.f, x, acc[q]);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) inert = inert + __shfl_xor(inert, m);
  if (lane == 0) p.pinert[(b * p.S + slab) * p.DB + dblk] = inert;
  if (!dvalid) return;
  float* out = p.psum + ((b * p.S + slab) * p.k) * (long long)p.d + dd;
#pragma unroll
  for (int q = 0; q < NB; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = q * 32 + mma_row(i, lane);
      if (j < p.k) out[(long long)j * p.d] = acc[q][i];
    }
}

// grid (batch), 256 threads: counts[b][j] and inertia[b] from the slab partials
__global__ __launch_bounds__(256) void reduce_kernel(const int* pcount, const float* pinert,
                                                     int S, int DB, int k, int* counts,
                                                     float* inertia) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
  const long long b = blockIdx.x;
  if (tid < k) {
    int c = 0;
    for (int s = 0; s < S; ++s) c += pcount[(b * S + s) * k + tid];
    counts[b * k + tid] = c;
  }
  const long long np = (long long)S * DB;
  const float* pi = pinert + b * np;
  float v = 0.f;
  for (long long i = tid; i < np; i += 256) v = v + pi[i];
  red[tid] = v;
  __syncthreads();
  for (int m = 128; m >= 1; m >>= 1) {
    if (tid < m) red[tid] = red[tid] + red[tid + m];
    __syncthreads();
  }
  if (tid == 0) inertia[b] = red[0];
}

// grid (ceil(k d / 256), batch): the slab sums in slab order, one division
__global__ __launch_bounds__(256) void finalize_kernel(const float* psum, const int* counts,
                                                       const float* C, int S, int k, int d,
                                                       float* Cn) {
  const long long b = blockIdx.y, kd = (long long)k * d;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= kd) return;
  const float* ps = psum + b * S * kd + e;
  float v = ps[0];
  for (int s = 1; s < S; ++s) v = v + ps[s * kd];
  const int cnt = counts[b * k + e / d];
  Cn[b * kd + e] = cnt > 0 ? __fdiv_rn(v, (float)cnt) : C[b * kd + e];
}

// ---------------------------------------------------------------- host side
struct Plan {
  int L, S, DB;
  size_t off_pcount, off_pinert, off_psum, bytes;
};

size_t round256(size_t x) { return (x + 255) & ~(size_t)255; }

// the workspace layout; false when the sizes leave 2^62 bytes
bool make_plan(long long batch, long long n, int d, int k, Plan* pl) {
  const long long L = slab_len(n);
  pl->L = (int)L;
  pl->S = (int)((n + L - 1) / L);
  pl->DB = (d + 31) / 32;
  const unsigned __int128 lim = (unsigned __int128)1 << 62;
  const unsigned __int128 items = (unsigned __int128)batch * (pl->S > 0 ? pl->S : 1);
  if (items * k * d * 4 >= lim) return false;
  size_t o = round256((size_t)batch * k * sizeof(float));  // |c_j|^2
  pl->off_pcount = o;
  o += round256((size_t)items * k * sizeof(int));
  pl->off_pinert = o;
  o += round256((size_t)items * pl->DB * sizeof(float));
  pl->off_psum = o;
  o += round256((size_t)items * k * d * sizeof(float));
  pl->bytes = o;
  return true;
}

int check_shape(long long batch, long long n, int d, long long ld, long long stride, int k) {
  if (batch < 0 || n < 0 || d < 1 || k < 1) return set_error(SPECENH_EINVAL, "kmeans: bad shape");
  if (k > MAXK)
    return set_error(SPECENH_EUNSUPPORTED, "kmeans: k " + std::to_string(k) +
                                               " is above the limit of " + std::to_string(MAXK));
  if (d > MAXD)
    return set_error(SPECENH_EUNSUPPORTED, "kmeans: d " + std::to_string(d) +
                                               " is above the limit of " + std::to_string(MAXD));
  if (n > 0x7fffffffLL)
    return set_error(SPECENH_EUNSUPPORTED, "kmeans: n must be below 2^31");
  if (ld < d) return set_error(SPECENH_EINVAL, "kmeans: ld < d");
  if (stride / ld < n) return set_error(SPECENH_EINVAL, "kmeans: stride < n*ld");
  return SPECENH_OK;
}

int check_ws(long long batch, long long n, int d, int k, const void* ws, size_t ws_bytes,
             Plan* pl) {
  if (!make_plan(batch, n, d, k, pl))
    return set_error(SPECENH_EUNSUPPORTED, "kmeans: the workspace would exceed 2^62 bytes");
  if (!ws) return set_error(SPECENH_EINVAL, "kmeans: null workspace");
  if (ws_bytes < pl->bytes)
    return set_error(SPECENH_EINVAL, "kmeans: workspace of " + std::to_string(ws_bytes) +
                                         " bytes, " + std::to_string(pl->bytes) + " needed");
  return SPECENH_OK;
}

int launched(const char* what) {
  return hipGetLastError() == hipSuccess ? SPECENH_OK : set_error(SPECENH_EHIP, what);
}

int run_assign(const float* X, long long batch, int n, int d, long long ld, long long stride,
               const float* C, int k, int* labels, float* cn, hipStream_t st) {
  const int nb = (k + 31) / 32, tiles = (n + TP - 1) / TP;
  for (long long b0 = 0; b0 < batch; b0 += 65535) {
    const unsigned nbat = (unsigned)(batch - b0 < 65535 ? batch - b0 : 65535);
    const float* Xc = X + b0 * stride;
    const float* Cc = C + b0 * k * d;
    float* cnc = cn + b0 * k;
    int* lc = labels + b0 * n;
    SPECENH_LAUNCH(cnorm_kernel, dim3(k, nbat), dim3(64), 0, st, Cc, d, cnc);
    const dim3 grid(tiles, nbat);
    if (nb <= 2)
      SPECENH_LAUNCH(assign_kernel<1>, grid, dim3(256), 0, st, Xc, n, d, ld, stride, Cc, k, cnc, lc);
    else if (nb <= 4)
      SPECENH_LAUNCH(assign_kernel<2>, grid, dim3(256), 0, st, Xc, n, d, ld, stride, Cc, k, cnc, lc);
    else
      SPECENH_LAUNCH(assign_kernel<4>, grid, dim3(256), 0, st, Xc, n, d, ld, stride, Cc, k, cnc, lc);
  }
  return launched("kmeans assign launch");
}

int run_update(UpdateArgs p, long long batch, float* Cn, int* counts, float* inertia,
               hipStream_t st) {
  const int nb = (p.k + 31) / 32;
  const long long kd = (long long)p.k * p.d;
  const unsigned ugrid = (unsigned)(((long long)p.S * p.DB + 3) / 4);
  for (long long b0 = 0; b0 < batch; b0 += 65535) {
    const unsigned nbat = (unsigned)(batch - b0 < 65535 ? batch - b0 : 65535);
    UpdateArgs q = p;
    q.X += b0 * p.stride;
    q.C += b0 * kd;
    q.labels += b0 * p.n;
    q.psum += b0 * p.S * kd;
    q.pcount += b0 * p.S * p.k;
    q.pinert += b0 * p.S * p.DB;
    const dim3 grid(ugrid, nbat);
    if (nb <= 1) SPECENH_LAUNCH(update_kernel<1>, grid, dim3(256), 0, st, q);
    else if (nb <= 2) SPECENH_LAUNCH(update_kernel<2>, grid, dim3(256), 0, st, q);
    else if (nb <= 4) SPECENH_LAUNCH(update_kernel<4>, grid, dim3(256), 0, st, q);
    else SPECENH_LAUNCH(update_kernel<8>, grid, dim3(256), 0, st, q);
    SPECENH_LAUNCH(reduce_kernel, dim3(nbat), dim3(256), 0, st, q.pcount, q.pinert, p.S, p.DB,
                   p.k, counts + b0 * p.k, inertia + b0);
    SPECENH_LAUNCH(finalize_kernel, dim3((unsigned)((kd + 255) / 256), nbat), dim3(256), 0, st,
                   q.psum, counts + b0 * p.k, q.C, p.S, p.k, p.d, Cn + b0 * kd);
  }
  return launched("kmeans update launch");
}

}  // namespace
}  // namespace specenh

using namespace specenh;

extern "C" {

size_t specenh_kmeans_workspace_bytes(long long batch, long long n, int d, int k) {
  if (batch < 0 || n < 0 || d < 1 || k < 1 || k > MAXK || d > MAXD || n > 0x7fffffffLL) return 0;
  Plan pl;
  return make_plan(batch, n, d, k, &pl) ? pl.bytes : 0;
}

int specenh_kmeans_assign(const void* X, long long batch, long long n, int d, long long ld,
                          long long stride, const void* C, int k, void* labels, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (int e = check_shape(batch, n, d, ld, stride, k)) return e;
  if (batch == 0 || n == 0) return SPECENH_OK;
  if (!X || !C || !labels) return set_error(SPECENH_EINVAL, "kmeans: null pointer");
  Plan pl;
  if (int e = check_ws(batch, n, d, k, workspace, workspace_bytes, &pl)) return e;
  return run_assign((const float*)X, batch, (int)n, d, ld, stride, (const float*)C, k,
                    (int*)labels, (float*)workspace, (hipStream_t)stream);
}

int specenh_kmeans_step(const void* X, long long batch, long long n, int d, long long ld,
                        long long stride, const void* C, int k, void* labels, void* C_new,
                        void* counts, void* inertia, void* workspace, size_t workspace_bytes,
                        void* stream) {
  if (int e = check_shape(batch, n, d, ld, stride, k)) return e;
  if (batch == 0 || n == 0) return SPECENH_OK;
  if (!X || !C || !labels || !C_new || !counts || !inertia)
    return set_error(SPECENH_EINVAL, "kmeans: null pointer");
  Plan pl;
  if (int e = check_ws(batch, n, d, k, workspace, workspace_bytes, &pl)) return e;
  char* ws = (char*)workspace;
  hipStream_t st = (hipStream_t)stream;
  if (int e = run_assign((const float*)X, batch, (int)n, d, ld, stride, (const float*)C, k,
                         (int*)labels, (float*)ws, st))
    return e;
  UpdateArgs p{};
  p.X = (const float*)X;
  p.C = (const float*)C;
  p.labels = (const int*)labels;
  p.psum = (float*)(ws + pl.off_psum);
  p.pcount = (int*)(ws + pl.off_pcount);
  p.pinert = (float*)(ws + pl.off_pinert);
  p.ld = ld;
  p.stride = stride;
  p.n = (int)n;
  p.d = d;
  p.k = k;
  p.L = pl.L;
  p.S = pl.S;
  p.DB = pl.DB;
  return run_update(p, batch, (float*)C_new, (int*)counts, (float*)inertia, st);
}

}  // extern "C"
