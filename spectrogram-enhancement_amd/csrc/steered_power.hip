// steered_power.hip — steered-response spectra of a channel array for gfx950: the Bartlett
// (conventional), Capon (minimum-variance) and MUSIC estimators are one arithmetic shape,
//
//   q[j][n] = sum_{m < M} w[j][m] | sum_{c < C} V[j][m][c] A[a(j)][n][c] |^2,
//
// a batched small complex product followed by a weighted sum of squared moduli. Rows V are
// the frame spectra the CSM's transform kernel wrote to its workspace (Bartlett: the matrix is
// never formed, A = conj(a)) or the eigenvectors of specenh_herm_eig (Capon: w = 1 / (lambda +
// delta), the result 1 / q; MUSIC: w = 0 on the signal subspace and 1 on the rest, the result
// |a|^2 / q, a sum of squares without the |a|^2 - ... cancellation).
//
// steered_power_kernel: a wave owns 32 steering rows n of one matrix j, a workgroup four such
// tiles (128 rows); the waves of a workgroup share nothing: no LDS, no barrier. The wave keeps
// its 32 x C slice of the table in registers (one float2 per lane and k step) and walks the
// rows m in tiles of 32, ascending. With V = Vr + i Vi and A = Ar + i Ai the tile's product is
//   Re P = sum Vr Ar + (-Vi) Ai,   Im P = sum Vr Ai + Vi Ar,
// on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: two channels a step, one operand VGPR per
// lane, the sign carried by the negated operand). Each of the four real products has two 32 x
// 32 accumulators, one for the even and one for the odd k steps, added pairwise in the
// epilogue: a single chain per component is one fmaf chain of 4 KH terms, and on rows that
// nearly cancel (a MUSIC peak, a single row) its rounding was 4.1 x numpy's complex64 product,
// past the 4 x the tests allow; eight chains of KH terms halve it. Lane half h takes the
// channels [h KH, (h + 1) KH) of its row, KH the k steps of the instantiation (C / 2 rounded
// up to a multiple of 4), so a lane reads one contiguous run of a row; the k order of a value
// is 0, KH, 1, KH + 1, ... and depends on C alone. The VALU epilogue of a tile squares, weights and sums the lane's 16
// rows in ascending order in fp32, adds the two lane halves (low rows' half first) and hands
// the tile's 32 rows (SPECENH_SPECTRAL_CHUNK) to an fp64 accumulator in a register. Channels
// past C, rows past M and steering rows past K are zero operands (predicated loads, never a
// read past a row); their products are exact zeros. |a_n|^2 comes from the same registers: an
// fmaf chain over the lane's channels, the low half plus the high half.
//
// No atomics, no workspace, no allocation at launch: q[j][n] is a function of V_j, w_j, row n
// of its table, M and C only, not of count, K, the tiling or j's position.
#include <hip/hip_runtime.h>

#include <string>

#include "specenh_beamform.h"
#include "runtime.hpp"
#include "averaging.hpp"

namespace specenh {
namespace {

constexpr int CT = 256;    // threads per workgroup: four waves, four tiles of steering rows
constexpr int TILE = 32;   // rows m and steering rows n of an MFMA tile
static_assert(TILE == SPECENH_SPECTRAL_CHUNK, "a row tile is the fp32 chunk");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct SteerArgs {
  const float2* v;        // matrix j at v + j * vms, row m at + m * vrs
  const float* w;         // [count][M], or null: all ones
  const float2* a;        // [a_count][K][C]
  const double* scale_v;  // [a_count], or null
  float* out;             // [count][K]
  long long j0;           // the launch's first matrix
  long long vms, vrs;
  long long a_count, a_inner;
  long long bin_inner;    // bins > 0: matrix j is bin (j / bin_inner) % bins of a one-sided
  int bins;               //   spectrum, the inner bins count twice
  int M, C, K;
  int ntile;              // workgroups per matrix: ceil(K / 128)
  int post, conj_a;
  double scale;
};

// grid (count * ntile): the tiles of one matrix are neighbouring workgroups
template <int KH>
__global__ __launch_bounds__(CT) void steered_power_kernel(SteerArgs p) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long jl = blockIdx.x / p.ntile;
  const int n0 = ((int)(blockIdx.x - jl * p.ntile) * (CT / 64) + wave) * TILE;
  if (n0 >= p.K) return;  // wave-uniform
  const long long j = p.j0 + jl;
  const int lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5;
  const int C = p.C, M = p.M, n = n0 + col;
  const int cbase = half * KH;  // this lane's channels: cbase + s
  const long long ta = (j / p.a_inner) % p.a_count;
  // the table: B[k = c][n], this lane's KH channels of steering row n
  float br[KH], bi[KH], an = 0.f;
  {
    const float2* arow = p.a + (ta * p.K + n) * C;
#pragma unroll
    for (int s = 0; s < KH; ++s) {
      float2 z = make_float2(0.f, 0.f);
      if (n < p.K && cbase + s < C) z = arow[cbase + s];
      br[s] = z.x;
      bi[s] = p.conj_a ? -z.y : z.y;
      an = fmaf(z.y, z.y, fmaf(z.x, z.x, an));
    }
  }
  const float an_o = __shfl_xor(an, 32);
  const double a2 = (double)((half ? an_o : an) + (half ? an : an_o));  // low half + high half
  const float2* vj = p.v + j * p.vms;
  const float* wj = p.w ? p.w + j * (long long)M : nullptr;
  double q = 0.0;
  for (int m0 = 0; m0 < M; m0 += TILE) {
    // A[m][k = c]: this lane's KH channels of row m0 + col
    float ar[KH], ai[KH];
    {
      const int m = m0 + col;
      const float2* vr = vj + (long long)m * p.vrs;
#pragma unroll
      for (int s = 0; s < KH; ++s) {
        float2 z = make_float2(0.f, 0.f);
        if (m < M && cbase + s < C) z = vr[cbase + s];
        ar[s] = z.x;
        ai[s] = z.y;
      }
    }
    // eight accumulators: each of the four real products in two chains (even and odd k steps)
    f32x16 rr[2] = {}, ii[2] = {}, ri[2] = {}, ir[2] = {};
#pragma unroll
    for (int s = 0; s < KH; ++s) {
      rr[s & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[s], br[s], rr[s & 1], 0, 0, 0);
      ii[s & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(-ai[s], bi[s], ii[s & 1], 0, 0, 0);
      ri[s & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ar[s], bi[s], ri[s & 1], 0, 0, 0);
      ir[s & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ai[s], br[s], ir[s & 1], 0, 0, 0);
    }
    // the lane's 16 rows of column n, ascending; rows past M are exact zeros
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = m0 + (i & 3) + 8 * (i >> 2) + 4 * half;
      const float re = (rr[0][i] + rr[1][i]) + (ii[0][i] + ii[1][i]);
      const float im = (ri[0][i] + ri[1][i]) + (ir[0][i] + ir[1][i]);
      const float pw = fmaf(im, im, re * re);
      float wt = 1.f;
      if (wj) wt = row < M ? wj[row] : 0.f;
      t = fmaf(wt, pw, t);
    }
    const float t_o = __shfl_xor(t, 32);
    q += (double)((half ? t_o : t) + (half ? t : t_o));
  }
  if (half || n >= p.K) return;
  double s = p.scale;
  if (p.scale_v) s *= p.scale_v[ta];
  if (p.bins > 0) {
    const int f = (int)((j / p.bin_inner) % p.bins);
    if (f > 0 && f < p.bins - 1) s *= 2.0;
  }
  double r;
  switch (p.post) {
    case SPECENH_STEER_SUM: r = q * s; break;
    case SPECENH_STEER_BARTLETT: r = q * s / (a2 * a2); break;
    case SPECENH_STEER_INVERSE: r = s / q; break;
    default: r = a2 / q; break;  // SPECENH_STEER_MUSIC
  }
  p.out[j * p.K + n] = (float)r;
}

// Launches the kernel over matrices [0, count) of `p` (p.j0 is set here).
int launch_steered(SteerArgs p, long long count, hipStream_t stream) {
  p.ntile = (p.K + 4 * TILE - 1) / (4 * TILE);
  // KH = C / 2 rounded up to a multiple of 4: at most 7 channels of zero operands
  static void (*const kernels[8])(SteerArgs) = {
      steered_power_kernel<4>,  steered_power_kernel<8>,  steered_power_kernel<12>,
      steered_power_kernel<16>, steered_power_kernel<20>, steered_power_kernel<24>,
      steered_power_kernel<28>, steered_power_kernel<32>};
  void (*kernel)(SteerArgs) = kernels[(p.C - 1) / 8];
  const long long step = 2147483647LL / p.ntile;  // matrices per launch
  for (long long j0 = 0; j0 < count; j0 += step) {
    const long long nj = count - j0 < step ? count - j0 : step;
    p.j0 = j0;
    launch(kernel, dim3((unsigned)(nj * p.ntile)), dim3(CT), 0, stream, p);
    if (int rc = launched("steered_power")) return rc;
  }
  return SPECENH_OK;
}

int check_table(long long channels, long long nsteer) {
  if (channels < 1 || channels > SPECENH_STEER_MAX_CHANNELS)
    return set_error(SPECENH_EINVAL, "channels must be in [1, 64]");
  if (nsteer < 1 || nsteer > SPECENH_STEER_MAX_NSTEER)
    return set_error(SPECENH_EINVAL, "nsteer must be in [1, 4096]");
  return SPECENH_OK;
}

// the split of a fused call, or a negative error; validates everything but the pointers
int split_for(const specenh_stft_plan* plan, long long batch, long long channels,
              long long length, long long navg, FrameSplit* s) {
  if (int rc = check_call(plan, batch, length, navg, true, s)) return rc;
  if (channels < 1 || channels > SPECENH_STEER_MAX_CHANNELS)
    return set_error(SPECENH_EINVAL, "channels must be in [1, 64]");
  return SPECENH_OK;
}

}  // namespace
}  // namespace specenh

extern "C" {

int specenh_steered_power(const void* v, const float* w, const void* a, long long count,
                          long long rows, long long channels, long long nsteer,
                          long long v_matrix_stride, long long v_row_stride, long long a_count,
                          long long a_inner, int conj_a, double scale,
                          const double* scale_table, int post, float* out, void* stream) {
  using namespace specenh;
  if (!v) return set_error(SPECENH_EINVAL, "null v");
  if (!a) return set_error(SPECENH_EINVAL, "null a");
  if (reinterpret_cast<size_t>(v) % 8) return set_error(SPECENH_EINVAL, "v must be 8-byte aligned");
  if (reinterpret_cast<size_t>(a) % 8) return set_error(SPECENH_EINVAL, "a must be 8-byte aligned");
  if (count < 0) return set_error(SPECENH_EINVAL, "count must be >= 0");
  if (rows < 1) return set_error(SPECENH_EINVAL, "rows must be >= 1");
  if (rows > (1ll << 30)) return set_error(SPECENH_EINVAL, "too many rows");
  if (int rc = check_table(channels, nsteer)) return rc;
  if (v_row_stride < channels) return set_error(SPECENH_EINVAL, "v_row_stride < channels");
  if (v_matrix_stride < (rows - 1) * v_row_stride + channels)
    return set_error(SPECENH_EINVAL, "v_matrix_stride < (rows - 1) * v_row_stride + channels");
  if (a_count < 1 || a_inner < 1)
    return set_error(SPECENH_EINVAL, "a_count and a_inner must be >= 1");
  if (a_count > 1 && (a_inner > (1ll << 40) / a_count || count % (a_count * a_inner)))
    return set_error(SPECENH_EINVAL, "count must be a multiple of a_count * a_inner");
  if (post < SPECENH_STEER_SUM || post > SPECENH_STEER_MUSIC)
    return set_error(SPECENH_EINVAL, "post must be in [0, 3]");
  if (!out) return set_error(SPECENH_EINVAL, "null out");
  if (count == 0) return SPECENH_OK;
  SteerArgs p{};
  p.v = reinterpret_cast<const float2*>(v);
  p.w = w;
  p.a = reinterpret_cast<const float2*>(a);
  p.scale_v = scale_table;
  p.out = out;
  p.vms = v_matrix_stride; p.vrs = v_row_stride;
  p.a_count = a_count; p.a_inner = a_inner;
  p.bins = 0; p.bin_inner = 1;
  p.M = (int)rows; p.C = (int)channels; p.K = (int)nsteer;
  p.post = post; p.conj_a = conj_a ? 1 : 0;
  p.scale = scale;
  return launch_steered(p, count, (hipStream_t)stream);
}

size_t specenh_array_spectrum_workspace_bytes(const specenh_stft_plan* plan, long long batch,
                                              long long channels, long long length,
                                              long long navg) {
  using namespace specenh;
  FrameSplit s;
  if (split_for(plan, batch, channels, length, navg, &s) != SPECENH_OK) return 0;
  return (size_t)batch * (size_t)(plan->nperseg / 2 + 1) * (size_t)s.Tu * (size_t)channels *
         sizeof(float2);
}

int specenh_array_spectrum(const specenh_stft_plan* plan, const float* x, long long batch,
                           long long channels, long long length, long long channel_stride,
                           long long batch_stride, long long navg, const void* a,
                           long long nsteer, int a_per_bin, float* out, void* workspace,
                           size_t workspace_bytes, void* stream) {
  using namespace specenh;
  if (!x) return set_error(SPECENH_EINVAL, "null x");
  if (!a) return set_error(SPECENH_EINVAL, "null a");
  if (reinterpret_cast<size_t>(a) % 8) return set_error(SPECENH_EINVAL, "a must be 8-byte aligned");
  FrameSplit s;
  if (int rc = split_for(plan, batch, channels, length, navg, &s)) return rc;
  if (int rc = check_stride(channel_stride, length, "channel_stride < length")) return rc;
  if (batch_stride < channels * channel_stride)
    return set_error(SPECENH_EINVAL, "batch_stride < channels * channel_stride");
  if (int rc = check_table(channels, nsteer)) return rc;
  if (!out) return set_error(SPECENH_EINVAL, "null out");
  if (batch == 0) return SPECENH_OK;
  const int C = (int)channels;
  const long long F = plan->nperseg / 2 + 1;
  if (int rc = check_workspace(
          workspace, workspace_bytes,
          specenh_array_spectrum_workspace_bytes(plan, batch, channels, length, navg)))
    return rc;
  SteerArgs p{};
  p.w = nullptr;
  p.a = reinterpret_cast<const float2*>(a);
  p.scale_v = nullptr;
  // group g of row (b, f) starts g * glen * C into it and Tu = G * glen: matrix j = (b, f, g)
  // starts j * glen * C into the workspace
  p.vms = s.glen * C; p.vrs = C;
  p.a_count = a_per_bin ? F : 1; p.a_inner = s.G;
  p.bins = (int)F; p.bin_inner = s.G;
  p.M = (int)s.glen; p.C = C; p.K = (int)nsteer;
  p.post = SPECENH_STEER_BARTLETT; p.conj_a = 1;
  p.scale = plan->scale / (4.0 * (double)s.glen);  // the rows are 2 X: the Gram kernel's m
  const long long step = 65535;  // shots per launch: grid.z of the transform
  const long long ws_shot = F * s.Tu * C, out_shot = F * s.G * nsteer;
  for (long long b0 = 0; b0 < batch; b0 += step) {
    const long long nb = batch - b0 < step ? batch - b0 : step;
    float2* ws = reinterpret_cast<float2*>(workspace) + b0 * ws_shot;
    if (int rc = csm_transform(plan, x + b0 * batch_stride, nb, C, channel_stride, batch_stride,
                               s.Tu, ws, (hipStream_t)stream))
      return rc;
    p.v = ws;
    p.out = out + b0 * out_shot;
    if (int rc = launch_steered(p, nb * F * s.G, (hipStream_t)stream)) return rc;
  }
  return SPECENH_OK;
}

}  // extern "C"
