// nlmeans.hip — non-local means denoising (skimage.restoration.denoise_nl_means, fast_mode
// weighting, no cutoff) on the GPU. include/specenh_nlmeans.h has the arithmetic and the error
// criterion; tests/nlmeans_local.py the numpy restatement.
//
// One workgroup of 256 threads per TR x TC output tile of one image. The tile and a halo of
// D + f on every side are loaded once into LDS as fp32 with reflection applied on load; the
// shift loop touches no global memory. A thread owns RUN vertically neighbouring pixels of one
// column: a wave is 64 neighbouring columns, so every LDS read is 64 consecutive dwords. The
// (RUN + P - 1) x P values under the thread's own patches stay in registers for the whole
// loop. Per shift the thread reads the same block at the shifted position, forms the squared
// differences, sums each of the RUN + P - 1 rows over its P columns, and each pixel adds the P
// row sums of its patch: the row sums are shared by the pixels of the run, nothing is shared
// between threads, and the loop has no barrier.
//
// All window sums add non-negative terms only (no sliding subtraction), every pixel runs the
// same sequence of operations whatever its place in the run, the tile or the batch, and the
// two accumulations are one fp32 chain each in shift order.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <string>

#include "specenh_nlmeans.h"
#include "filters_u8.hpp"
#include "runtime.hpp"

namespace specenh {

namespace {

constexpr int TR = SPECENH_NLMEANS_TILE_ROWS;
constexpr int TC = SPECENH_NLMEANS_TILE_COLS;
constexpr int MAXP = SPECENH_NLMEANS_MAX_PATCH;
constexpr int MAXD = SPECENH_NLMEANS_MAX_DISTANCE;
constexpr int MAXH = MAXD + MAXP / 2;   // the halo at the limits
constexpr int MAX_DIM = (1 << 30) - 1;  // rows, cols: 2 n and n + tile + halo fit an int
constexpr int PITCH = TC + 2 * MAXH;    // dwords of a tile row
constexpr int TILE_ROWS = TR + 2 * MAXH;
constexpr int RUN = TR * TC / 256;      // pixels of a thread: a vertical run of one column
static_assert(TC == 64, "a wave is one row of 64 neighbouring columns");
static_assert(RUN * 256 == TR * TC && RUN * 4 == TR, "four waves, RUN rows each");

template <typename T, int P>
__global__ __launch_bounds__(256) void nlmeans_kernel(const T* S, int rows, int cols,
                                                      long long stride, int tiles_x, int D,
                                                      float scale, float sig, T* out) {
  constexpr int F = P / 2, WR = RUN + P - 1;
  __shared__ float tile[TILE_ROWS * PITCH];
  const int tid = threadIdx.x, H = D + F;
  const long long b = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const T* src = S + b * stride;

  // Tile with halo. A pixel past the image's last row or column by more than the halo feeds
  // only outputs that are not stored: it is left at 0, which also bounds reflect101's loop.
  const int r0 = ty * TR - H, c0 = tx * TC - H;
  const int th = TR + 2 * H, tw = TC + 2 * H;
  for (int idx = tid; idx < th * tw; idx += 256) {
    const int y = idx / tw, x = idx - y * tw;
    const int r = r0 + y, c = c0 + x;
    float v = 0.f;
    if (r < rows + H && c < cols + H)
      v = (float)src[(long long)reflect101(r, rows) * cols + reflect101(c, cols)];
    tile[y * PITCH + x] = v;
  }
  __syncthreads();

  // tile (y, x) is the image's (r0 + y, c0 + x). The thread's pixels are the tile's output
  // rows RUN*rg .. RUN*rg + RUN - 1 of output column col; the block under their patches
  // begins at tile (D + RUN*rg, D + col), the block of shift (i - D, j - D) at (i + RUN*rg,
  // j + col): both stay inside th x tw.
  const int rg = tid >> 6, col = tid & 63;
  const float* own = tile + (D + RUN * rg) * PITCH + D + col;
  float cv[WR][P];
#pragma unroll
  for (int k = 0; k < WR; ++k)
#pragma unroll
    for (int j = 0; j < P; ++j) cv[k][j] = own[k * PITCH + j];

  float sum_w[RUN], sum_wv[RUN], res[RUN];
#pragma unroll
  for (int p = 0; p < RUN; ++p) {
    sum_w[p] = 0.f;
    sum_wv[p] = 0.f;
  }
  const int side = 2 * D + 1;
  for (int i = 0; i < side; ++i) {
    // one tile index per pair of block rows, stepped with j: an LDS read's two immediate
    // offsets reach 255 dwords, two rows of the pitch, so no address is formed per read
    int pair[(WR + 1) / 2];
#pragma unroll
    for (int g = 0; g < (WR + 1) / 2; ++g) pair[g] = (i + RUN * rg + 2 * g) * PITCH + col;
    for (int j = 0; j < side; ++j) {
#pragma clang fp contract(off)
      float hs[WR], v[RUN];
#pragma unroll
      for (int k = 0; k < WR; ++k) {
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < P; ++m) {
          const float u = tile[pair[k / 2] + (k % 2) * PITCH + m];
          const float e = cv[k][m] - u;
          s = m == 0 ? e * e : __builtin_fmaf(e, e, s);
          if (m == F && k >= F && k < F + RUN) v[k - F] = u;
        }
        hs[k] = s;
      }
#pragma unroll
      for (int p = 0; p < RUN; ++p) {
        float d2 = hs[p];
#pragma unroll
        for (int m = 1; m < P; ++m) d2 = d2 + hs[p + m];
        const float x = fmaxf(__builtin_fmaf(d2, scale, -sig), 0.f);
        const float w = __builtin_amdgcn_exp2f(-x);
        sum_w[p] = sum_w[p] + w;
        sum_wv[p] = __builtin_fmaf(w, v[p], sum_wv[p]);
      }
#pragma unroll
      for (int g = 0; g < (WR + 1) / 2; ++g) ++pair[g];
    }
  }
#pragma unroll
  for (int p = 0; p < RUN; ++p)  // D = 0: the only weight is 1; the input's bits, -0 included
    res[p] = D == 0 ? cv[p + F][F] : __fdiv_rn(sum_wv[p], sum_w[p]);

  const int c = tx * TC + col;
  if (c >= cols) return;
  T* o = out + b * stride + c;
#pragma unroll
  for (int p = 0; p < RUN; ++p) {
    const int r = ty * TR + RUN * rg + p;
    if (r < rows) o[(long long)r * cols] = (T)res[p];
  }
}

template <typename T, int P>
void launch_nlmeans(const T* S, long long batch, int rows, int cols, long long stride,
                    long long tiles, int tiles_x, int D, float scale, float sig, T* out,
                    hipStream_t st) {
  for (long long b0 = 0; b0 < batch; b0 += 65535) {
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    SPECENH_LAUNCH((nlmeans_kernel<T, P>), dim3((unsigned)tiles, (unsigned)nb), dim3(256), 0, st,
                   S + b0 * stride, rows, cols, stride, tiles_x, D, scale, sig,
                   out + b0 * stride);
  }
}

template <typename T>
int run_nlmeans(const T* S, long long batch, int rows, int cols, long long stride,
                long long tiles, int tiles_x, int P, int D, float scale, float sig, T* out,
                hipStream_t st) {
  switch (P) {
    case 1: launch_nlmeans<T, 1>(S, batch, rows, cols, stride, tiles, tiles_x, D, scale, sig, out, st); break;
    case 3: launch_nlmeans<T, 3>(S, batch, rows, cols, stride, tiles, tiles_x, D, scale, sig, out, st); break;
    case 5: launch_nlmeans<T, 5>(S, batch, rows, cols, stride, tiles, tiles_x, D, scale, sig, out, st); break;
    case 7: launch_nlmeans<T, 7>(S, batch, rows, cols, stride, tiles, tiles_x, D, scale, sig, out, st); break;
    default: launch_nlmeans<T, 9>(S, batch, rows, cols, stride, tiles, tiles_x, D, scale, sig, out, st); break;
  }
  return hipGetLastError() == hipSuccess ? SPECENH_OK : set_error(SPECENH_EHIP, "nlmeans launch");
}

// a positive double as a float, kept finite so that 0 * scale stays 0
float finite_float(double x) { return x > FLT_MAX ? FLT_MAX : (float)x; }

}  // namespace
}  // namespace specenh

using namespace specenh;

extern "C" {

int specenh_nlmeans(int dtype, const void* S, long long batch, int rows, int cols,
                    long long stride, int patch_size, int patch_distance, double h, double sigma,
                    void* out, void* stream) {
  if (int e = check_common(dtype, S, batch, rows, cols, stride, out)) return e;
  if (patch_size < 1 || patch_size % 2 == 0)
    return set_error(SPECENH_EINVAL, "nlmeans: patch_size must be odd and positive");
  if (patch_distance < 0)
    return set_error(SPECENH_EINVAL, "nlmeans: patch_distance must not be negative");
  if (!std::isfinite(h) || h <= 0)
    return set_error(SPECENH_EINVAL, "nlmeans: h must be finite and positive");
  if (!std::isfinite(sigma) || sigma < 0)
    return set_error(SPECENH_EINVAL, "nlmeans: sigma must be finite and not negative");
  if (patch_size > MAXP)
    return set_error(SPECENH_EUNSUPPORTED, "nlmeans: patch_size " + std::to_string(patch_size) +
                                               " is above the limit of " + std::to_string(MAXP));
  if (patch_distance > MAXD)
    return set_error(SPECENH_EUNSUPPORTED,
                     "nlmeans: patch_distance " + std::to_string(patch_distance) +
                         " is above the limit of " + std::to_string(MAXD));
  // tile and halo coordinates and the reflection (2 n - 2 - p) are int arithmetic
  if (rows > MAX_DIM || cols > MAX_DIM)
    return set_error(SPECENH_EUNSUPPORTED, "nlmeans: rows and cols must be below 2^30");
  const int tiles_x = (cols + TC - 1) / TC;
  const long long tiles = (long long)((rows + TR - 1) / TR) * tiles_x;
  if (tiles > 0x7fffffffLL)
    return set_error(SPECENH_EUNSUPPORTED, "nlmeans: the image has more than 2^31 - 1 tiles");
  if (batch == 0) return SPECENH_OK;
  // exp(-a) = exp2(-(sum e^2) log2(e) / (P^2 h^2) + 2 sigma^2 log2(e) / h^2), floored at 0
  const double log2e = 1.4426950408889634074, h2 = h * h;
  const float scale = finite_float(log2e / ((double)patch_size * patch_size * h2));
  const float sig = finite_float(2.0 * sigma * sigma * log2e / h2);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SPECENH_DTYPE_F64)
    return run_nlmeans<double>((const double*)S, batch, rows, cols, stride, tiles, tiles_x,
                               patch_size, patch_distance, scale, sig, (double*)out, st);
  return run_nlmeans<float>((const float*)S, batch, rows, cols, stride, tiles, tiles_x,
                            patch_size, patch_distance, scale, sig, (float*)out, st);
}

}  // extern "C"
