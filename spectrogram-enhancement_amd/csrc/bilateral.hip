// bilateral.hip — the bilateral label filter of spec_denoising/dataset.ipynb (bilateral(src):
// uint8 quantisation, cv2.bilateralFilter(u8, 15, 75, 75), rescale) on the GPU. OpenCV is
// absent, so its 8-bit one-channel algorithm is restated (include/specenh_bilateral.h has the
// arithmetic; tests/bilateral_local.py the numpy restatement).
//
// One workgroup of 256 threads per TR x TC output tile of one image. The tile and a halo of
// `radius` bytes on every side are loaded once into LDS with BORDER_REFLECT_101 applied on
// load; no tap touches global memory. A thread owns four neighbouring pixels of one row: a
// tap's four bytes are one unaligned dword of the tile, assembled from two aligned LDS reads,
// and its space weight and tile offset are one wave-uniform LDS read. What is left per tap and
// pixel is the gather cw[|v - v0|]. The 256-entry colour table is replicated 32 times,
// entry t of lane l at dword 32 t + (l mod 32): a ds_read_b32 is served in two groups of 32
// lanes over 32 banks, so every lane of a group has a bank of its own and the gather never
// serialises, whatever the image holds.
//
// Every pixel runs the same accumulation code whatever tile it falls in: w_k is one fp32
// product, sum w_k and sum v_k w_k are one fp32 chain each in tap order, one division, round
// half to even.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "specenh_bilateral.h"
#include "filters_u8.hpp"
#include "runtime.hpp"

namespace specenh {

namespace {

constexpr int TR = SPECENH_BILATERAL_TILE_ROWS;
constexpr int TC = SPECENH_BILATERAL_TILE_COLS;
constexpr int MAXR = SPECENH_BILATERAL_MAX_RADIUS;
constexpr int SIDE = 2 * MAXR + 1;
constexpr int MAX_TAPS = 709;  // the disc of radius 15
// a tile row: TC + 2 radius bytes and the dword a thread's second read may reach into
constexpr int PITCH = (TC + 2 * MAXR + 4 + 3) / 4 * 4;
constexpr int TILE_BYTES = (TR + 2 * MAXR) * PITCH;
constexpr int CW_REP = 32;  // copies of the colour table: one per bank of a ds_read_b32
static_assert(TR * (TC / 4) == 256, "one thread per four pixels of a tile row");
static_assert(TC / 4 == 32, "a lane group of 32 reads 32 consecutive dwords of one tile row");

// The tables of one call, built on the host; kernel arguments (2 KiB).
struct BilateralTables {
  float cw[256];                      // colour weight of |v - v0|
  float sw[MAXR * MAXR + 1];          // space weight of i^2 + j^2
  unsigned short row_start[SIDE];     // index of the first tap of tap row i + radius
  unsigned char half[SIDE];           // taps of that row: j = -half .. half
  int radius, taps;
};

struct Tap {
  float w;  // space weight
  int off;  // (i + radius) * PITCH + (j + radius)
};

__global__ __launch_bounds__(256) void bilateral_u8_kernel(const unsigned char* img, int rows,
                                                           int cols, long long stride,
                                                           int tiles_x, BilateralTables tb,
                                                           unsigned char* out) {
  __shared__ float cw[256 * CW_REP];
  __shared__ __attribute__((aligned(8))) Tap taps[MAX_TAPS];
  __shared__ __attribute__((aligned(16))) unsigned char tile[TILE_BYTES];
  const int R = tb.radius, tid = threadIdx.x;
  const long long b = blockIdx.y;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const unsigned char* src = img + b * stride;

  for (int idx = tid; idx < 256 * CW_REP; idx += 256) cw[idx] = tb.cw[idx / CW_REP];
  const int side = 2 * R + 1;
  for (int idx = tid; idx < side * side; idx += 256) {
    const int ii = idx / side, i = ii - R, j = idx - ii * side - R;
    const int h = tb.half[ii];
    if (j >= -h && j <= h) taps[tb.row_start[ii] + j + h] = Tap{tb.sw[i * i + j * j], ii * PITCH + j + R};
  }
  // Tile with halo. A pixel past the image's last row or column by more than the radius feeds
  // only outputs that are not stored: it is left at 0, which also bounds reflect101's loop.
  const int r0 = ty * TR - R, c0 = tx * TC - R;
  const int th = TR + 2 * R, tw = TC + 2 * R;
  for (int idx = tid; idx < th * tw; idx += 256) {
    const int y = idx / tw, x = idx - y * tw;
    const int r = r0 + y, c = c0 + x;
    unsigned char v = 0;
    if (r < rows + R && c < cols + R)
      v = src[(long long)reflect101(r, rows) * cols + reflect101(c, cols)];
    tile[y * PITCH + x] = v;
  }
  __syncthreads();

  const int row = tid >> 5, cg = tid & 31;
  const int base = row * PITCH + 4 * cg;  // a multiple of 4: the shift below is wave-uniform
  const unsigned* t32 = reinterpret_cast<const unsigned*>(tile);
  const float* cwl = cw + (tid & (CW_REP - 1));
  int v0[4];
  {
    const int ad = base + R * PITCH + R;
    const unsigned px = __builtin_amdgcn_alignbyte(t32[(ad >> 2) + 1], t32[ad >> 2], ad & 3);
#pragma unroll
    for (int p = 0; p < 4; ++p) v0[p] = (int)((px >> (8 * p)) & 255u);
  }
  float sum_w[4] = {0.f, 0.f, 0.f, 0.f}, sum_vw[4] = {0.f, 0.f, 0.f, 0.f};
  const int n = tb.taps;
  // w is rounded before it enters either sum: the compiler must not fold the product into
  // the addition of sum_w; the multiply-add of sum_vw is asked for by name
  for (int k = 0; k < n; ++k) {
#pragma clang fp contract(off)
    const Tap t = taps[k];
    const int ad = base + t.off;
    const unsigned px = __builtin_amdgcn_alignbyte(t32[(ad >> 2) + 1], t32[ad >> 2], ad & 3);
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int v = (int)((px >> (8 * p)) & 255u);
      const int dv = v > v0[p] ? v - v0[p] : v0[p] - v;
      const float w = t.w * cwl[dv * CW_REP];
      sum_w[p] = sum_w[p] + w;
      sum_vw[p] = __builtin_fmaf((float)v, w, sum_vw[p]);
    }
  }
  const int r = ty * TR + row, c = tx * TC + 4 * cg;
  if (r >= rows) return;
  unsigned char* o = out + b * ((long long)rows * cols) + (long long)r * cols + c;
#pragma unroll
  for (int p = 0; p < 4; ++p)
    if (c + p < cols) o[p] = (unsigned char)__float2int_rn(__fdiv_rn(sum_vw[p], sum_w[p]));
}

// cv2's radius from (d, sigma_space); sigma_space already made positive
int bilateral_radius(int d, double sigma_space, int* radius) {
  double r = d <= 0 ? std::nearbyint(1.5 * sigma_space) : (double)(d / 2);
  if (r < 1.0) r = 1.0;
  if (r > MAXR)
    return set_error(SPECENH_EUNSUPPORTED,
                     "bilateral: radius " + std::to_string((long long)std::fmin(r, 1e18)) +
                         " is above the limit of " + std::to_string(MAXR) +
                         " (d <= 31, or sigma_space <= 10 for d <= 0)");
  *radius = (int)r;
  return SPECENH_OK;
}

int bilateral_tables(int d, double sigma_color, double sigma_space, BilateralTables* tb) {
  if (!std::isfinite(sigma_color) || !std::isfinite(sigma_space))
    return set_error(SPECENH_EINVAL, "bilateral: sigma_color and sigma_space must be finite");
  if (sigma_color <= 0) sigma_color = 1;
  if (sigma_space <= 0) sigma_space = 1;
  int R;
  if (int e = bilateral_radius(d, sigma_space, &R)) return e;
  const double gc = -0.5 / (sigma_color * sigma_color), gs = -0.5 / (sigma_space * sigma_space);
  for (int t = 0; t < 256; ++t) tb->cw[t] = (float)std::exp((double)t * t * gc);
  for (int q = 0; q <= MAXR * MAXR; ++q) tb->sw[q] = q <= R * R ? (float)std::exp(q * gs) : 0.f;
  int n = 0;
  for (int ii = 0; ii < SIDE; ++ii) {
    const int i = ii - R;
    int h = 0;
    if (ii <= 2 * R)
      while ((h + 1) * (h + 1) + i * i <= R * R) ++h;
    tb->row_start[ii] = (unsigned short)n;
    tb->half[ii] = (unsigned char)h;
    if (ii <= 2 * R) n += 2 * h + 1;
  }
  tb->radius = R;
  tb->taps = n;
  return SPECENH_OK;
}

int check_u8(const void* img, long long batch, int rows, int cols, long long stride,
             const void* out) {
  if (batch < 0 || rows <= 0 || cols <= 0) return set_error(SPECENH_EINVAL, "bad shape");
  if (stride < (long long)rows * cols) return set_error(SPECENH_EINVAL, "stride < rows*cols");
  if (batch > 0 && (!img || !out)) return set_error(SPECENH_EINVAL, "null pointer");
  return SPECENH_OK;
}

int check_tiles(int rows, int cols, long long* tiles, int* tiles_x) {
  *tiles_x = (cols + TC - 1) / TC;
  *tiles = (long long)((rows + TR - 1) / TR) * *tiles_x;
  if (*tiles > 0x7fffffffLL)
    return set_error(SPECENH_EUNSUPPORTED, "bilateral: the image has more than 2^31 - 1 tiles");
  return SPECENH_OK;
}

void launch_bilateral(const unsigned char* img, long long batch, int rows, int cols,
                      long long stride, const BilateralTables& tb, long long tiles, int tiles_x,
                      unsigned char* out, hipStream_t st) {
  const long long n = (long long)rows * cols;
  for (long long b0 = 0; b0 < batch; b0 += 65535) {
    const long long nb = batch - b0 < 65535 ? batch - b0 : 65535;
    SPECENH_LAUNCH(bilateral_u8_kernel, dim3((unsigned)tiles, (unsigned)nb), dim3(256), 0, st,
                   img + b0 * stride, rows, cols, stride, tiles_x, tb, out + b0 * n);
  }
}

inline size_t round256(size_t n) { return (n + 255) / 256 * 256; }

template <typename T>
int run_bilateral(const T* S, long long batch, int rows, int cols, long long stride,
                  const BilateralTables& tb, long long tiles, int tiles_x, T* out, void* ws,
                  hipStream_t st) {
  const size_t n = (size_t)batch * rows * cols;
  double* stats = (double*)ws;
  unsigned char* a = (unsigned char*)ws + round256((size_t)batch * 16);
  unsigned char* f = a + round256(n);
  launch_quant_u8<T>(S, batch, rows, cols, stride, stats, a, st);
  launch_bilateral(a, batch, rows, cols, (long long)rows * cols, tb, tiles, tiles_x, f, st);
  launch_rescale_u8<T>(f, batch, rows, cols, stride, stats, out, st);
  return hipGetLastError() == hipSuccess ? SPECENH_OK
                                         : set_error(SPECENH_EHIP, "bilateral launch");
}

}  // namespace
}  // namespace specenh

using namespace specenh;

extern "C" {

int specenh_bilateral_taps(int d, double sigma_space, int* radius, int* taps) {
  BilateralTables tb;
  if (int e = bilateral_tables(d, 1.0, sigma_space, &tb)) return e;
  if (radius) *radius = tb.radius;
  if (taps) *taps = tb.taps;
  return SPECENH_OK;
}

int specenh_bilateral_u8(const unsigned char* img, long long batch, int rows, int cols,
                         long long stride, int d, double sigma_color, double sigma_space,
                         unsigned char* out, void* stream) {
  if (int e = check_u8(img, batch, rows, cols, stride, out)) return e;
  BilateralTables tb;
  if (int e = bilateral_tables(d, sigma_color, sigma_space, &tb)) return e;
  long long tiles;
  int tiles_x;
  if (int e = check_tiles(rows, cols, &tiles, &tiles_x)) return e;
  if (batch == 0) return SPECENH_OK;
  launch_bilateral(img, batch, rows, cols, stride, tb, tiles, tiles_x, out, (hipStream_t)stream);
  return hipGetLastError() == hipSuccess ? SPECENH_OK
                                         : set_error(SPECENH_EHIP, "bilateral launch");
}

size_t specenh_bilateral_workspace_bytes(long long batch, int rows, int cols) {
  if (batch <= 0 || rows <= 0 || cols <= 0) return 16;
  const size_t n = (size_t)batch * rows * cols;
  return round256((size_t)batch * 16) + 2 * round256(n);
}

int specenh_bilateral(int dtype, const void* S, long long batch, int rows, int cols,
                      long long stride, int d, double sigma_color, double sigma_space,
                      void* out, void* workspace, void* stream) {
  if (int e = check_common(dtype, S, batch, rows, cols, stride, out)) return e;
  BilateralTables tb;
  if (int e = bilateral_tables(d, sigma_color, sigma_space, &tb)) return e;
  long long tiles;
  int tiles_x;
  if (int e = check_tiles(rows, cols, &tiles, &tiles_x)) return e;
  if (batch == 0) return SPECENH_OK;
  if (!workspace) return set_error(SPECENH_EINVAL, "null workspace");
  if ((size_t)workspace % 16) return set_error(SPECENH_EINVAL, "workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (dtype == SPECENH_DTYPE_F64)
    return run_bilateral<double>((const double*)S, batch, rows, cols, stride, tb, tiles, tiles_x,
                                 (double*)out, workspace, st);
  return run_bilateral<float>((const float*)S, batch, rows, cols, stride, tb, tiles, tiles_x,
                              (float*)out, workspace, st);
}

}  // extern "C"
