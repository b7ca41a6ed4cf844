// filters_u8.hpp — what the uint8 label filters share (filters.hip: gaussblr, morph;
// bilateral.hip: bilateral): the argument checks of every label filter, the quantisation
// (rescale(src)*255).astype('uint8') of a batch, the rescale of a uint8 batch as numpy
// evaluates it, and OpenCV's BORDER_REFLECT_101. The kernels live in filters.hip.
#pragma once

#include <hip/hip_runtime.h>

namespace specenh {

// dtype f32/f64, batch >= 0, rows/cols >= 1, stride >= rows*cols, non-null S/out when batch > 0
int check_common(int dtype, const void* S, long long batch, int rows, int cols, long long stride,
                 const void* out);

// BORDER_REFLECT_101, applied as often as needed; a dimension of 1 maps to index 0
__device__ __forceinline__ int reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) {
    if (p < 0) p = -p;
    if (p >= n) p = 2 * n - 2 - p;
  }
  return p;
}

// {min, max} of every spectrogram into stats[2 * batch], then q[batch][rows][cols] =
// (T)((S - min) / (max - min)) * 255 truncated to uint8 (two launches). T = float or double.
template <typename T>
void launch_quant_u8(const T* S, long long batch, int rows, int cols, long long stride,
                     double* stats, unsigned char* q, hipStream_t st);

// {min, max} of every uint8 image into stats, then out = (u - min) / (max - min) as a true
// (fp64) division rounded to T (two launches); a constant image gives 0/0 = NaN
template <typename T>
void launch_rescale_u8(const unsigned char* u, long long batch, int rows, int cols,
                       long long stride, double* stats, T* out, hipStream_t st);

}  // namespace specenh
