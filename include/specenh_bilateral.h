/* specenh_bilateral.h — the bilateral label filter of libspecenh.so, an extension of the
 * C-ABI in specenh.h (same error codes and dtype codes) beside the label filters declared
 * there (specenh_gaussblr, specenh_morph). */
#ifndef SPECENH_BILATERAL_H
#define SPECENH_BILATERAL_H

#include <stddef.h>

#include "specenh.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- bilateral filter
 * spec_denoising/dataset.ipynb, bilateral(src):
 *     src = (rescale(src)*255).astype('uint8'); out = cv2.bilateralFilter(src, 15, 75, 75)
 *     return rescale(out)
 * OpenCV's 8-bit, one-channel algorithm restated (BORDER_REFLECT_101):
 *   sigma_color <= 0 and sigma_space <= 0 become 1;
 *   radius = d <= 0 ? cvRound(1.5 sigma_space) : d / 2, at least 1 (cvRound: half to even);
 *   taps: every (i, j) in [-radius, radius]^2 with i^2 + j^2 <= radius^2, row-major in (i, j),
 *         the centre included: 149 for radius 7;
 *   sw[k] = (float)exp(-0.5 (i^2 + j^2) / sigma_space^2),
 *   cw[t] = (float)exp(-0.5 t^2 / sigma_color^2), t = 0 .. 255, both exp in fp64 on the host;
 *   out = cvRound(sum_k v_k w_k / sum_k w_k), w_k = sw[k] cw[|v_k - v0|].
 * The kernel forms w_k as one fp32 product and accumulates both sums in fp32 in tap order, one
 * chain per sum, divides once and rounds half to even: a pixel's result depends on its
 * neighbourhood alone, not on the tile it falls in, the batch index or the stride. Against the
 * same quotient with fp64 products and sums the fp32 quotient is within
 * 255 (2 taps + 3) 2^-24.
 *
 * One workgroup per SPECENH_BILATERAL_TILE_ROWS x SPECENH_BILATERAL_TILE_COLS output tile of
 * one image; the tables travel as kernel arguments: no allocation, graph-capturable. */
#define SPECENH_BILATERAL_MAX_RADIUS 15
#define SPECENH_BILATERAL_TILE_ROWS 8
#define SPECENH_BILATERAL_TILE_COLS 128

/* The radius (>= 1) and the tap count cv2 derives from (d, sigma_space), each written where
 * its pointer is not null. SPECENH_EINVAL for a non-finite sigma_space, SPECENH_EUNSUPPORTED
 * (nothing written) for a radius above SPECENH_BILATERAL_MAX_RADIUS. */
int specenh_bilateral_taps(int d, double sigma_space, int* radius, int* taps);

/* The raw 8-bit filter. img: device uint8, image b at img + b*stride (bytes), row-major
 * rows x cols, stride >= rows*cols; out: device uint8, contiguous [batch][rows][cols], must not
 * overlap img. */
int specenh_bilateral_u8(const unsigned char* img, long long batch, int rows, int cols,
                         long long stride, int d, double sigma_color, double sigma_space,
                         unsigned char* out, void* stream);

/* bilateral(src) on a batch of spectrograms: quantise as specenh_gaussblr does, filter,
 * rescale as numpy does on a uint8 array ((u - min) / (max - min) in fp64; a constant result
 * gives NaN). dtype: SPECENH_DTYPE_F32 or _F64; S and out as for specenh_gaussblr (spectrogram
 * b at S + b*stride elements, out with the same stride). workspace: device, 16-byte aligned,
 * specenh_bilateral_workspace_bytes(batch, rows, cols) bytes: the statistics (16 bytes a
 * spectrogram) and two uint8 planes, each rounded up to 256 bytes; 16 for an empty call. */
size_t specenh_bilateral_workspace_bytes(long long batch, int rows, int cols);
int specenh_bilateral(int dtype, const void* S, long long batch, int rows, int cols,
                      long long stride, int d, double sigma_color, double sigma_space,
                      void* out, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SPECENH_BILATERAL_H */
