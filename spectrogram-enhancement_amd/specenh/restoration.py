"""Drop-in for the ``from skimage import restoration`` line of the reference's files
(spec_denoising/pipeline_data.py:21, VAE/*.py, the notebooks): the toolbox's non-local means
denoiser on the GPU.

    from specenh import restoration
    clean = restoration.denoise_nl_means(s, patch_size=7, patch_distance=11, h=0.08, sigma=0.1)

``denoise_nl_means`` runs as one HIP kernel (csrc/nlmeans.hip) with scikit-image's
``fast_mode=True`` weighting: uniform patch weights, 2 sigma^2 subtracted from the patch
distance, floored at 0. One difference is deliberate: scikit-image drops the shifts whose
scaled distance exceeds 5, here every shift keeps its weight (include/specenh_nlmeans.h).
numpy in, numpy out (float32 stays float32, all else is computed from and returned as float64;
the arithmetic is fp32 either way); a device tensor, 2-D or [batch, rows, cols], stays on the
device.
"""
from __future__ import annotations

from . import filters as _filters


def denoise_nl_means(image, patch_size=7, patch_distance=11, h=0.1, fast_mode=True, sigma=0.0):
    """skimage.restoration.denoise_nl_means for one 2-D image (or a device batch).
    ``fast_mode=False`` (Gaussian-weighted patches) is not implemented."""
    if not fast_mode:
        raise NotImplementedError("denoise_nl_means: only fast_mode=True (uniform patch weights) "
                                  "is implemented")
    return _filters.nl_means(image, patch_size, patch_distance, h, sigma)
