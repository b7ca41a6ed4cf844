"""ctypes binding of libspecenh.so (the C-ABI declared in include/specenh.h).

torch is imported first so that the HIP runtime already mapped by torch
(torch/lib/libamdhip64.so, SONAME libamdhip64.so.7) is the one libspecenh.so
binds to: device pointers and streams from torch are then valid in the library.

There is no fallback: if the library is missing or fails to load, every op
raises ExtensionNotLoaded.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch  # noqa: F401  (must precede the dlopen below; see module docstring)

# SPECENH_LIB: development A/B builds only (tools/build_variant.sh); default = in-tree build
LIB_PATH = os.environ.get("SPECENH_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                         "libspecenh.so")

SPECENH_OK = 0
SPECENH_EINVAL = -1
SPECENH_EUNSUPPORTED = -2
SPECENH_EHIP = -3
SPECENH_ENOMEM = -4
SPECENH_ERANGE = -5
SVD_OPTIMAL = 0
FILTER_NORM = 0
FILTER_RESCALE = 1
FILTER_MEANSUB = 2
SVD_COMPUTE = 1

STFT_LOG = 1
STFT_NORMALIZE = 2
STFT_DROP_NYQUIST = 4
STFT_EXACT = 8  # one frame per FFT (include/specenh.h SPECENH_STFT_EXACT)

DETREND = {False: 0, None: 0, "constant": 1, "c": 1, "linear": 2, "l": 2}
SCALING = {"density": 0, "spectrum": 1}
BOUNDARY_NONE = 0
BOUNDARY_ZEROS = 1


class ExtensionNotLoaded(RuntimeError):
    pass


_lock = threading.Lock()
_lib = None

# name -> (restype, argtypes); must match include/specenh.h exactly
_c = ctypes
SIGNATURES = {
    "specenh_last_error": (_c.c_char_p, []),
    "specenh_version": (_c.c_char_p, []),
    "specenh_set_variant": (_c.c_int, [_c.c_char_p, _c.c_int]),
    "specenh_get_variant": (_c.c_int, [_c.c_char_p, _c.POINTER(_c.c_int)]),
    "specenh_last_kernel_name": (_c.c_char_p, []),
    "specenh_launch_count": (_c.c_longlong, []),
    "specenh_kernel_name_at": (_c.c_char_p, [_c.c_longlong]),
    "specenh_stream_wait": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int]),
    "specenh_stft_frames": (_c.c_longlong, [_c.c_longlong, _c.c_int, _c.c_int]),
    "specenh_stft_plan_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int,
                                            _c.POINTER(_c.c_double), _c.c_double, _c.c_int,
                                            _c.c_int, _c.c_double]),
    "specenh_stft_plan_destroy": (_c.c_int, [_c.c_void_p]),
    "specenh_stft_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_longlong]),
    "specenh_stft_psd_f16": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_longlong, _c.c_longlong,
                                        _c.c_longlong, _c.c_void_p, _c.c_int, _c.c_void_p]),
    "specenh_stft_psd": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_longlong, _c.c_longlong,
                                    _c.c_longlong, _c.c_void_p, _c.c_int, _c.c_void_p,
                                    _c.c_void_p]),
    "specenh_csd_plan_create": (_c.c_int, [_c.POINTER(_c.c_void_p), _c.c_int, _c.c_int,
                                           _c.POINTER(_c.c_double), _c.c_double, _c.c_int,
                                           _c.c_int]),
    "specenh_csd_plan_destroy": (_c.c_int, [_c.c_void_p]),
    "specenh_csd": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_longlong,
                               _c.c_longlong, _c.c_longlong, _c.c_longlong, _c.c_void_p, _c.c_int,
                               _c.c_void_p]),
    "specenh_svd_workspace_bytes": (_c.c_size_t, [_c.c_longlong, _c.c_int, _c.c_int, _c.c_int]),
    "specenh_svd_denoise_workspace_bytes": (_c.c_size_t, [_c.c_longlong, _c.c_int, _c.c_int,
                                                          _c.c_int, _c.c_int]),
    "specenh_svd_denoise": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                       _c.c_longlong, _c.c_int, _c.c_int, _c.c_void_p,
                                       _c.c_void_p, _c.c_void_p]),
    "specenh_svd_denoise_ex": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                          _c.c_longlong, _c.c_int, _c.c_int, _c.c_void_p,
                                          _c.c_int, _c.c_void_p, _c.c_void_p]),
    "specenh_svd_optimal_workspace_bytes": (_c.c_size_t, [_c.c_longlong, _c.c_int, _c.c_int]),
    "specenh_svd_denoise_optimal": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                               _c.c_longlong, _c.c_int, _c.c_void_p,
                                               _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                               _c.c_void_p]),
    "specenh_conv2d": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                  _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                  _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                  _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int,
                                  _c.c_int, _c.c_void_p, _c.c_void_p]),
    "specenh_conv2d_wgrad": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_void_p]),
    "specenh_conv2d_wgrad_ex": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                           _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int,
                                           _c.c_void_p, _c.c_void_p]),
    "specenh_conv2d_wgrad_workspace_bytes": (_c.c_size_t, [_c.c_int] * 7),
    "specenh_conv2d_wgrad_pooled": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int,
                                               _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                               _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                               _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                               _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                               _c.c_void_p]),
    "specenh_conv2d_pooled_in": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                            _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                            _c.c_int, _c.c_int, _c.c_int, _c.c_void_p, _c.c_int,
                                            _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                            _c.c_void_p, _c.c_void_p]),
    "specenh_convt_conv_out": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                          _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int,
                                          _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p,
                                          _c.c_void_p]),
    "specenh_convt_conv_out_train": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int,
                                                _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                                _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p,
                                                _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                                _c.c_void_p]),
    "specenh_decoder3": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_int,
                                    _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                    _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p,
                                    _c.c_void_p]),
    "specenh_decoder3_ex": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                       _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p,
                                       _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_int,
                                       _c.c_void_p, _c.c_int, _c.c_void_p]),
    "specenh_encoder2": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                    _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p,
                                    _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "specenh_maxpool2_fwd": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                        _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "specenh_maxpool2_bwd": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                        _c.c_int, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                        _c.c_void_p]),
    "specenh_bce_logits": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_longlong,
                                      _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p]),
    "specenh_adam_step": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                     _c.c_longlong, _c.c_float, _c.c_float, _c.c_float,
                                     _c.c_float, _c.c_float, _c.c_void_p, _c.c_int,
                                     _c.c_void_p]),
    "specenh_adam_step_flip": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                          _c.c_longlong, _c.c_float, _c.c_float, _c.c_float,
                                          _c.c_float, _c.c_float, _c.c_void_p, _c.c_int, _c.c_int,
                                          _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "specenh_weight_flip_transpose": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_int,
                                                 _c.c_int, _c.c_void_p, _c.c_void_p]),
    "specenh_cast": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_int, _c.c_void_p, _c.c_longlong,
                                _c.c_void_p]),
    "specenh_filter_workspace_bytes": (_c.c_size_t, [_c.c_longlong, _c.c_int]),
    "specenh_filter": (_c.c_int, [_c.c_int, _c.c_int, _c.c_void_p, _c.c_longlong, _c.c_int,
                                  _c.c_int, _c.c_longlong, _c.c_void_p, _c.c_void_p,
                                  _c.c_void_p]),
    "specenh_quantfilt": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                     _c.c_longlong, _c.c_double, _c.c_void_p, _c.c_void_p]),
    "specenh_u8filter_workspace_bytes": (_c.c_size_t, [_c.c_longlong, _c.c_int, _c.c_int]),
    "specenh_gaussblr": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                    _c.c_longlong, _c.c_int, _c.c_int, _c.c_double, _c.c_void_p,
                                    _c.c_void_p, _c.c_void_p]),
    "specenh_morph": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                 _c.c_longlong, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    "specenh_strips_pack": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                       _c.c_longlong, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                       _c.c_void_p]),
    "specenh_strips_unpack": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                         _c.c_int, _c.c_void_p, _c.c_void_p]),
}

# the complex STFT / inverse STFT entry points; must match include/specenh_stft_complex.h
SIGNATURES_STFT_COMPLEX = {
    "specenh_stft_complex_frames": (_c.c_longlong, [_c.c_longlong, _c.c_int, _c.c_int, _c.c_int,
                                                    _c.c_int]),
    "specenh_stft_complex": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_longlong, _c.c_longlong,
                                        _c.c_longlong, _c.c_void_p, _c.c_int, _c.c_int,
                                        _c.c_void_p]),
    "specenh_istft_length": (_c.c_longlong, [_c.c_longlong, _c.c_int, _c.c_int, _c.c_int]),
    "specenh_istft": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_longlong,
                                 _c.c_longlong, _c.c_void_p, _c.c_longlong, _c.c_int,
                                 _c.c_void_p]),
}

# time-averaged spectra (Welch / CSD / coherence); must match include/specenh_spectral.h
SPECTRAL_CHUNK = 32  # SPECENH_SPECTRAL_CHUNK: frames summed in fp32 before fp64 takes over
SPECTRAL_PXX, SPECTRAL_PYY, SPECTRAL_PXY, SPECTRAL_COH = 1, 2, 4, 8  # operator output mask
SIGNATURES_SPECTRAL = {
    "specenh_spectral_groups": (_c.c_longlong, [_c.c_longlong, _c.c_longlong]),
    "specenh_spectral_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_longlong,
                                                       _c.c_longlong, _c.c_longlong]),
    "specenh_spectral_mean": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_longlong,
                                         _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                         _c.c_longlong, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                         _c.c_void_p, _c.c_void_p, _c.c_void_p]),
}

# cross-spectral matrix of a channel array; must match include/specenh_csm.h
CSM_MAX_CHANNELS = 64  # SPECENH_CSM_MAX_CHANNELS
CSM_CSM, CSM_COH = 1, 2  # operator output mask
# The tensor layer splits the batch so that one launch's workspace (the spectra of every
# frame, 8 B F T C bytes a shot) stays under this many bytes; a single shot above it still
# runs alone. Results do not depend on the split.
CSM_WORKSPACE_CAP = 1 << 30
SIGNATURES_CSM = {
    "specenh_csm_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_longlong, _c.c_longlong,
                                                  _c.c_longlong, _c.c_longlong]),
    "specenh_csm": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_longlong, _c.c_longlong,
                               _c.c_longlong, _c.c_longlong, _c.c_longlong, _c.c_longlong,
                               _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_size_t,
                               _c.c_void_p]),
}

# mode decomposition (batched Hermitian eigensolver); must match include/specenh_modes.h
HERM_EIG_MAX_N = 64  # SPECENH_HERM_EIG_MAX_N
HERM_EIG_MAX_SWEEPS = 16  # SPECENH_HERM_EIG_MAX_SWEEPS
SIGNATURES_MODES = {
    "specenh_herm_eig": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                    _c.c_longlong, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                    _c.c_void_p]),
}

# bispectrum and squared bicoherence; must match include/specenh_bispectrum.h
BISPEC_BISPEC, BISPEC_BICOH = 1, 2  # operator output mask
SIGNATURES_BISPECTRUM = {
    "specenh_bispectrum_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_longlong,
                                                         _c.c_longlong, _c.c_longlong,
                                                         _c.c_longlong]),
    "specenh_bispectrum": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                      _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                      _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                      _c.c_longlong, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                      _c.c_size_t, _c.c_void_p]),
    "specenh_bispectrum_spectra": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p,
                                              _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                              _c.c_longlong, _c.c_longlong, _c.c_void_p,
                                              _c.c_void_p, _c.c_void_p]),
}

# two-point wavenumber-frequency spectrum S(k, f); must match include/specenh_wavenumber.h
WAVENUMBER_MIN_NK, WAVENUMBER_MAX_NK = 4, 256
SIGNATURES_WAVENUMBER = {
    "specenh_wavenumber_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_longlong,
                                                         _c.c_longlong, _c.c_longlong,
                                                         _c.c_longlong]),
    "specenh_wavenumber_spectrum": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p,
                                               _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                               _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                               _c.c_void_p, _c.c_void_p, _c.c_size_t,
                                               _c.c_void_p]),
    "specenh_wavenumber_spectra": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_longlong,
                                              _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                              _c.c_longlong, _c.c_void_p, _c.c_void_p]),
}

# block-averaged cross-correlation; must match include/specenh_correlation.h
CORR_RAW, CORR_COEFF = 0, 1  # SPECENH_CORR_RAW, SPECENH_CORR_COEFF
CORR_MAX_NPERSEG = 2048  # the padded transform is at most the 4096 points of the LDS FFT
SIGNATURES_CORRELATION = {
    "specenh_correlation_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_longlong,
                                                          _c.c_longlong, _c.c_longlong,
                                                          _c.c_longlong]),
    "specenh_correlation": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_longlong,
                                       _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                       _c.c_longlong, _c.c_longlong, _c.c_int, _c.c_void_p,
                                       _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
}

# steered-response spectra (Bartlett, Capon, MUSIC); must match include/specenh_beamform.h
STEER_MAX_CHANNELS = 64  # SPECENH_STEER_MAX_CHANNELS
STEER_MAX_NSTEER = 4096  # SPECENH_STEER_MAX_NSTEER
# SPECENH_STEER_*: the epilogue of the steered-power kernel
STEER_SUM, STEER_BARTLETT, STEER_INVERSE, STEER_MUSIC = 0, 1, 2, 3
SIGNATURES_BEAMFORM = {
    "specenh_steered_power": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_longlong,
                                         _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                         _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                         _c.c_longlong, _c.c_int, _c.c_double, _c.c_void_p,
                                         _c.c_int, _c.c_void_p, _c.c_void_p]),
    "specenh_array_spectrum_workspace_bytes": (_c.c_size_t, [_c.c_void_p, _c.c_longlong,
                                                             _c.c_longlong, _c.c_longlong,
                                                             _c.c_longlong]),
    "specenh_array_spectrum": (_c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_longlong,
                                          _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                          _c.c_longlong, _c.c_longlong, _c.c_void_p,
                                          _c.c_longlong, _c.c_int, _c.c_void_p, _c.c_void_p,
                                          _c.c_size_t, _c.c_void_p]),
}

# complex FIR filter bank (wavelet transform); must match include/specenh_wavelet.h
FB_COMPLEX, FB_POWER, FB_POWER_MEAN = 0, 1, 2  # SPECENH_FB_*: what an output element holds
FB_MAX_HALF = 1024  # SPECENH_FB_MAX_HALF
FB_NFFT = (256, 512, 1024, 2048, 4096)  # the transform lengths of the overlap-save blocks
SIGNATURES_WAVELET = {
    "specenh_filterbank_nfft": (_c.c_int, [_c.c_int, _c.c_int]),
    "specenh_filterbank_tables_bytes": (_c.c_size_t, [_c.c_int, _c.c_int]),
    "specenh_filterbank_tables": (_c.c_int, [_c.c_int, _c.POINTER(_c.c_int),
                                             _c.POINTER(_c.c_double), _c.c_int, _c.c_void_p]),
    "specenh_filterbank": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int, _c.c_void_p,
                                      _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                      _c.c_longlong, _c.c_int, _c.c_void_p, _c.c_void_p]),
}

# cross spectrum of a pair through a filter bank; must match include/specenh_wavelet_cross.h
XWT_POINT, XWT_MEAN = 0, 1  # SPECENH_XWT_*: values at every hop-th sample, or hop-window means
SIGNATURES_WAVELET_CROSS = {
    "specenh_filterbank_cross": (_c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_int,
                                            _c.c_void_p, _c.c_void_p, _c.c_longlong,
                                            _c.c_longlong, _c.c_longlong, _c.c_longlong,
                                            _c.c_longlong, _c.c_int, _c.c_void_p, _c.c_void_p,
                                            _c.c_void_p, _c.c_void_p]),
    "specenh_filterbank_cross_chunk": (_c.c_int, [_c.c_int, _c.c_int, _c.c_int, _c.c_longlong,
                                                  _c.c_longlong, _c.c_longlong, _c.c_int,
                                                  _c.c_int]),
}

# bilateral label filter; must match include/specenh_bilateral.h
BILATERAL_MAX_RADIUS = 15  # SPECENH_BILATERAL_MAX_RADIUS
# SPECENH_BILATERAL_TILE_ROWS / _COLS: the output tile of one workgroup
BILATERAL_TILE_ROWS, BILATERAL_TILE_COLS = 8, 128
SIGNATURES_BILATERAL = {
    "specenh_bilateral_taps": (_c.c_int, [_c.c_int, _c.c_double, _c.POINTER(_c.c_int),
                                          _c.POINTER(_c.c_int)]),
    "specenh_bilateral_u8": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                        _c.c_longlong, _c.c_int, _c.c_double, _c.c_double,
                                        _c.c_void_p, _c.c_void_p]),
    "specenh_bilateral_workspace_bytes": (_c.c_size_t, [_c.c_longlong, _c.c_int, _c.c_int]),
    "specenh_bilateral": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                     _c.c_longlong, _c.c_int, _c.c_double, _c.c_double,
                                     _c.c_void_p, _c.c_void_p, _c.c_void_p]),
}

# non-local means denoising; must match include/specenh_nlmeans.h
NLMEANS_MAX_PATCH = 9  # SPECENH_NLMEANS_MAX_PATCH
NLMEANS_MAX_DISTANCE = 15  # SPECENH_NLMEANS_MAX_DISTANCE
# SPECENH_NLMEANS_TILE_ROWS / _COLS: the output tile of one workgroup
NLMEANS_TILE_ROWS, NLMEANS_TILE_COLS = 16, 64
SIGNATURES_NLMEANS = {
    "specenh_nlmeans": (_c.c_int, [_c.c_int, _c.c_void_p, _c.c_longlong, _c.c_int, _c.c_int,
                                   _c.c_longlong, _c.c_int, _c.c_int, _c.c_double, _c.c_double,
                                   _c.c_void_p, _c.c_void_p]),
}

# k-means clustering; must match include/specenh_kmeans.h
KMEANS_MAX_K = 256  # SPECENH_KMEANS_MAX_K
KMEANS_MAX_D = 65536  # SPECENH_KMEANS_MAX_D
# SPECENH_KMEANS_TILE / _CHUNK / _SLAB: points of a workgroup, d of a chunk of the dot
# products, points of a slab of the update (the rounding counts c_s and c_u follow from them)
KMEANS_TILE, KMEANS_CHUNK, KMEANS_SLAB = 64, 32, 1024
SIGNATURES_KMEANS = {
    "specenh_kmeans_workspace_bytes": (_c.c_size_t, [_c.c_longlong, _c.c_longlong, _c.c_int,
                                                     _c.c_int]),
    "specenh_kmeans_assign": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_longlong, _c.c_int,
                                         _c.c_longlong, _c.c_longlong, _c.c_void_p, _c.c_int,
                                         _c.c_void_p, _c.c_void_p, _c.c_size_t, _c.c_void_p]),
    "specenh_kmeans_step": (_c.c_int, [_c.c_void_p, _c.c_longlong, _c.c_longlong, _c.c_int,
                                       _c.c_longlong, _c.c_longlong, _c.c_void_p, _c.c_int,
                                       _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                       _c.c_void_p, _c.c_size_t, _c.c_void_p]),
}


def lib():
    """Load (once) and return the ctypes handle; raise ExtensionNotLoaded on failure."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ExtensionNotLoaded(
                f"{LIB_PATH} not found: build it with `python spectrogram-enhancement_amd/build.py` "
                "(there is no CPU fallback)")
        try:
            h = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:
            raise ExtensionNotLoaded(f"failed to load {LIB_PATH}: {e}") from e
        dev_build = bool(os.environ.get("SPECENH_LIB"))
        for name, (res, args) in {**SIGNATURES, **SIGNATURES_STFT_COMPLEX,
                                  **SIGNATURES_SPECTRAL, **SIGNATURES_CSM,
                                  **SIGNATURES_MODES, **SIGNATURES_BISPECTRUM,
                                  **SIGNATURES_WAVENUMBER, **SIGNATURES_CORRELATION,
                                  **SIGNATURES_BEAMFORM, **SIGNATURES_WAVELET,
                                  **SIGNATURES_WAVELET_CROSS,
                                  **SIGNATURES_BILATERAL, **SIGNATURES_NLMEANS,
                                  **SIGNATURES_KMEANS}.items():
            if dev_build and not hasattr(h, name):
                continue  # an older revision's build for an A/B run (tools/build_rev_lib.sh)
            fn = getattr(h, name)
            fn.restype = res
            fn.argtypes = args
        _lib = h
    return _lib


def last_error() -> str:
    return lib().specenh_last_error().decode(errors="replace")


def check(rc: int, what: str = "") -> int:
    """Map a C-ABI return code onto the reference's Python exception types."""
    if rc >= 0:
        return rc
    msg = f"{what}: {last_error()}" if what else last_error()
    if rc == SPECENH_EINVAL:
        raise ValueError(msg)
    if rc == SPECENH_EUNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == SPECENH_ENOMEM:
        raise MemoryError(msg)
    if rc == SPECENH_ERANGE:
        raise IndexError(msg)
    raise RuntimeError(msg)


def current_stream_handle(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def get_variant(name: str) -> int:
    v = ctypes.c_int(0)
    check(lib().specenh_get_variant(name.encode(), ctypes.byref(v)), "get_variant")
    return v.value


def set_variant(name: str, value: int) -> None:
    """Select a kernel variant (runtime.hpp: the A/B switches; SPECENH_<name> in the
    environment sets the process default, read once)."""
    check(lib().specenh_set_variant(name.encode(), int(value)), "set_variant")


class variant:
    """Context manager: ``with _lib.variant("CONV_NO_S2", 1): ...`` restores the old value."""

    def __init__(self, name: str, value: int):
        self.name, self.value = name, int(value)

    def __enter__(self):
        self.old = get_variant(self.name)
        set_variant(self.name, self.value)
        return self

    def __exit__(self, *exc):
        set_variant(self.name, self.old)
        return False


def stream_wait(waiter, signaler, device_scope: bool = True) -> None:
    """``waiter`` (torch.cuda.Stream) waits for the work enqueued on ``signaler`` so far, through
    a library event recorded with a device-scope release (specenh_stream_wait)."""
    check(lib().specenh_stream_wait(waiter.cuda_stream, signaler.cuda_stream,
                                    1 if device_scope else 0), "stream_wait")


def last_kernel_name() -> str:
    """Mangled symbol of the last kernel the calling thread launched through the library."""
    return lib().specenh_last_kernel_name().decode(errors="replace")


def launch_count() -> int:
    """Kernels the calling thread has launched through the library so far."""
    return int(lib().specenh_launch_count())


def kernel_names(first: int, end: int) -> list:
    """Symbols of this thread's launches [first, end) (specenh_launch_count numbering)."""
    L = lib()
    return [L.specenh_kernel_name_at(i).decode(errors="replace") for i in range(first, end)]
