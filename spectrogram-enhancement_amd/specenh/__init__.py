"""specenh — MI355X-native spectrogram-enhancement hot path (gfx950, HIP via a C-ABI).

Reference-compatible entry points (same names/arguments as the reference):
  specenh.pipeline_data : specgr, norm, rescale, quantfilt, gaussblr, meansub, morph, and
                          bilateral (the denoiser of spec_denoising/dataset.ipynb)
  specenh.restoration   : denoise_nl_means (non-local means, for `from skimage import restoration`)
  specenh.cluster       : KMeans (for `from sklearn.cluster import KMeans`), batched kmeans,
                          segment (pixel k-means: a data-driven mode / background mask)
  specenh.svd           : omega, denoiseSignal, computeSignal
  specenh.strips        : patch, unpatch, reshape
  specenh.keras         : layers / Model / compile / fit / predict / save / load_model
scipy-compatible return path (complex STFT, gain mask, inverse STFT):
  specenh.signal        : stft, istft (numpy); specenh.stft.stft / istft (device tensors)
scipy-compatible time-averaged spectra (Welch PSD, CSD, coherence, coherogram):
  specenh.signal        : welch, csd, coherence (numpy); specenh.spectral (device tensors)
cross-spectral matrix and coherence matrix of a channel array (every pair in one call):
  specenh.signal.cross_spectral_matrix (numpy); specenh.spectral.cross_spectral_matrix,
  coherence_matrix (device tensors)
bispectrum and squared bicoherence (three-wave coupling, auto and cross):
  specenh.signal.bicoherence (numpy); specenh.bispectrum.bispectrum, bicoherence,
  bispectrum_from_spectra, summed_bicoherence (device tensors)
two-point wavenumber-frequency spectrum S(k, f) (dispersion relation from two channels):
  specenh.signal.wavenumber_spectrum (numpy); specenh.wavenumber.wavenumber_spectrum,
  wavenumber_spectrum_from_spectra, conditional_spectrum, dispersion (device tensors)
block-averaged lagged cross-correlation (time-delay estimation, correlation time):
  specenh.signal.correlate (numpy); specenh.correlation.correlate, autocorrelate,
  correlation_lags, time_delay, correlation_time (device tensors)
steered-response spectra of a channel array (Bartlett, Capon, MUSIC: mode numbers, wavenumbers):
  specenh.signal.array_spectrum (numpy); specenh.beamform.array_spectrum,
  mode_number_spectrum, steered_power, steering_vectors, delay_steering (device tensors)
continuous wavelet transform (Morlet scalogram) and complex FIR filter bank:
  specenh.signal.cwt (numpy); specenh.wavelet.cwt, scalogram, filter_bank, FilterBank,
  morlet_filters, morlet_scales, scale_to_frequency, cone_of_influence (device tensors)
cross-wavelet spectrum, wavelet coherence and phase of channel pairs (mode numbers of chirps):
  specenh.signal.wavelet_coherence (numpy); specenh.wavelet.cross_wavelet, cross_filter_bank,
  wavelet_coherence, smoothing_windows (device tensors)
Device fast paths: specgr_batch, denoise_batch, cross_spectrogram_batch, and
specenh.autograd (differentiable Conv2D / Conv2DTranspose / MaxPooling2D / BCE).
Every one of them reaches the HIP kernels through the ``torch.ops.specenh`` operators
(specenh/ops.py, registered when the package is imported) and the C-ABI.

Importing the package does not touch the GPU; the HIP library is loaded on the
first op call and its absence raises specenh._lib.ExtensionNotLoaded.
"""
__version__ = "0.2.0"

from . import ops  # noqa: E402,F401  (registers torch.ops.specenh.*)
from . import restoration  # noqa: E402,F401  (specenh.restoration.denoise_nl_means)
from . import cluster  # noqa: E402,F401  (specenh.cluster.KMeans)


def load_library():
    """Load libspecenh.so now (raises ExtensionNotLoaded if it is missing)."""
    from . import _lib

    return _lib.lib()
