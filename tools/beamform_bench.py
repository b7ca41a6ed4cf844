"""Time the steered-response spectra (csrc/steered_power.hip) on 8 shots x 40 channels x 65,536
samples, nperseg 1024 / noverlap 768 hamm, linear detrend, density, K = 65 mode numbers
(n = -32 .. 32 on 40 irregular angles), whole shot and 31 blocks of 8 frames, in one process:

  bartlett, capon, music   specenh.beamform.array_spectrum whole
  kernel_rows   torch.ops.specenh.steered_power_out alone on the resident frame spectra (the
                Bartlett shape: M = the group's frames)
  kernel_eig    the same on resident eigenvectors and Capon weights (M = C)
  csm_einsum    what Bartlett replaces: cross_spectral_matrix + torch.einsum
  modes_einsum_capon, modes_einsum_music
                what Capon and MUSIC replace: array_modes(k = C) + torch.einsum

HIP events around each route, 2 warm-ups, interleaved rounds, median (and min). Recorded
alongside: the kernel's achieved FLOP/s on 8 M C K a matrix against the 157.3 TF fp32 peak, its
algorithmic bytes (rows, table, weights, output; each once) against the 8.0 TB/s of HBM, the
agreement of each route with what it replaces, and the kernel's resource usage
(-Rpass-analysis=kernel-resource-usage).
    python tools/beamform_bench.py [--json PATH] [--rounds N]"""
import json

from benchlib import measure, parse_args, resources, write_json  # puts the package on sys.path

import numpy as np
import torch
from specenh import _lib, beamform, ops as _ops, spectral
from specenh.synthetic import plasma_chirps_torch

path, ROUNDS, _ = parse_args(7)
B, C, L, N, NOV, WIN, FS, K = 8, 40, 65536, 1024, 768, "hamm", 500000.0, 65
WARM = 2
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12
KW = dict(fs=FS, window=WIN, nperseg=N, noverlap=NOV, detrend="linear", scaling="density")
ops = torch.ops.specenh

angles = np.sort(np.random.default_rng(40).uniform(0, 2 * np.pi, C))
A = beamform.steering_vectors(angles, np.arange(K) - K // 2, "cuda")
x = plasma_chirps_torch(B * C, L, seed=1, device="cuda").reshape(B, C, L)
res = {"plan": {"nperseg": N, "noverlap": NOV, "window": WIN, "detrend": "linear",
                "scaling": "density"}, "batch": B, "channels": C, "length": L, "nsteer": K,
       "rounds": ROUNDS, "warmups": WARM, "peak_fp32_flops": PEAK_FLOPS,
       "peak_hbm_bytes_per_s": PEAK_BYTES,
       "kernel_resources": resources("steered_power.hip"), "runs": {}}
print(json.dumps(res["kernel_resources"]), flush=True)


def kernel_figures(ms, count, M, weights):
    flops = 8.0 * M * C * K * count
    nbytes = count * M * C * 8 + K * C * 8 + (count * M * 4 if weights else 0) + count * K * 4
    s = ms * 1e-3
    return {"matrices": count, "rows": M, "flops": flops, "algorithmic_bytes": nbytes,
            "tflops": flops / s / 1e12, "fraction_of_fp32_peak": flops / s / PEAK_FLOPS,
            "gbytes_per_s": nbytes / s / 1e9, "fraction_of_hbm_peak": nbytes / s / PEAK_BYTES}


def capon_weights(lam, loading=1e-2):
    lam = lam.double()
    d = lam.clamp_min(0) + loading * lam.sum(-1, keepdim=True) / C
    return torch.where(d == 0, torch.zeros_like(d), 1.0 / d).float()


def einsum_bartlett(navg):
    S = spectral.cross_spectral_matrix(x, navg=navg, want=("csm",), **KW)[2]["csm"]
    return torch.einsum("ki,bfgij,kj->bfgk", A, S, A.conj()).real / C ** 2


def einsum_eig(navg, method):
    est = spectral.array_modes(x, k=C, navg=navg, **KW)[2]
    p2 = torch.einsum("bfgmc,kc->bfgmk", est["modes"], A).abs() ** 2
    if method == "capon":
        return 1.0 / (capon_weights(est["power"])[..., None] * p2).sum(-2)
    return C / p2[..., 2:, :].sum(-2)


def agreement(a, b):
    """max over matrices of max_n |a - b| / max_n |b|."""
    return float(((a - b).abs().amax(-1) / b.abs().amax(-1)).max())


for label, navg in (("whole shot", 0), ("31 blocks of 8 frames", 8)):
    args = (N, NOV, WIN, FS, 0, 2, navg)
    T = (L - N) // (N - NOV) + 1
    glen, G = (navg, T // navg) if navg else (T, 1)
    F = N // 2 + 1
    count = B * F * G
    # resident inputs of the kernel alone: the frame spectra, the eigenvectors and weights
    ws = _ops.array_spectrum_workspace(x, *args)
    out = torch.empty((B, F, G, K), device="cuda")
    ops.array_spectrum_out(x, *args, A, out, ws)
    rows = ws.view(torch.complex64).view(B, F, G, glen, C)
    est = spectral.array_modes(x, k=C, navg=navg, **KW)[2]
    vec, wts = est["modes"], capon_weights(est["power"])
    del est
    runs = {"bartlett": lambda: beamform.array_spectrum(x, A, navg=navg, **KW),
            "capon": lambda: beamform.array_spectrum(x, A, "capon", navg=navg, **KW),
            "music": lambda: beamform.array_spectrum(x, A, "music", 2, navg=navg, **KW),
            "kernel_rows": lambda: ops.steered_power_out(rows, None, A, _lib.STEER_BARTLETT, 1.0,
                                                         True, None, out),
            "kernel_eig": lambda: ops.steered_power_out(vec, wts, A, _lib.STEER_INVERSE, 1.0,
                                                        False, None, out),
            "csm_einsum": lambda: einsum_bartlett(navg),
            "modes_einsum_capon": lambda: einsum_eig(navg, "capon"),
            "modes_einsum_music": lambda: einsum_eig(navg, "music")}
    entry = {"navg": navg, "groups": G, "frames_per_group": glen, "matrices": count,
             "csm_bytes_not_held_by_bartlett": count * C * C * 8}
    entry.update(measure(runs, ROUNDS, WARM))
    entry["kernel_rows_figures"] = kernel_figures(entry["kernel_rows_ms_median"], count, glen,
                                                  False)
    entry["kernel_eig_figures"] = kernel_figures(entry["kernel_eig_ms_median"], count, C, True)
    entry["csm_einsum_over_bartlett"] = (entry["csm_einsum_ms_median"]
                                         / entry["bartlett_ms_median"])
    for m in ("capon", "music"):
        entry[f"modes_einsum_{m}_over_{m}"] = (entry[f"modes_einsum_{m}_ms_median"]
                                               / entry[f"{m}_ms_median"])
    entry["agreement"] = {
        "bartlett": agreement(runs["bartlett"]()[2], einsum_bartlett(navg)),
        "capon": agreement(runs["capon"]()[2], einsum_eig(navg, "capon")),
        "music": agreement(runs["music"]()[2], einsum_eig(navg, "music"))}
    print(f"{label:24s} " + "  ".join(f"{n} {entry[n + '_ms_median']:.3f} ms" for n in runs),
          flush=True)
    print(f"{label:24s} kernel_rows {entry['kernel_rows_figures']['tflops']:.2f} TF "
          f"{entry['kernel_rows_figures']['gbytes_per_s']:.0f} GB/s  kernel_eig "
          f"{entry['kernel_eig_figures']['tflops']:.2f} TF "
          f"{entry['kernel_eig_figures']['gbytes_per_s']:.0f} GB/s  agreement "
          f"{entry['agreement']}", flush=True)
    res["runs"][label] = entry
    del rows, ws, vec, wts, out
    torch.cuda.empty_cache()
write_json(res, path)
