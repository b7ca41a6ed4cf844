"""Time the fused averaged spectra (specenh_spectral_mean) at the C2 shape (4096 x 65536
samples, nperseg 1024 / noverlap 768 hamm, linear detrend, density) against the routes that
exist without it, in the same run: specenh_stft_psd flags 0 followed by .mean(-1) for the
Welch PSD, and specenh_csd COMPLEX followed by .mean(-1) for the averaged cross spectrum,
both on the device. HIP events around each route, a warm-up, interleaved rounds, median (and
min) of ROUNDS runs each; algorithmic bytes over the time as a fraction of 8 TB/s.
    python tools/spectral_bench.py [B] [--json PATH]"""
import statistics

from benchlib import parse_args, sample, write_json  # puts the package on sys.path

import torch
from specenh import ops as _ops
from specenh import spectral, stft
from specenh.synthetic import plasma_chirps_torch

path, _, args = parse_args()
B = int(args[0]) if args else 4096
L, N, NOV, WIN, FS = 65536, 1024, 768, "hamm", 500000.0
DENSITY, LINEAR = 0, 2
ROUNDS, WARM, HBM = 25, 3, 8.0e12
F = N // 2 + 1
NAVG = 8
ops = torch.ops.specenh
PLAN = (N, NOV, WIN, FS, DENSITY, LINEAR)

x = plasma_chirps_torch(B, L, seed=1, device="cuda")
y = 0.7 * torch.roll(x, 3, dims=1) + 0.5 * plasma_chirps_torch(B, L, seed=2, device="cuda")
T = stft.frame_count(L, N, NOV)
G = spectral.group_count(T, NAVG)
P = torch.empty((B, F, T), device="cuda")


def outputs(groups, pair):
    return [torch.empty((B, F, groups), device="cuda", dtype=torch.complex64 if i == 2
                        else torch.float32) if pair or i == 0 else None for i in range(4)]


W0, W8, A0, A8 = outputs(1, False), outputs(G, False), outputs(1, True), outputs(G, True)
ws0 = _ops.spectral_workspace(x, *PLAN, 0)
ws8 = _ops.spectral_workspace(x, *PLAN, NAVG)
sig, spec = 4 * B * L, B * F  # bytes of one signal; elements of one [B][F] output

runs = {
    "stft_psd flags=0 + mean": (
        lambda: ops.stft_psd_out(x, *PLAN, 1e-11, 0, P) or P.mean(-1),
        sig + 4 * spec * T + 4 * spec * T + 4 * spec),
    "csd complex + mean": (lambda: ops.csd(x, y, *PLAN, 0).mean(-1),
                           2 * sig + 8 * spec * T + 8 * spec * T + 8 * spec),
    "spectral_mean welch navg=0": (lambda: ops.spectral_mean_out(x, None, *PLAN, 0, *W0, ws0),
                                   sig + 4 * spec),
    "spectral_mean welch navg=8": (lambda: ops.spectral_mean_out(x, None, *PLAN, NAVG, *W8, ws8),
                                   sig + 4 * spec * G),
    "spectral_mean pair navg=0": (lambda: ops.spectral_mean_out(x, y, *PLAN, 0, *A0, ws0),
                                  2 * sig + 20 * spec),
    "spectral_mean pair navg=8": (lambda: ops.spectral_mean_out(x, y, *PLAN, NAVG, *A8, ws8),
                                  2 * sig + 20 * spec * G),
}
times = sample({k: fn for k, (fn, _) in runs.items()}, ROUNDS, WARM)
# the fused results against the routes they replace
ops.stft_psd_out(x, *PLAN, 1e-11, 0, P)
ops.spectral_mean_out(x, y, *PLAN, 0, *A0, ws0)
old_pxx, old_pxy = P.mean(-1), ops.csd(x, y, *PLAN, 0).mean(-1)
agree = {"pxx_normwise": float(((A0[0][..., 0] - old_pxx).abs().amax(1) / old_pxx.amax(1)).max()),
         "pxy_normwise": float(((A0[2][..., 0] - old_pxy).abs().amax(1)
                                / old_pxy.abs().amax(1)).max())}
res = {"shape": {"batch": B, "length": L, "nperseg": N, "noverlap": NOV, "window": WIN,
                 "detrend": "linear", "scaling": "density", "frames": T, "navg": NAVG,
                 "groups": G},
       "rounds": ROUNDS, "hbm_bytes_per_s": HBM, "agreement_with_existing_routes": agree,
       "workspace_bytes": {"navg=0": int(ws0.numel()), "navg=8": int(ws8.numel())},
       "kernels": {}}
med = {k: statistics.median(v) for k, v in times.items()}
for k, (_, alg) in runs.items():
    base = med["stft_psd flags=0 + mean" if "welch" in k or "stft_psd" in k
               else "csd complex + mean"]
    res["kernels"][k] = {"ms_median": med[k], "ms_min": min(times[k]), "algorithmic_bytes": alg,
                         "hbm_fraction": alg / (med[k] * 1e-3) / HBM,
                         "x_existing_route": med[k] / base}
    print(f"{k:28s} median {med[k]:8.4f} ms  min {min(times[k]):8.4f} ms  "
          f"{alg / med[k] / 1e6:6.0f} GB/s  frac {alg / (med[k] * 1e-3) / HBM:.3f}  "
          f"x existing route {med[k] / base:.3f}", flush=True)
print(f"agreement with the existing routes (normwise): {agree}")
write_json(res, path)
