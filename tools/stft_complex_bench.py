"""Time the complex STFT and the inverse STFT at the C2 shape (4096 x 65536 samples, nperseg
1024 / noverlap 768 hamm, boundary='zeros') against specenh_stft_psd with flags = 0 at the
same shape in the same run. HIP events around single launches, a warm-up, interleaved rounds,
median (and min) of ROUNDS launches each; algorithmic bytes over the time as a fraction of
8 TB/s.   python tools/stft_complex_bench.py [B] [--json PATH]"""
import statistics

from benchlib import parse_args, sample, write_json  # puts the package on sys.path

import torch
from specenh import stft
from specenh.synthetic import plasma_chirps_torch

path, _, args = parse_args()
B = int(args[0]) if args else 4096
L, N, NOV, WIN, FS = 65536, 1024, 768, "hamm", 500000.0
ROUNDS, WARM, HBM = 25, 3, 8.0e12
F = N // 2 + 1
ops = torch.ops.specenh

x = plasma_chirps_torch(B, L, seed=1, device="cuda")
T = stft.complex_frame_count(L, N, NOV, "zeros", True)
n_out = stft.istft_length(T, N, NOV, True)
Z = torch.empty((B, F, T), dtype=torch.complex64, device="cuda")
y = torch.empty((B, n_out), device="cuda")
Tp = stft.frame_count(L, N, NOV)
P = torch.empty((B, F, Tp), device="cuda")
gain = torch.rand((B, F - 1, T), device="cuda")

runs = {
    "stft_psd flags=0": (lambda: ops.stft_psd_out(x, N, NOV, WIN, FS, 0, 0, 1e-11, 0, P),
                         B * (4 * L + 4 * F * Tp)),
    "stft_complex": (lambda: ops.stft_complex_out(x, N, NOV, WIN, FS, 1, 0, 1, True, Z),
                     B * (4 * L + 8 * F * T)),
    "istft": (lambda: ops.istft_out(Z, None, N, NOV, WIN, FS, 1, True, y),
              B * (8 * F * T + 4 * n_out)),
    "istft gain[F-1]": (lambda: ops.istft_out(Z, gain, N, NOV, WIN, FS, 1, True, y),
                        B * (8 * F * T + 4 * (F - 1) * T + 4 * n_out)),
}
times = sample({k: fn for k, (fn, _) in runs.items()}, ROUNDS, WARM)
ops.istft_out(Z, None, N, NOV, WIN, FS, 1, True, y)
rt = float((y[:, :L] - x).abs().max() / x.abs().max())
res = {"shape": {"batch": B, "length": L, "nperseg": N, "noverlap": NOV, "window": WIN,
                 "boundary": "zeros", "frames": T, "n_out": n_out},
       "rounds": ROUNDS, "hbm_bytes_per_s": HBM, "round_trip_normwise": rt, "kernels": {}}
base = statistics.median(times["stft_psd flags=0"])
for k, (_, alg) in runs.items():
    med, mn = statistics.median(times[k]), min(times[k])
    res["kernels"][k] = {"ms_median": med, "ms_min": mn, "algorithmic_bytes": alg,
                         "hbm_fraction": alg / (med * 1e-3) / HBM, "x_stft_psd": med / base}
    print(f"{k:18s} median {med:.4f} ms  min {mn:.4f} ms  {alg / med / 1e6:.0f} GB/s  "
          f"frac {alg / (med * 1e-3) / HBM:.3f}  x psd {med / base:.2f}", flush=True)
print(f"round trip max|istft(stft(x)) - x| / max|x| = {rt:.2e}")
write_json(res, path)
