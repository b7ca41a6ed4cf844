"""Time the block-averaged cross-correlation (csrc/correlation.hip) at nperseg 1024 / noverlap
768 boxcar, constant detrend, maxlag 256, on 64 pairs of 65,536-sample shots (T = 253 frames),
whole-shot (navg 0) and as 31 blocks of 8 frames, in one process:

  correlation   torch.ops.specenh.correlation_out on preallocated buffers: the chunk kernel
                (and, whole-shot, the fold kernel)
  layer         specenh.correlation.correlate: the same plus the tensor layer's allocations
  auto          correlation_out with y = x: one signal loaded and transformed
  welch_csd     torch.ops.specenh.spectral_mean_out (pxx, pyy, pxy) on the same plan: the
                unpadded sibling, one N/2-point transform a frame instead of an N-point one
  torch         what it replaces: unfold -> detrend -> torch.fft.rfft(n = 2 N) -> conj(X) Y ->
                mean over the group -> irfft -> the lags, divided by sqrt(Ex Ey)

HIP events around each route, 3 warm-ups, interleaved rounds, median (and min). The algorithmic
traffic (the samples of both signals that enter a group read once, the lags and energies
written) over the correlation's time is reported as a fraction of the HBM ceiling of
tools/spectral_bench.py (8.0e12 B/s). A last table times the whole-shot call for 4 to 256
pairs: where it stops being flat is where every CU has as many workgroups as its LDS holds.
Also recorded: the agreement with the torch expression on the coefficient scale and the
kernels' resource usage (-Rpass-analysis=kernel-resource-usage).
    python tools/correlation_bench.py [--json PATH] [--rounds N]"""
import json

from benchlib import measure, parse_args, resources, write_json  # puts the package on sys.path

import torch
from specenh import correlation as co
from specenh import ops as sops
from specenh.synthetic import plasma_chirps_torch

path, ROUNDS, _ = parse_args(11)
N, NOV, WIN, FS, L, B, M = 1024, 768, "boxcar", 500000.0, 65536, 64, 256
HOP = N - NOV
T = (L - N) // HOP + 1
WARM, HBM = 3, 8.0e12
OP = (N, NOV, WIN, FS, 0, 1)  # density (unused), constant detrend
ops = torch.ops.specenh
SHAPES = [("B64 navg0", 0), ("B64 navg8", 8)]


def torch_rho(x, y, navg):
    """The definition in torch: rho [B, G, 2 M + 1] through per-frame padded spectra."""
    glen = navg or T
    G = T // glen

    def frames(s):
        f = s.unfold(1, N, HOP)[:, :G * glen]
        return f - f.mean(-1, keepdim=True)

    fx, fy = frames(x), frames(y)
    X, Y = torch.fft.rfft(fx, n=2 * N), torch.fft.rfft(fy, n=2 * N)
    C = (X.conj() * Y).view(B, G, glen, N + 1).mean(2)
    r = torch.fft.irfft(C, n=2 * N)
    r = torch.cat([r[..., 2 * N - M:], r[..., :M + 1]], dim=-1)
    ex = (fx * fx).sum(-1).view(B, G, glen).mean(-1)
    ey = (fy * fy).sum(-1).view(B, G, glen).mean(-1)
    return r / (ex * ey).sqrt().unsqueeze(-1)


res = {"plan": {"nperseg": N, "noverlap": NOV, "window": WIN, "detrend": "constant"},
       "length": L, "frames": T, "maxlag": M, "pairs": B, "rounds": ROUNDS, "warmups": WARM,
       "hbm_ceiling_bytes_per_s": HBM, "kernel_resources": resources("correlation.hip"),
       "shapes": {}}
print(json.dumps(res["kernel_resources"]), flush=True)
x, y = (plasma_chirps_torch(B, L, seed=s, device="cuda") for s in (1, 2))
y = 0.7 * torch.roll(x, 3, dims=1) + 0.5 * y  # partly coherent, as the parity tests
F = N // 2 + 1
for label, navg in SHAPES:
    G = 1 if navg <= 0 else T // navg
    used = G * (navg or T)
    out = torch.empty((B, G, 2 * M + 1), device="cuda")
    en = torch.empty((B, G, 2), device="cuda")
    ws = sops.correlation_workspace(x, y, *OP, navg, M)
    pxx, pyy = (torch.empty((B, F, G), device="cuda") for _ in range(2))
    pxy = torch.empty((B, F, G), dtype=torch.complex64, device="cuda")
    sws = sops.spectral_workspace(x, *OP, navg)
    kw = dict(fs=FS, window=WIN, nperseg=N, noverlap=NOV, detrend="constant", navg=navg, maxlag=M)
    runs = {"correlation": lambda: ops.correlation_out(x, y, *OP, navg, M, 1, out, en, ws),
            "layer": lambda: co.correlate(x, y, **kw),
            "auto": lambda: ops.correlation_out(x, x, *OP, navg, M, 1, out, en, ws),
            "welch_csd": lambda: ops.spectral_mean_out(x, y, *OP, navg, pxx, pyy, pxy, None, sws),
            "torch": lambda: torch_rho(x, y, navg)}
    entry = {"batch": B, "navg": navg, "groups": G, "frames_used": used,
             "workspace_bytes": int(ws.numel()) if ws.numel() > 1 else 0,
             "output_bytes": out.numel() * 4}
    entry.update(measure(runs, ROUNDS, WARM))
    samples = (used - 1) * HOP + N
    nbytes = B * (2 * samples * 4 + G * (2 * M + 1) * 4 + G * 8)
    entry["algorithmic_bytes"] = nbytes
    entry["correlation_bytes_per_s"] = nbytes / (entry["correlation_ms_median"] * 1e-3)
    entry["correlation_over_hbm_ceiling"] = entry["correlation_bytes_per_s"] / HBM
    entry["frame_pairs_per_s"] = B * used / (entry["correlation_ms_median"] * 1e-3)
    entry["torch_over_correlation"] = entry["torch_ms_median"] / entry["correlation_ms_median"]
    entry["correlation_over_welch_csd"] = (entry["correlation_ms_median"]
                                           / entry["welch_csd_ms_median"])
    ops.correlation_out(x, y, *OP, navg, M, 1, out, en, ws)
    diff = (out.double() - torch_rho(x, y, navg).double()).abs().max()
    entry["max_abs_difference_from_torch_on_the_coefficient_scale"] = float(diff)
    print(f"{label:10s} " + "  ".join(f"{n} {entry[n + '_ms_median']:8.3f} ms" for n in runs),
          flush=True)
    print(f"{label:10s} correlation {entry['correlation_bytes_per_s']:.3e} B/s = "
          f"{entry['correlation_over_hbm_ceiling']:.4f} of the HBM ceiling; "
          f"{entry['frame_pairs_per_s']:.3e} frame pairs/s; torch / correlation "
          f"{entry['torch_over_correlation']:.1f}; correlation / welch_csd "
          f"{entry['correlation_over_welch_csd']:.2f}; differs from torch by "
          f"{float(diff):.2e}", flush=True)
    res["shapes"][label] = entry
    del out, en, ws, pxx, pyy, pxy
# how the whole-shot call scales with the pairs: 8 chunk workgroups a pair
del x, y
res["whole_shot_scaling_us_median"] = {}
for pairs in (4, 16, 32, 64, 128, 256):
    xs, ys = (plasma_chirps_torch(pairs, L, seed=s, device="cuda") for s in (3, 4))
    out = torch.empty((pairs, 1, 2 * M + 1), device="cuda")
    ws = sops.correlation_workspace(xs, ys, *OP, 0, M)
    m = measure({"correlation": lambda: ops.correlation_out(xs, ys, *OP, 0, M, 1, out, None, ws)},
                ROUNDS, WARM)
    res["whole_shot_scaling_us_median"][str(pairs)] = m["correlation_ms_median"] * 1e3
    del xs, ys, out, ws
print("whole-shot: " + "  ".join(f"{p} pairs {t:7.1f} us"
                                 for p, t in res["whole_shot_scaling_us_median"].items()),
      flush=True)
write_json(res, path)
