"""Time the cross-spectral matrix of a channel array (specenh_csm: every frame transformed
once, then a Gram product per bin on the fp32 matrix cores) against the route it replaces, in
the same run: C (C - 1) / 2 calls of spectral_mean for the cross spectra of the pairs plus C
calls for the Welch PSDs of the diagonal (nperseg 1024 / noverlap 768 hamm, linear detrend,
density). HIP events around each route, a warm-up, interleaved rounds, median (and min). The
split between the two kernels comes from one torch.profiler pass of their own; the Gram
kernel's rate is the MFMA work it issues (32x32 tiles, padded channels included) and the work
of the upper triangle alone, over its time, against the 157 TF fp32 peak.
    python tools/csm_bench.py [--json PATH] [--rounds N]"""
import statistics

from benchlib import parse_args, sample, write_json  # puts the package on sys.path

import torch
from specenh import ops as _ops
from specenh import spectral, stft
from specenh.synthetic import plasma_chirps_torch

path, ROUNDS, _ = parse_args(11)
N, NOV, WIN, FS = 1024, 768, "hamm", 500000.0
DENSITY, LINEAR = 0, 2
WARM, PEAK = 3, 157.0e12
F = N // 2 + 1
PLAN = (N, NOV, WIN, FS, DENSITY, LINEAR)
ops = torch.ops.specenh
# (label, B, C, L, navg)
SHAPES = [("B8 C40 L65536 navg0", 8, 40, 65536, 0),
          ("B8 C40 L65536 navg8", 8, 40, 65536, 8),
          ("B1 C40 L1048576 navg0", 1, 40, 1 << 20, 0),
          ("B8 C4 L65536 navg0", 8, 4, 65536, 0)]


def kernel_split(fn):
    """Device time of the two kernels of one call, from a profiler pass of its own."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for name in ("csm_transform_kernel", "csm_gram_kernel"):
                if name in ev.key:
                    t = getattr(ev, "device_time_total", None)
                    if t is None:
                        t = ev.cuda_time_total
                    out[name] = out.get(name, 0.0) + t / 1e3  # us -> ms
        return out if len(out) == 2 else None
    except Exception as e:  # the profiler is optional: the split is then not reported
        print(f"kernel split not measured: {e!r}")
        return None


res = {"plan": {"nperseg": N, "noverlap": NOV, "window": WIN, "detrend": "linear",
                "scaling": "density"}, "rounds": ROUNDS, "fp32_peak_flops": PEAK, "shapes": {}}
for label, B, C, L, navg in SHAPES:
    x = plasma_chirps_torch(B * C, L, seed=1, device="cuda").reshape(B, C, L)
    T = stft.frame_count(L, N, NOV)
    G = spectral.group_count(T, navg)
    Tu = G * (navg if navg >= 1 else T)
    shape = (B, F, G, C, C)
    S = torch.empty(shape, dtype=torch.complex64, device="cuda")
    K = torch.empty(shape, device="cuda")
    ws = _ops.csm_workspace(x, *PLAN, navg)
    rows = [x[:, c] for c in range(C)]  # [B, L] views, row stride C L
    pw = _ops.spectral_workspace(rows[0], *PLAN, navg)
    pxy = torch.empty((B, F, G), dtype=torch.complex64, device="cuda")
    pxx = torch.empty((B, F, G), device="cuda")

    def matrix():
        ops.csm_out(x, *PLAN, navg, S, K, ws)

    def pairs():
        for i in range(C):
            ops.spectral_mean_out(rows[i], None, *PLAN, navg, pxx, None, None, None, pw)
            for j in range(i + 1, C):
                ops.spectral_mean_out(rows[i], rows[j], *PLAN, navg, None, None, pxy, None, pw)

    runs = {"csm": matrix, "pair route": pairs}
    times = sample(runs, ROUNDS, WARM)
    # agreement of the two routes on one pair and one diagonal element
    matrix()
    ops.spectral_mean_out(rows[1], rows[C - 1], *PLAN, navg, None, None, pxy, None, pw)
    ops.spectral_mean_out(rows[2], None, *PLAN, navg, pxx, None, None, None, pw)
    agree = {
        "pxy_normwise": float(((S[..., 1, C - 1] - pxy).abs().amax(1) / pxy.abs().amax(1)).max()),
        "pxx_normwise": float(((S[..., 2, 2].real - pxx).abs().amax(1) / pxx.amax(1)).max())}
    med = {k: statistics.median(v) for k, v in times.items()}
    split = kernel_split(matrix)
    ntp = 1 if C <= 32 else 3
    issued = B * G * F * ntp * (Tu // G + 1) // 2 * 4 * (2 * 32 * 32 * 2)  # 4 MFMAs a frame pair
    useful = 8.0 * B * F * Tu * C * (C + 1) / 2
    entry = {"batch": B, "channels": C, "length": L, "navg": navg, "frames": T, "groups": G,
             "workspace_bytes": int(ws.numel()),
             "csm_ms_median": med["csm"], "csm_ms_min": min(times["csm"]),
             "pair_route_ms_median": med["pair route"],
             "pair_route_ms_min": min(times["pair route"]),
             "pair_route_launches": C * (C + 1) // 2,
             "speedup_over_pair_route": med["pair route"] / med["csm"],
             "fft_count_ratio": C - 1 + 1.0 / C,  # frames transformed: pair route / csm
             "agreement_with_pair_route": agree,
             "kernel_ms": split}
    if split:
        t = split["csm_gram_kernel"] * 1e-3
        entry["gram_issued_flops"] = issued
        entry["gram_issued_fraction_of_peak"] = issued / t / PEAK
        entry["gram_upper_triangle_fraction_of_peak"] = useful / t / PEAK
    res["shapes"][label] = entry
    print(f"{label:24s} csm {med['csm']:9.4f} ms  pair route {med['pair route']:10.4f} ms  "
          f"x{entry['speedup_over_pair_route']:.1f} (FFT-count ratio {entry['fft_count_ratio']:.1f})"
          f"  split {split}  workspace {ws.numel() / 1e6:.0f} MB  agree {agree}", flush=True)
    del x, S, K, ws, rows
    torch.cuda.empty_cache()
write_json(res, path)
