"""Time the bispectrum / squared bicoherence (csrc/bispectrum.hip) at nperseg 1024 / noverlap
768 hamm, linear detrend, on 65,536-sample shots (T = 253 frames, F = 513 bins, 131,841 bin
pairs with k + l <= 512), in one process:

  bicoherence   specenh.bispectrum.bispectrum(want=("bicoh",)) whole: transform + accumulate,
                auto (x alone) and cross (x, y, z), whole-shot (navg 0) and in 8-frame blocks,
                on the full plane and with nbins = 128
  accumulate    torch.ops.specenh.bispectrum_spectra_out alone on resident spectra [B, T, F]
  transform     the same call as `bicoherence` with nbins = 1: one tile per shot and group is
                left of the accumulate kernel, so this is the transform kernel and the launches
  torch         what it replaces: specenh.stft.stft(boundary=None, padded=False, scaling='psd')
                and the broadcasting expression of the definition ([b, F, F, T] temporaries), on
                the leading shots that fit, with `bicoherence` timed on those same shots

HIP events around each route, 3 warm-ups, interleaved rounds, median (and min). The batch of
a shape is chosen so that its outputs, [B, G, K, K] x 4 bytes (12 with the bispectrum), stay
below 1 GiB. The accumulate kernel's rate is reported in pair-frames a second (pairs of the
domain x frames x shots; the auto case computes half of them and mirrors) beside the derived
VALU ceiling 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz / 10 instructions = 7.9e12 a second.
Also recorded: the agreement of the kernel with the torch expression and the kernels'
resource usage (-Rpass-analysis=kernel-resource-usage).
    python tools/bispectrum_bench.py [--json PATH] [--rounds N]"""
import json

from benchlib import measure, parse_args, resources, write_json  # puts the package on sys.path

import torch
from specenh import bispectrum as bs
from specenh import stft
from specenh.synthetic import plasma_chirps_torch

path, ROUNDS, _ = parse_args(11)
N, NOV, WIN, FS, L = 1024, 768, "hamm", 500000.0, 65536
F, T = N // 2 + 1, (L - N) // (N - NOV) + 1
WARM = 3
CEILING = 256 * 4 * 32 * 2.4e9 / 10
KW = dict(fs=FS, window=WIN, nperseg=N, noverlap=NOV, detrend="linear", scaling="density")
ops = torch.ops.specenh
# (label, B, navg, nbins)
SHAPES = [("B64 navg0 full", 64, 0, None), ("B8 navg8 full", 8, 8, None),
          ("B64 navg0 nbins128", 64, 0, 128), ("B64 navg8 nbins128", 64, 8, 128)]
TORCH_SHOTS = 2  # [b, 513, 513, 253] complex64 is 0.53 GB a shot and temporary


def torch_bicoherence(x, y, z):
    """The definition by broadcasting on per-frame spectra: b2 [b, F, F]."""
    Z = [stft.stft(s, fs=FS, window=WIN, nperseg=N, noverlap=NOV, detrend="linear",
                   boundary=None, padded=False, scaling="psd")[2] for s in (x, y, z)]
    k = torch.arange(F, device=x.device)
    m = k[:, None] + k[None, :]
    P = Z[0][:, :, None, :] * Z[1][:, None, :, :]
    Zm = Z[2][:, m.clamp(max=F - 1), :]
    Bs = (P * Zm.conj()).mean(-1)
    b2 = Bs.abs() ** 2 / ((P.abs() ** 2).mean(-1) * (Zm.abs() ** 2).mean(-1))
    return torch.where(m <= F - 1, b2, torch.zeros_like(b2))


pairs = F * (F + 1) // 2
res = {"plan": {"nperseg": N, "noverlap": NOV, "window": WIN, "detrend": "linear",
                "scaling": "density"}, "length": L, "frames": T, "bins": F, "domain_pairs": pairs,
       "rounds": ROUNDS, "warmups": WARM, "valu_ceiling_pair_frames_per_s": CEILING,
       "kernel_resources": resources("bispectrum.hip"), "shapes": {}}
print(json.dumps(res["kernel_resources"]), flush=True)
for label, B, navg, nbins in SHAPES:
    x, y = (plasma_chirps_torch(B, L, seed=s, device="cuda") for s in (1, 2))
    z = x * y + 0.3 * x
    K = nbins or F
    G = 1 if navg <= 0 else T // navg
    used = G * (navg or T)
    X, Y, Z = (stft.stft(s, fs=FS, window=WIN, nperseg=N, noverlap=NOV, detrend="linear",
                         boundary=None, padded=False, scaling="psd")[2].transpose(1, 2)
               .contiguous() for s in (x, y, z))
    out = torch.empty((B, G, K, K), device="cuda")
    kw = dict(navg=navg, nbins=nbins, want=("bicoh",), **KW)
    runs = {"bicoherence_auto": lambda: bs.bispectrum(x, **kw),
            "bicoherence_cross": lambda: bs.bispectrum(x, y, z, **kw),
            "accumulate_auto": lambda: ops.bispectrum_spectra_out(X, None, None, navg, K, None, out),
            "accumulate_cross": lambda: ops.bispectrum_spectra_out(X, Y, Z, navg, K, None, out),
            "transform_auto": lambda: bs.bispectrum(x, **dict(kw, nbins=1)),
            "transform_cross": lambda: bs.bispectrum(x, y, z, **dict(kw, nbins=1))}
    entry = {"batch": B, "navg": navg, "groups": G, "nbins": K, "frames_used": used,
             "output_bytes": out.numel() * 4}
    entry.update(measure(runs, ROUNDS, WARM))
    k = torch.arange(K)
    inside = int((k[:, None] + k[None, :] <= F - 1).sum())
    entry["pair_frames"] = inside * used * B
    for which in ("auto", "cross"):
        entry[f"accumulate_{which}_pair_frames_per_s"] = \
            entry["pair_frames"] / (entry[f"accumulate_{which}_ms_median"] * 1e-3)
        entry[f"accumulate_{which}_over_ceiling"] = \
            entry[f"accumulate_{which}_pair_frames_per_s"] / CEILING
    print(f"{label:20s} " + "  ".join(f"{n} {entry[n + '_ms_median']:8.3f} ms" for n in runs),
          flush=True)
    print(f"{label:20s} accumulate rate auto {entry['accumulate_auto_pair_frames_per_s']:.3e} "
          f"cross {entry['accumulate_cross_pair_frames_per_s']:.3e} pair-frames/s "
          f"(ceiling {CEILING:.2e})", flush=True)
    if navg == 0 and nbins is None:  # what it replaces, on the shots that fit
        b = TORCH_SHOTS
        xs, ys, zs = x[:b], y[:b], z[:b]
        base = measure({"torch_cross": lambda: torch_bicoherence(xs, ys, zs),
                        "bicoherence_cross_same_shots": lambda: bs.bispectrum(xs, ys, zs, **kw)},
                       ROUNDS, WARM)
        base["shots"] = b
        base["torch_over_bicoherence"] = (base["torch_cross_ms_median"]
                                          / base["bicoherence_cross_same_shots_ms_median"])
        got = bs.bispectrum(xs, ys, zs, **kw)[2]["bicoh"][:, 0]
        base["max_abs_difference"] = float((got - torch_bicoherence(xs, ys, zs)).abs().max())
        entry["torch_baseline"] = base
        print(f"{label:20s} torch on {b} shots {base['torch_cross_ms_median']:.3f} ms, kernels "
              f"{base['bicoherence_cross_same_shots_ms_median']:.3f} ms, max |difference| "
              f"{base['max_abs_difference']:.2e}", flush=True)
    res["shapes"][label] = entry
    del x, y, z, X, Y, Z, out
    torch.cuda.empty_cache()
write_json(res, path)
