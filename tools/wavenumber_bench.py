"""Time the two-point wavenumber-frequency spectrum S(k, f) (csrc/wavenumber.hip) at nperseg
1024 / noverlap 768 hamm, constant detrend, nk = 64, on 64 pairs of 65,536-sample shots
(T = 253 frames, F = 513 bins), whole-shot (navg 0) and in 8-frame blocks, in one process:

  wavenumber    specenh.wavenumber.wavenumber_spectrum whole: transform + accumulate
  accumulate    torch.ops.specenh.wavenumber_spectra_out alone on resident spectra [B, T, F]
  transform     specenh.bispectrum.bispectrum(x, y, nbins=1): the shared transform of both
                signals (transform_frames) and one tile per shot and group of another kernel,
                so this is the transform kernel and the launches
  torch         what it replaces: specenh.stft.stft(boundary=None, padded=False, scaling='psd')
                of both signals, atan2, and index_add_ over the [B, T, F] temporary

HIP events around each route, 3 warm-ups, interleaved rounds, median (and min). The accumulate
kernel's algorithmic traffic, 2 * Tu * F * 8 bytes read and G * F * K * 4 written per pair, over
its time is reported as a fraction of the HBM ceiling of tools/spectral_bench.py (8.0e12 B/s).
A last table times the accumulate kernel alone, whole-shot, for 4 to 256 pairs and nk 16, 64,
256: where it stops being flat is where every CU has as many waves as its LDS holds.
Also recorded: the agreement of the kernel with the torch expression (rows that differ by more
than 1e-5 of their total are rows where rounding moved a frame across a bin edge) and the
kernels' resource usage (-Rpass-analysis=kernel-resource-usage).
    python tools/wavenumber_bench.py [--json PATH] [--rounds N]"""
import json
import math

from benchlib import measure, parse_args, resources, write_json  # puts the package on sys.path

import torch
from specenh import bispectrum as bs
from specenh import stft
from specenh import wavenumber as wn
from specenh.synthetic import plasma_chirps_torch

path, ROUNDS, _ = parse_args(11)
N, NOV, WIN, FS, L, B, NK = 1024, 768, "hamm", 500000.0, 65536, 64, 64
F, T = N // 2 + 1, (L - N) // (N - NOV) + 1
WARM, HBM = 3, 8.0e12
KW = dict(fs=FS, window=WIN, nperseg=N, noverlap=NOV, detrend="constant", scaling="density")
ops = torch.ops.specenh
SHAPES = [("B64 navg0", 0), ("B64 navg8", 8)]


def spectra(s):
    return stft.stft(s, fs=FS, window=WIN, nperseg=N, noverlap=NOV, detrend="constant",
                     boundary=None, padded=False, scaling="psd")[2]  # [B, F, T]


def torch_skf(x, y, navg):
    """The definition in torch: S [B, G, F, K] by atan2 and a scatter-add."""
    X, Y = spectra(x), spectra(y)
    glen = navg or T
    G = T // glen
    X, Y = X[:, :, :G * glen], Y[:, :, :G * glen]
    c = X.conj() * Y
    j = (torch.round(torch.atan2(c.imag, c.real) * (NK / (2 * math.pi))).long() + NK // 2) % NK
    o = torch.full((F, 1), 2.0, device=x.device)
    o[0] = o[F - 1] = 1.0
    w = o * (X.real ** 2 + X.imag ** 2 + Y.real ** 2 + Y.imag ** 2) / (2 * glen)
    b = torch.arange(B, device=x.device)[:, None, None]
    f = torch.arange(F, device=x.device)[None, :, None]
    g = (torch.arange(G * glen, device=x.device) // glen)[None, None, :]
    idx = ((b * G + g) * F + f) * NK + j
    out = torch.zeros(B * G * F * NK, device=x.device)
    out.index_add_(0, idx.reshape(-1), w.reshape(-1))
    return out.view(B, G, F, NK)


res = {"plan": {"nperseg": N, "noverlap": NOV, "window": WIN, "detrend": "constant",
                "scaling": "density"}, "length": L, "frames": T, "bins": F, "nk": NK, "pairs": B,
       "rounds": ROUNDS, "warmups": WARM, "hbm_ceiling_bytes_per_s": HBM,
       "kernel_resources": resources("wavenumber.hip"), "shapes": {}}
print(json.dumps(res["kernel_resources"]), flush=True)
x, y = (plasma_chirps_torch(B, L, seed=s, device="cuda") for s in (1, 2))
y = 0.7 * torch.roll(x, 3, dims=1) + 0.5 * y  # partly coherent, as the parity tests
X, Y = (spectra(s).transpose(1, 2).contiguous() for s in (x, y))
for label, navg in SHAPES:
    G = 1 if navg <= 0 else T // navg
    used = G * (navg or T)
    out = torch.empty((B, G, F, NK), device="cuda")
    kw = dict(navg=navg, nk=NK, **KW)
    runs = {"wavenumber": lambda: wn.wavenumber_spectrum(x, y, **kw),
            "accumulate": lambda: ops.wavenumber_spectra_out(X, Y, navg, NK, out),
            "transform": lambda: bs.bispectrum(x, y, None, navg=navg, nbins=1, want=("bicoh",),
                                               **KW),
            "torch": lambda: torch_skf(x, y, navg)}
    entry = {"batch": B, "navg": navg, "groups": G, "frames_used": used,
             "output_bytes": out.numel() * 4}
    entry.update(measure(runs, ROUNDS, WARM))
    nbytes = B * (2 * used * F * 8 + G * F * NK * 4)
    entry["accumulate_bytes"] = nbytes
    entry["accumulate_bytes_per_s"] = nbytes / (entry["accumulate_ms_median"] * 1e-3)
    entry["accumulate_over_hbm_ceiling"] = entry["accumulate_bytes_per_s"] / HBM
    entry["torch_over_wavenumber"] = entry["torch_ms_median"] / entry["wavenumber_ms_median"]
    got, ref = wn.wavenumber_spectrum(x, y, **kw)[3].double(), torch_skf(x, y, navg).double()
    rows = (got - ref).abs().sum(-1) > 1e-5 * ref.sum(-1)
    entry["rows"] = rows.numel()
    entry["rows_differing_from_torch"] = int(rows.sum())
    same = (got - ref).abs() * (~rows)[..., None]
    entry["max_abs_difference_over_max_other_rows"] = float(same.max() / ref.max())
    print(f"{label:10s} " + "  ".join(f"{n} {entry[n + '_ms_median']:8.3f} ms" for n in runs),
          flush=True)
    print(f"{label:10s} accumulate {entry['accumulate_bytes_per_s']:.3e} B/s = "
          f"{entry['accumulate_over_hbm_ceiling']:.3f} of the HBM ceiling; torch / wavenumber "
          f"{entry['torch_over_wavenumber']:.1f}; {entry['rows_differing_from_torch']} of "
          f"{entry['rows']} rows differ from torch, the others by "
          f"{entry['max_abs_difference_over_max_other_rows']:.2e}", flush=True)
    res["shapes"][label] = entry
    del out
# how the accumulate kernel alone scales with the pairs (9 tiles of 64 bins each) and with nk
del x, y, X, Y
res["accumulate_scaling_us_median"] = {}
gen = torch.Generator(device="cuda")
gen.manual_seed(3)
for nk in (16, 64, 256):
    row = {}
    for pairs in (4, 16, 28, 56, 64, 128, 256):
        X, Y = (torch.view_as_complex(torch.randn(pairs, T, F, 2, device="cuda", generator=gen))
                for _ in range(2))
        out = torch.empty((pairs, 1, F, nk), device="cuda")
        m = measure({"accumulate": lambda: ops.wavenumber_spectra_out(X, Y, 0, nk, out)},
                    ROUNDS, WARM)
        row[str(pairs)] = m["accumulate_ms_median"] * 1e3
    res["accumulate_scaling_us_median"][str(nk)] = row
    print(f"accumulate alone, whole-shot, nk {nk:3d}: " +
          "  ".join(f"{p} pairs {t:6.1f} us" for p, t in row.items()), flush=True)
write_json(res, path)
