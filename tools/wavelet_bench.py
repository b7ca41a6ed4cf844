"""Time the Morlet scalogram and wavelet transform (csrc/filterbank.hip): 128 scales at 16
voices an octave, the longest wavelet with L = 1024 (scales 256 .. 1.04 samples, nfft 4096), in
one process:

  B64 mean     64 shots x 65,536 samples, mean power over hop 128: a [128, 512] image a shot
  B1 1M mean   one 2^20-sample shot, mean power over hop 2048: [128, 512]
  B4 complex   4 shots x 65,536 samples, the complex transform at every sample (hop 1)

  filterbank   torch.ops.specenh.filterbank_out on a preallocated buffer: one launch
  layer        specenh.wavelet.scalogram / cwt with a prebuilt FilterBank: the same plus the
               tensor layer's allocation
  torch        what it replaces: whole-shot torch.fft.rfft padded to a power of two, the
               broadcast product with whole-length tables of the wavelets (the non-negative
               frequencies: the analytic-wavelet shortcut of Torrence & Compo eq. 4-6),
               torch.fft.ifft, then abs() ** 2 and the hop mean

HIP events around each route, 3 warm-ups, interleaved rounds, median (and min). Alongside the
times: their ratio, the peak device memory each route holds (torch's allocator), and the
kernel's arithmetic rate, 5 nfft log2 nfft flops per scale and block, as a fraction of the VALU
ceiling at the v_fma_f32 issue rate tools/micro/valu_rate.hip measures (2.9 cycles a wave
instruction; an instruction counted as one flop a lane). The torch expression drops the
wavelets' negative-frequency response, so the agreement is recorded twice: against it on the
scales of 4 samples and more (below, the wavelet's band folds over Nyquist and the shortcut
does not compute the definition), and on one shot at every scale against the full-spectrum
torch.fft.fft form.
A last table times the mean-power call for 1 to 64 shots: a single shot must already fill the
chip. Also recorded: the kernels' resource usage (-Rpass-analysis=kernel-resource-usage).
    python tools/wavelet_bench.py [--json PATH] [--rounds N]"""
import json
import math

from benchlib import measure, parse_args, resources, write_json  # puts the package on sys.path

import numpy as np
import torch
from specenh import _lib
from specenh import wavelet as wv
from specenh.synthetic import plasma_chirps_torch

path, ROUNDS, _ = parse_args(7)
S, VOICES, LMAX, NFFT, WARM = 128, 16, 1024, 4096, 3
VALU_OPS = 256 * 4 * 64 / 2.9 * 2.4e9  # lane instructions a second at the v_fma_f32 issue rate
ops = torch.ops.specenh
SCALES = (LMAX / wv.SUPPORT) * 2.0 ** (-np.arange(S)[::-1] / VOICES)  # ascending, 1.04 .. 256
TAPS = wv.morlet_filters(SCALES)
assert max(h.size // 2 for h in TAPS) == LMAX
# Below s = 4 samples the wavelet's band (centre w0 / s rad a sample, width 1 / s) reaches past
# Nyquist and folds onto negative frequencies: the half-spectrum shortcut of the torch
# expression does not compute the definition there, so it is compared on the scales from 4 up.
ANALYTIC = int(np.searchsorted(SCALES, 4.0))
# (label, shots, length, hop, mode)
SHAPES = [("B64 mean", 64, 65536, 128, "mean_power"), ("B1 1M mean", 1, 1 << 20, 2048, "mean_power"),
          ("B4 complex", 4, 65536, 1, "complex")]


def whole_tables(npad):
    """[S, npad] complex64 on the host: the DFT of the wavelets wrapped circularly at the
    padded length (fp64, 16 wavelets at a time)."""
    out = np.empty((S, npad), dtype=np.complex64)
    for s0 in range(0, S, 16):
        H = np.zeros((16, npad), dtype=np.complex128)
        for i, h in enumerate(TAPS[s0:s0 + 16]):
            L = h.size // 2
            H[i, np.arange(-L, L + 1) % npad] = h
        out[s0:s0 + 16] = np.fft.fft(H, axis=-1)
    return out


def torch_cwt(x, Hpos, npad, hop, mode):
    X = torch.fft.rfft(x, n=npad)
    W = torch.fft.ifft(X[:, None, :] * Hpos[None], n=npad)[..., :x.shape[1]]
    if mode == "complex":
        return W[..., ::hop]
    P = W.abs() ** 2
    To = x.shape[1] // hop
    return P[..., :To * hop].reshape(P.shape[:-1] + (To, hop)).mean(-1)


def torch_cwt_full(x, Hfull, npad):
    X = torch.fft.fft(x, n=npad)
    return torch.fft.ifft(X[:, None, :] * Hfull[None])[..., :x.shape[1]]


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return int(peak)


def row_error(a, b):
    """max over rows of max |a - b| / max |b|."""
    return float(((a - b).abs().amax(-1) / b.abs().amax(-1)).max())


res = {"scales": S, "voices_per_octave": VOICES, "lmax": LMAX, "nfft": NFFT, "w0": wv.W0,
       "support": wv.SUPPORT, "scale_range_samples": [float(SCALES[0]), float(SCALES[-1])],
       "rounds": ROUNDS, "warmups": WARM, "valu_ceiling_lane_ops_per_s": VALU_OPS,
       "half_spectrum_compared_from_scale_index": ANALYTIC,
       "kernel_resources": resources("filterbank.hip"), "shapes": {}}
print(json.dumps(res["kernel_resources"]), flush=True)
bank = wv.FilterBank(TAPS, nfft=NFFT, device="cuda")
KIND = {"mean_power": _lib.FB_POWER_MEAN, "complex": _lib.FB_COMPLEX}
for label, B, L, hop, mode in SHAPES:
    x = plasma_chirps_torch(B, L, seed=1, device="cuda")
    x = x + 0.1 * torch.randn(x.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    npad = 1 << math.ceil(math.log2(L + LMAX))
    Hhost = whole_tables(npad)
    Hpos = torch.from_numpy(np.ascontiguousarray(Hhost[:, :npad // 2 + 1])).cuda()
    To = L // hop if mode == "mean_power" else (L - 1) // hop + 1
    out = torch.empty((B, S, To), device="cuda",
                      dtype=torch.complex64 if mode == "complex" else torch.float32)
    layer = ((lambda: wv.scalogram(x, SCALES, hop=hop, bank=bank)) if mode == "mean_power"
             else (lambda: wv.cwt(x, SCALES, hop=hop, bank=bank)))
    runs = {"filterbank": lambda: ops.filterbank_out(x, bank.tables, LMAX, hop, KIND[mode], out),
            "layer": layer,
            "torch": lambda: torch_cwt(x, Hpos, npad, hop, mode)}
    entry = {"shots": B, "length": L, "hop": hop, "mode": mode, "columns": To,
             "torch_padded_length": npad, "output_bytes": out.numel() * out.element_size()}
    entry.update(measure(runs, ROUNDS, WARM))
    V = bank.block(hop)
    blocks = B * ((To + V // hop - 1) // (V // hop))
    flops = blocks * S * 5.0 * NFFT * math.log2(NFFT)
    t = entry["filterbank_ms_median"] * 1e-3
    entry["blocks"] = blocks
    entry["fft_flops"] = flops
    entry["filterbank_flops_per_s"] = flops / t
    entry["filterbank_over_valu_ceiling"] = flops / t / VALU_OPS
    entry["torch_over_filterbank"] = entry["torch_ms_median"] / entry["filterbank_ms_median"]
    entry["filterbank_bytes_held"] = (x.numel() * 4 + bank.tables.numel() * 8
                                      + out.numel() * out.element_size())
    entry["torch_tables_bytes"] = Hpos.numel() * 8
    entry["layer_peak_bytes"] = peak_bytes(layer)
    entry["torch_peak_bytes"] = peak_bytes(runs["torch"])
    runs["filterbank"]()
    ref = torch_cwt(x, Hpos, npad, hop, mode)
    entry["row_difference_from_torch_half_spectrum"] = row_error(out[:, ANALYTIC:], ref[:, ANALYTIC:])
    del ref
    full = torch_cwt_full(x[:1], torch.from_numpy(Hhost).cuda(), npad)
    if mode == "complex":
        full = full[..., ::hop]
    else:
        P = full.abs() ** 2
        full = P[..., :To * hop].reshape(P.shape[:-1] + (To, hop)).mean(-1)
    entry["row_difference_from_torch_full_spectrum_one_shot"] = row_error(out[:1], full)
    print(f"{label:11s} " + "  ".join(f"{n} {entry[n + '_ms_median']:8.3f} ms" for n in runs)
          + f"  torch / filterbank {entry['torch_over_filterbank']:.2f}; "
          f"{entry['filterbank_flops_per_s']:.3e} flop/s = "
          f"{entry['filterbank_over_valu_ceiling']:.3f} of the VALU ceiling; peak bytes layer "
          f"{entry['layer_peak_bytes']:.3e}, torch {entry['torch_peak_bytes']:.3e}; differs from "
          f"torch by {entry['row_difference_from_torch_half_spectrum']:.2e} (half spectrum), "
          f"{entry['row_difference_from_torch_full_spectrum_one_shot']:.2e} (full, one shot)",
          flush=True)
    res["shapes"][label] = entry
    del x, out, Hpos, Hhost, full, runs, layer
    torch.cuda.empty_cache()
# how the mean-power call scales with the shots: 32 blocks a shot of 65,536 samples
res["mean_power_scaling_us_median"] = {}
for shots in (1, 2, 4, 16, 64):
    xs = plasma_chirps_torch(shots, 65536, seed=3, device="cuda")
    out = torch.empty((shots, S, 512), device="cuda")
    m = measure({"filterbank": lambda: ops.filterbank_out(xs, bank.tables, LMAX, 128,
                                                          _lib.FB_POWER_MEAN, out)}, ROUNDS, WARM)
    res["mean_power_scaling_us_median"][str(shots)] = m["filterbank_ms_median"] * 1e3
    del xs, out
print("mean power, 65,536 samples: " + "  ".join(
    f"{p} shots {t:8.1f} us" for p, t in res["mean_power_scaling_us_median"].items()), flush=True)
write_json(res, path)
