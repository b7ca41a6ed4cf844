"""Time the fused cross-wavelet spectrum (csrc/filterbank_cross.hip) against the composition it
replaces: 128 Morlet scales at 16 voices an octave, the longest wavelet with L = 1024 (nfft
4096), in one process:

  B64    64 pairs x 65,536 samples, means over hop 128: three [128, 512] images a pair
  B1     one pair of the same length
  B1 1M  one pair of 2^20 samples, means over hop 2048

  cross        torch.ops.specenh.filterbank_cross_out on preallocated buffers: one launch
  layer        specenh.wavelet.cross_wavelet(mean=True) with a prebuilt FilterBank: the same plus
               the tensor layer's allocation
  composed     what it replaces: cwt(x) and cwt(y) at every sample (two launches of
               filterbank_kernel, each writing a complex [pairs, 128, length] tensor), the torch
               products conj(Wx) Wy, |Wx|^2, |Wy|^2, a reshape and the mean over each window.
               Run over all pairs at once unless --chunk N splits it over N pairs at a time
               (recorded in the result)
  scalogram    specenh.wavelet.scalogram of the 2 x pairs signals: the floor, the same count
               of inverse transforms with one block in flight a workgroup less

HIP events around each route, 3 warm-ups, interleaved rounds, median (and min). Alongside the
times: their ratios, the peak device memory each route holds (torch's allocator), the row
difference of the two routes, and the kernel's arithmetic rate, 5 nfft log2 nfft flops a
transform (2 S + 2 a block), as a fraction of the VALU ceiling at the v_fma_f32 issue rate
tools/micro/valu_rate.hip measures (2.9 cycles a wave instruction; an instruction counted as one
flop a lane). Also recorded: the kernels' resource usage (-Rpass-analysis=kernel-resource-usage).
    python tools/wavelet_coherence_bench.py [--json PATH] [--rounds N] [--chunk N]"""
import json
import math

from benchlib import measure, parse_args, resources, write_json  # puts the package on sys.path

import numpy as np
import torch
from specenh import _lib
from specenh import ops as host_ops
from specenh import wavelet as wv
from specenh.synthetic import plasma_chirps_torch

path, ROUNDS, rest = parse_args(7)
CHUNK = int(rest[rest.index("--chunk") + 1]) if "--chunk" in rest else 0
S, VOICES, LMAX, NFFT, WARM = 128, 16, 1024, 4096, 3
VALU_OPS = 256 * 4 * 64 / 2.9 * 2.4e9  # lane instructions a second at the v_fma_f32 issue rate
ops = torch.ops.specenh
SCALES = (LMAX / wv.SUPPORT) * 2.0 ** (-np.arange(S)[::-1] / VOICES)  # ascending, 1.04 .. 256
# (label, pairs, length, hop)
SHAPES = [("B64", 64, 65536, 128), ("B1", 1, 65536, 128), ("B1 1M", 1, 1 << 20, 2048)]


def composed(x, y, bank, hop, chunk):
    """(sxy, sxx, syy) by two cwt calls and torch; `chunk` pairs at a time (0: all)."""
    B, L = x.shape
    To = L // hop
    outs = []
    for b0 in range(0, B, chunk or B):
        b1 = min(B, b0 + (chunk or B))
        Wx = wv.cwt(x[b0:b1], SCALES, bank=bank)
        Wy = wv.cwt(y[b0:b1], SCALES, bank=bank)

        def mean(v):
            return v[..., :To * hop].reshape(v.shape[:-1] + (To, hop)).mean(-1)

        outs.append((mean(Wx.conj() * Wy), mean(Wx.real ** 2 + Wx.imag ** 2),
                     mean(Wy.real ** 2 + Wy.imag ** 2)))
        del Wx, Wy
    return tuple(torch.cat(o) for o in zip(*outs)) if len(outs) > 1 else outs[0]


def peak_bytes(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return int(peak)


def row_error(a, b, scale):
    """max over rows of max |a - b| / scale."""
    return float(((a - b).abs().amax(-1) / scale).max())


res = {"scales": S, "voices_per_octave": VOICES, "lmax": LMAX, "nfft": NFFT, "w0": wv.W0,
       "support": wv.SUPPORT, "scale_range_samples": [float(SCALES[0]), float(SCALES[-1])],
       "rounds": ROUNDS, "warmups": WARM, "valu_ceiling_lane_ops_per_s": VALU_OPS,
       "composition_chunk_pairs": CHUNK or "all pairs at once",
       "kernel_resources": resources("filterbank_cross.hip"), "shapes": {}}
print(json.dumps(res["kernel_resources"]), flush=True)
bank = wv.FilterBank(wv.morlet_filters(SCALES), nfft=NFFT, device="cuda")
assert bank.lmax == LMAX
for label, B, L, hop in SHAPES:
    gen = torch.Generator("cuda").manual_seed(2)
    x = plasma_chirps_torch(B, L, seed=1, device="cuda")
    x = x + 0.1 * torch.randn(x.shape, device="cuda", generator=gen)
    y = torch.roll(x, 3, dims=1) + 0.5 * torch.randn(x.shape, device="cuda", generator=gen)
    xy = torch.cat([x, y])
    To = L // hop
    sxy = torch.empty((B, S, To), device="cuda", dtype=torch.complex64)
    sxx, syy = torch.empty((B, S, To), device="cuda"), torch.empty((B, S, To), device="cuda")
    runs = {"cross": lambda: ops.filterbank_cross_out(x, y, bank.tables, LMAX, hop, _lib.XWT_MEAN,
                                                      sxy, sxx, syy),
            "layer": lambda: wv.cross_wavelet(x, y, SCALES, hop=hop, bank=bank),
            "composed": lambda: composed(x, y, bank, hop, CHUNK),
            "scalogram": lambda: wv.scalogram(xy, SCALES, hop=hop, bank=bank)}
    entry = {"pairs": B, "length": L, "hop": hop, "columns": To,
             "filters_per_workgroup": host_ops.filterbank_cross_chunk(S, NFFT, LMAX, B, L, hop,
                                                                      _lib.XWT_MEAN),
             "output_bytes": 16 * sxx.numel(),
             "composed_intermediate_bytes": 2 * 8 * (CHUNK or B) * S * L}
    entry.update(measure(runs, ROUNDS, WARM))
    Vh = bank.block(hop) // hop
    blocks = B * ((To + Vh - 1) // Vh)
    sc = entry["filters_per_workgroup"]
    chunks = (S + sc - 1) // sc
    flops = blocks * (2 * S + 2 * chunks) * 5.0 * NFFT * math.log2(NFFT)
    t = entry["cross_ms_median"] * 1e-3
    entry["blocks"] = blocks
    entry["transforms"] = blocks * (2 * S + 2 * chunks)
    entry["fft_flops"] = flops
    entry["cross_flops_per_s"] = flops / t
    entry["cross_over_valu_ceiling"] = flops / t / VALU_OPS
    entry["composed_over_cross"] = entry["composed_ms_median"] / entry["cross_ms_median"]
    entry["cross_over_scalogram"] = entry["cross_ms_median"] / entry["scalogram_ms_median"]
    entry["layer_peak_bytes"] = peak_bytes(runs["layer"])
    entry["composed_peak_bytes"] = peak_bytes(runs["composed"])
    runs["cross"]()
    ref = composed(x, y, bank, hop, CHUNK)
    top = (ref[1].amax(-1) * ref[2].amax(-1)).sqrt()
    entry["row_difference_from_composed"] = {
        "sxy_over_sqrt_max_sxx_max_syy": row_error(sxy, ref[0], top),
        "sxx_over_row_max": row_error(sxx, ref[1], ref[1].amax(-1)),
        "syy_over_row_max": row_error(syy, ref[2], ref[2].amax(-1))}
    print(f"{label:6s} " + "  ".join(f"{n} {entry[n + '_ms_median']:8.3f} ms" for n in runs)
          + f"  composed / cross {entry['composed_over_cross']:.2f}, cross / scalogram "
          f"{entry['cross_over_scalogram']:.2f}; {entry['cross_flops_per_s']:.3e} flop/s = "
          f"{entry['cross_over_valu_ceiling']:.3f} of the VALU ceiling; peak bytes layer "
          f"{entry['layer_peak_bytes']:.3e}, composed {entry['composed_peak_bytes']:.3e}; "
          f"differs from composed by {entry['row_difference_from_composed']}", flush=True)
    res["shapes"][label] = entry
    del x, y, xy, sxy, sxx, syy, ref, runs
    torch.cuda.empty_cache()
write_json(res, path)
