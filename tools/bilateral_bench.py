"""Time the bilateral label filter (csrc/bilateral.hip) with the reference's (15, 75, 75), 149
taps, in one process:

  shot   20 x 256 x 3905   one shot's channels at the production shape
  C5     4096 x 128 x 128  the C5 batch

  u8       specenh_bilateral_u8 on a preallocated output: the tiled kernel alone
  layer    specenh.filters.bilateral on a float32 device batch: statistics, quantisation, the
           kernel, statistics, rescale, and the tensor layer's allocations
  torch    what it replaces, on as many images as fit comfortably: reflect-pad, unfold to the
           15 x 15 neighbourhoods, the disc's 149 columns, gather of the colour weights,
           weighted sums, division, round (float32)

HIP events around each route, 3 warm-ups, interleaved rounds, median (and min). Alongside the
times: tap-pixels a second, and that rate against two ceilings of the kernel's inner loop as the
compiler emits it (per tap and wave of 256 tap-pixels):
  VALU  38 wave instructions (per pixel: byte difference, its absolute value in two, the table
        address, the byte to float, product, sum, multiply-add; per tap: address arithmetic and
        the byte alignment), at the v_fma_f32 issue rate tools/micro/valu_rate.hip measures
        (2.9 cycles a wave instruction on each of a CU's four SIMDs);
  LDS   14 LDS-array cycles a CU (the uniform tap record 2, the two tile dwords 4, four
        conflict-free gathers 8).
The ceiling nearer to the measured rate is the one that binds. No counter profile is taken
here. Also recorded: how many pixels differ from the torch expression (both are float32
evaluations of one quotient; they may round a near-half apart) and the kernel's resource usage.
    python tools/bilateral_bench.py [--json PATH] [--rounds N]"""
import ctypes
import json

from benchlib import measure, parse_args, resources, write_json  # puts the package on sys.path

import numpy as np
import torch
import torch.nn.functional as F
from specenh import _lib, filters

path, ROUNDS, _ = parse_args(7)
WARM = 3
D, SC, SS = 15, 75.0, 75.0
CLOCK = 2.4e9
VALU_WAVE_INSTR_PER_TAP, LDS_CYCLES_PER_TAP, PIX_PER_WAVE_TAP = 38, 14, 256
VALU_TP = 256 * 4 / 2.9 * CLOCK / VALU_WAVE_INSTR_PER_TAP * PIX_PER_WAVE_TAP  # tap-pixels / s
LDS_TP = 256 * CLOCK / LDS_CYCLES_PER_TAP * PIX_PER_WAVE_TAP
# (label, images, rows, cols, images of the torch route)
SHAPES = [("shot", 20, 256, 3905, 1), ("C5", 4096, 128, 128, 16)]
L = _lib.lib()
r_, n_ = ctypes.c_int(), ctypes.c_int()
_lib.check(L.specenh_bilateral_taps(D, SS, ctypes.byref(r_), ctypes.byref(n_)))
R, TAPS = r_.value, n_.value


def host_tables():
    ii, jj = np.mgrid[-R:R + 1, -R:R + 1]
    disc = (ii * ii + jj * jj <= R * R).reshape(-1)
    sw = np.exp(-0.5 * (ii * ii + jj * jj).reshape(-1)[disc] / (SS * SS)).astype(np.float32)
    t = np.arange(256, dtype=np.float64)
    cw = np.exp(-0.5 * t * t / (SC * SC)).astype(np.float32)
    return (torch.from_numpy(np.flatnonzero(disc)).cuda(), torch.from_numpy(sw).cuda(),
            torch.from_numpy(cw).cuda())


DISC, SW, CW = host_tables()


def torch_bilateral_u8(u):
    """u [B, rows, cols] uint8 -> uint8, float32 sums in torch's reduction order."""
    B, rows, cols = u.shape
    x = F.pad(u.float()[:, None], (R, R, R, R), mode="reflect")
    nb = F.unfold(x, 2 * R + 1).index_select(1, DISC)               # [B, taps, rows * cols]
    c = u.float().reshape(B, 1, -1)
    w = SW[None, :, None] * CW[(nb - c).abs().long()]
    q = (nb * w).sum(1) / w.sum(1)
    return torch.round(q).to(torch.uint8).reshape(B, rows, cols)


def u8_call(img, out):
    B, rows, cols = img.shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.specenh_bilateral_u8(ctypes.c_void_p(img.data_ptr()), B, rows, cols, rows * cols,
                                      D, SC, SS, ctypes.c_void_p(out.data_ptr()), st), "u8")


res = {"d": D, "sigma_color": SC, "sigma_space": SS, "radius": R, "taps": TAPS,
       "tile": [_lib.BILATERAL_TILE_ROWS, _lib.BILATERAL_TILE_COLS], "rounds": ROUNDS,
       "warmups": WARM, "valu_ceiling_tap_pixels_per_s": VALU_TP,
       "lds_ceiling_tap_pixels_per_s": LDS_TP, "counter_profile": "not taken",
       "kernel_resources": resources("bilateral.hip"), "shapes": {}}
print(json.dumps(res["kernel_resources"]), flush=True)
for label, B, rows, cols, Bt in SHAPES:
    g = torch.Generator("cuda").manual_seed(1)
    S = torch.rand((B, rows, cols), device="cuda", generator=g)
    S = S * 0.3 + torch.exp(-0.5 * ((torch.arange(rows, device="cuda")[:, None] - rows / 2) / 3) ** 2)
    img = (filters.rescale(S) * 255).to(torch.uint8)
    out = torch.empty_like(img)
    runs = {"u8": lambda: u8_call(img, out), "layer": lambda: filters.bilateral(S),
            "torch": lambda: torch_bilateral_u8(img[:Bt])}
    entry = {"images": B, "rows": rows, "cols": cols, "torch_images": Bt}
    entry.update(measure(runs, ROUNDS, WARM))
    tp = B * rows * cols * TAPS
    t = entry["u8_ms_median"] * 1e-3
    entry["tap_pixels"] = tp
    entry["u8_tap_pixels_per_s"] = tp / t
    entry["u8_over_valu_ceiling"] = tp / t / VALU_TP
    entry["u8_over_lds_ceiling"] = tp / t / LDS_TP
    entry["binds"] = "VALU issue" if VALU_TP < LDS_TP else "LDS gather"
    entry["layer_over_u8"] = entry["layer_ms_median"] / entry["u8_ms_median"]
    entry["torch_ms_per_image"] = entry["torch_ms_median"] / Bt
    entry["torch_over_u8_per_image"] = entry["torch_ms_per_image"] / (entry["u8_ms_median"] / B)
    u8_call(img, out)
    ref = torch_bilateral_u8(img[:Bt])
    diff = (out[:Bt].int() - ref.int()).abs()
    entry["pixels_differing_from_torch"] = int((diff > 0).sum())
    entry["pixels_compared"] = int(diff.numel())
    entry["largest_difference_from_torch"] = int(diff.max())
    print(f"{label:5s} " + "  ".join(f"{n} {entry[n + '_ms_median']:9.3f} ms" for n in runs)
          + f" ({Bt} images)  {entry['u8_tap_pixels_per_s']:.3e} tap-pixels/s = "
          f"{entry['u8_over_valu_ceiling']:.3f} of the VALU ceiling, "
          f"{entry['u8_over_lds_ceiling']:.3f} of the LDS ceiling; layer / u8 "
          f"{entry['layer_over_u8']:.2f}; torch / u8 per image "
          f"{entry['torch_over_u8_per_image']:.1f}; {entry['pixels_differing_from_torch']} of "
          f"{entry['pixels_compared']} pixels differ from torch (by at most "
          f"{entry['largest_difference_from_torch']})", flush=True)
    res["shapes"][label] = entry
    del S, img, out, ref, diff, runs
    torch.cuda.empty_cache()
write_json(res, path)
