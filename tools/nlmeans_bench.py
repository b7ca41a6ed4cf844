"""Time non-local means (csrc/nlmeans.hip) with scikit-image's defaults (patch_size 7,
patch_distance 11: 23 x 23 = 529 shifts, h 0.1, sigma 0), in one process:

  shot   20 x 256 x 3905   one shot's channels at the production shape
  C5     4096 x 128 x 128  the C5 stream

  kernel   specenh_nlmeans on a preallocated output: the tiled kernel alone
  layer    specenh.filters.nl_means on a float32 device batch: the kernel and the tensor
           layer's allocation
  torch    what it replaces, on as many images as fit comfortably: a loop over the shifts of
           the shifted view of the reflect-padded image, difference, square, avg_pool2d over the
           patch, exp, two accumulations; one division (float32)

HIP events around each route, 3 warm-ups, interleaved rounds, median (and min). The kernel is
timed twice a round, first (right after the previous round's torch route and its thousands of
small launches) and again after the layer route, into a fresh output: the two tell an effect of
the route order or of the output buffer from a cost of the kernel. Alongside the times:
shift-pixels a second, and that rate against two ceilings of the kernel's shift loop (patch_size
7, float32), counted here from the ISA the installed compiler emits with the library's flags, per
shift and wave (256 shift-pixels, a lane's four pixels):
  VALU  the loop's vector instructions, a packed one (v_pk_*) counted twice, at the v_fma_f32
        issue rate tools/micro/valu_rate.hip measures (2.9 cycles a wave instruction on each of
        a CU's four SIMDs). With hipcc of ROCm 7.2.0 (AMD clang 22.0.0git) it is 194: 70
        differences, 10 squares and 60 multiply-adds into the ten row sums, 24 additions into
        the four patch sums, per pixel the scale multiply-add, the floor, the exponential, the
        addition and the multiply-add of the two chains, and 10 for the five LDS addresses;
  LDS   the LDS-array cycles of the loop's reads a CU (ds_read_b32 2, ds_read2_b32 4, ...): 140
        with that compiler (35 reads of two dwords a lane).
Another compiler allocates and schedules differently; the counts, the compiler's version and the
kernels' resource usage are written into the result. The ceiling nearer to the measured rate is
the one that binds. No counter profile is taken here. Also recorded: the largest difference from
the torch expression (both are float32 evaluations of one quotient).
    python tools/nlmeans_bench.py [--json PATH] [--rounds N]"""
import collections
import ctypes
import json
import os
import re
import subprocess
import tempfile

from benchlib import measure, parse_args, resources, write_json  # puts the package on sys.path

import torch
import torch.nn.functional as F
from specenh import _lib, filters

path, ROUNDS, _ = parse_args(5)
WARM = 3
P, D, H, SIGMA = 7, 11, 0.1, 0.0
SHIFTS = (2 * D + 1) ** 2
CLOCK = 2.4e9
PIX_PER_WAVE_SHIFT = 256
# LDS-array cycles of a wave's read, conflict-free
LDS_READ_CYCLES = {"ds_read_b32": 2, "ds_read_b64": 2, "ds_read_b96": 8, "ds_read_b128": 4,
                   "ds_read2_b32": 4, "ds_read2_b64": 8, "ds_read2st64_b32": 4,
                   "ds_read2st64_b64": 8}


def shift_loop_counts():
    """(VALU wave instructions, LDS cycles, {mnemonic: count}, compiler version) of the shift
    loop of nlmeans_kernel<float, 7>: the innermost loop of its ISA that holds the four
    exponentials, compiled with the library's flags by the compiler at hand."""
    import build  # spectrogram-enhancement_amd/build.py
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "nlmeans.s")
        r = subprocess.run([build.HIPCC, *build.CFLAGS, "--cuda-device-only", "-S",
                            os.path.join(build.CSRC, "nlmeans.hip"), "-o", asm],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        text = open(asm).read()
    ver = subprocess.run([build.HIPCC, "--version"], capture_output=True, text=True).stdout
    ver = " / ".join(line.strip() for line in ver.splitlines()[:2])
    m = re.search(r"^(\w*nlmeans_kernelIfLi%dE\w*):" % P, text, flags=re.M)
    body = text[m.end():text.index(".Lfunc_end", m.end())].splitlines()
    labels = {mm.group(1): n for n, line in enumerate(body)
              if (mm := re.match(r"(\.LBB\d+_\d+):", line))}
    best = []
    for n, line in enumerate(body):
        mm = re.search(r"s_cbranch\w+\s+(\.LBB\d+_\d+)", line)
        if mm and labels.get(mm.group(1), n) < n:
            ins = [x.split()[0] for x in body[labels[mm.group(1)]:n + 1]
                   if x.startswith("\t") and not x.strip().startswith((".", ";"))]
            # the innermost loop that holds the exponentials: a lane's four pixels
            if ins.count("v_exp_f32_e64") + ins.count("v_exp_f32_e32") == 4 and (
                    not best or len(ins) < len(best)):
                best = ins
    if not best:
        raise RuntimeError("shift loop not found in the ISA")
    c = collections.Counter(best)
    valu = sum((2 if k.startswith("v_pk_") else 1) * v for k, v in c.items() if k.startswith("v_"))
    unknown = [k for k in c if k.startswith("ds_") and k not in LDS_READ_CYCLES]
    if unknown:
        raise RuntimeError(f"LDS instructions without a cycle count: {unknown}")
    lds = sum(LDS_READ_CYCLES[k] * v for k, v in c.items() if k.startswith("ds_"))
    return valu, lds, dict(c), ver


VALU_WAVE_INSTR_PER_SHIFT, LDS_CYCLES_PER_SHIFT, LOOP_ISA, COMPILER = shift_loop_counts()
VALU_TP = 256 * 4 / 2.9 * CLOCK / VALU_WAVE_INSTR_PER_SHIFT * PIX_PER_WAVE_SHIFT  # shift-pixels / s
LDS_TP = 256 * CLOCK / LDS_CYCLES_PER_SHIFT * PIX_PER_WAVE_SHIFT
# (label, images, rows, cols, images of the torch route)
SHAPES = [("shot", 20, 256, 3905, 1), ("C5", 4096, 128, 128, 16)]
L = _lib.lib()


def torch_nl_means(u):
    """u [B, rows, cols] float32 -> float32, the composition the kernel replaces."""
    B, rows, cols = u.shape
    f = P // 2
    x = F.pad(u[:, None], (D + f,) * 4, mode="reflect")
    own = x[:, :, D:D + rows + 2 * f, D:D + cols + 2 * f]
    sw = torch.zeros_like(u)
    swv = torch.zeros_like(u)
    for i in range(2 * D + 1):
        for j in range(2 * D + 1):
            sh = x[:, :, i:i + rows + 2 * f, j:j + cols + 2 * f]
            d2 = F.avg_pool2d((own - sh) ** 2, P, stride=1)[:, 0]
            w = torch.exp(-torch.clamp(d2 - 2 * SIGMA * SIGMA, min=0) / (H * H))
            sw += w
            swv += w * sh[:, 0, f:f + rows, f:f + cols]
    return swv / sw


def kernel_call(img, out):
    B, rows, cols = img.shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.specenh_nlmeans(0, ctypes.c_void_p(img.data_ptr()), B, rows, cols, rows * cols,
                                 P, D, H, SIGMA, ctypes.c_void_p(out.data_ptr()), st), "nlmeans")


res = {"patch_size": P, "patch_distance": D, "h": H, "sigma": SIGMA, "shifts": SHIFTS,
       "tile": [_lib.NLMEANS_TILE_ROWS, _lib.NLMEANS_TILE_COLS], "rounds": ROUNDS,
       "warmups": WARM, "valu_wave_instructions_per_shift": VALU_WAVE_INSTR_PER_SHIFT,
       "lds_cycles_per_shift": LDS_CYCLES_PER_SHIFT, "shift_loop_isa": LOOP_ISA,
       "compiler": COMPILER,
       "valu_ceiling_shift_pixels_per_s": VALU_TP, "lds_ceiling_shift_pixels_per_s": LDS_TP,
       "counter_profile": "not taken", "note": "a first version; no counter profile taken",
       "kernel_resources": resources("nlmeans.hip"), "shapes": {}}
print(json.dumps(res["kernel_resources"]), flush=True)
print(f"shift loop: {VALU_WAVE_INSTR_PER_SHIFT} VALU wave instructions, {LDS_CYCLES_PER_SHIFT} "
      f"LDS cycles ({COMPILER})", flush=True)
for label, B, rows, cols, Bt in SHAPES:
    g = torch.Generator("cuda").manual_seed(1)
    S = torch.rand((B, rows, cols), device="cuda", generator=g) * 0.3
    S = (S + torch.exp(-0.5 * ((torch.arange(rows, device="cuda")[:, None] - rows / 2) / 3) ** 2)) / 1.3
    out = torch.empty_like(S)
    runs = {"kernel": lambda: kernel_call(S, out),
            "layer": lambda: filters.nl_means(S, P, D, H, SIGMA),
            "kernel_after_layer": lambda: kernel_call(S, torch.empty_like(S)),
            "torch": lambda: torch_nl_means(S[:Bt])}
    entry = {"images": B, "rows": rows, "cols": cols, "torch_images": Bt}
    entry.update(measure(runs, ROUNDS, WARM))
    sp = B * rows * cols * SHIFTS
    t = entry["kernel_ms_median"] * 1e-3
    entry["shift_pixels"] = sp
    entry["kernel_shift_pixels_per_s"] = sp / t
    entry["kernel_over_valu_ceiling"] = sp / t / VALU_TP
    entry["kernel_over_lds_ceiling"] = sp / t / LDS_TP
    t2 = entry["kernel_after_layer_ms_median"] * 1e-3
    entry["kernel_after_layer_shift_pixels_per_s"] = sp / t2
    entry["kernel_after_layer_over_valu_ceiling"] = sp / t2 / VALU_TP
    entry["kernel_after_layer_over_lds_ceiling"] = sp / t2 / LDS_TP
    entry["nearer_ceiling"] = "VALU issue" if VALU_TP < LDS_TP else "LDS reads"
    entry["layer_over_kernel"] = entry["layer_ms_median"] / entry["kernel_ms_median"]
    entry["layer_over_kernel_after_layer"] = (entry["layer_ms_median"]
                                              / entry["kernel_after_layer_ms_median"])
    entry["torch_ms_per_image"] = entry["torch_ms_median"] / Bt
    entry["kernel_ms_per_image"] = entry["kernel_ms_median"] / B
    entry["torch_over_kernel_per_image"] = entry["torch_ms_per_image"] / entry["kernel_ms_per_image"]
    kernel_call(S, out)
    diff = (out[:Bt] - torch_nl_means(S[:Bt])).abs()
    entry["largest_difference_from_torch"] = float(diff.max())
    entry["pixels_compared"] = int(diff.numel())
    print(f"{label:5s} " + "  ".join(f"{n} {entry[n + '_ms_median']:9.3f} ms" for n in runs)
          + f" ({Bt} images)  {entry['kernel_shift_pixels_per_s']:.3e} shift-pixels/s = "
          f"{entry['kernel_over_valu_ceiling']:.3f} of the VALU ceiling, "
          f"{entry['kernel_over_lds_ceiling']:.3f} of the LDS ceiling; layer / kernel "
          f"{entry['layer_over_kernel']:.2f}; torch / kernel per image "
          f"{entry['torch_over_kernel_per_image']:.1f}; largest difference from torch "
          f"{entry['largest_difference_from_torch']:.2e}", flush=True)
    res["shapes"][label] = entry
    del S, out, diff, runs
    torch.cuda.empty_cache()
write_json(res, path)
