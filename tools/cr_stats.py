"""Per-wave clocks of the segments of a row sweep's step (development build):
    tools/build_variant.sh crstats conv_rows.hip -DSPECENH_CR_STATS
    SPECENH_LIB=$PWD/tools/variants/libspecenh_crstats.so python tools/cr_stats.py [N] [H]
    SPECENH_LIB=$PWD/tools/variants/libspecenh_crstats.so python tools/cr_stats.py enc2 [N] [H]
Without `enc2`: conv_rows_pool_kernel at the C5 conv3 + pool launch shape. For each schedule
(CONV_ROWS_SCHED = 0, 1) the mean shader clocks per step and wave of: the pool and store head,
the DMA issue, the fragment reads until the first MFMA can issue, the MFMA block, the vmcnt wait
and the barrier wait. Schedule 1 has no separate head or read segment (both run under its MFMA
block).
With `enc2`: enc2_rows_kernel at the C5 fused-encoder launch shape (N images of H x 128), for
each schedule (ENC2_SCHED = 0, 1): the pool + store head (schedule 1: the two storing waves'
whole-line store), the DMA issue (image rows are staged once: no copy shift since the packed
conv1), conv1 (schedule 1: with the pool under it), the conv2 block, the vmcnt wait and the
barrier wait; waves 0-3 (DMA, the ledger) and waves 4-7 also as two means.
A stamp is an s_memtime and two lgkmcnt waits: read the shares, not the totals. Waves 0-3 move
the rows (LDS-DMA); wave w shares a SIMD with w + 4."""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "spectrogram-enhancement_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import specenh  # noqa: E402,F401
from specenh import _lib  # noqa: E402

args = sys.argv[1:]
ENC2 = bool(args) and args[0] == "enc2"
if ENC2:
    args = args[1:]
SEGS = ["head", "dma", "conv1", "conv2", "vmcnt", "barrier"] if ENC2 else \
    ["head", "dma", "reads", "mfma", "vmcnt", "barrier"]
SWITCH = "ENC2_SCHED" if ENC2 else "CONV_ROWS_SCHED"
N = int(args[0]) if len(args) > 0 else 2048
H = int(args[1]) if len(args) > 1 else (128 if ENC2 else 32)
dev = torch.device("cuda", 0)
L = _lib.lib()
if not hasattr(L, "specenh_cr_stats"):
    sys.exit("this library has no step clocks: build it with -DSPECENH_CR_STATS (see above)")

if ENC2:
    x = torch.rand(N, H, 128, 1, device=dev).half()
    w1 = (torch.randn(16, 5, 5, 1, device=dev) * 0.3).half()
    b1 = torch.randn(16, device=dev) * 0.2
    w2 = (torch.randn(32, 5, 5, 16, device=dev) * 0.08).half()
    b2 = torch.randn(32, device=dev) * 0.2
    out = torch.empty(N, H // 4, 32, 32, dtype=torch.float16, device=dev)

    def launch():
        torch.ops.specenh.encoder2_out(x, w1, b1, 16, w2, b2, 32, 5, out)
else:
    C, CO, W, K = 32, 64, 32, 5
    x = (torch.rand(N, H, W, C, device=dev) * 0.5).half()
    w = (torch.randn(CO, K, K, C, device=dev) * 0.05).half()
    b = torch.randn(CO, device=dev) * 0.1
    out = torch.empty(N, H // 2, W // 2, CO, dtype=torch.float16, device=dev)

    def launch():
        torch.ops.specenh.conv2d_out(x, w, b, K, K, CO, 1, K // 2, K // 2, 1, H, W, 1, None, None,
                                     out, True, None)


def row(label, m):
    print(f"  {label:>5} " + "".join(f"{v:10.0f}" for v in m) + f"{m.sum():10.0f}")


for sched in (0, 1):
    _lib.set_variant(SWITCH, sched)
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(10):
        launch()
    ev[1].record()
    ev[1].synchronize()
    name = _lib.last_kernel_name()
    buf = (ctypes.c_ulonglong * (1024 * 8 * 8))()
    assert L.specenh_cr_stats(buf, ctypes.sizeof(buf)) == 0
    st = np.frombuffer(buf, dtype=np.uint64).reshape(1024, 8, 8).astype(np.float64)
    G = int((st[:, 0, 6] > 0).sum())  # workgroups of the last launch
    st = st[:G]
    steps = st[:, :, 6]
    per = st[:, :, :6] / np.maximum(steps, 1)[:, :, None]
    print(f"{SWITCH}={sched}  N={N} H={H}  {ev[0].elapsed_time(ev[1]) / 10:.4f} ms per launch "
          f"(stamped build), {G} workgroups, {steps.mean():.0f} steps each")
    print(f"  {name}")
    print("   wave " + "".join(s.rjust(10) for s in SEGS) + "     total")
    for wv in range(8):
        row(str(wv), per[:, wv].mean(axis=0))
    if ENC2:
        row("0-3", per[:, :4].mean(axis=(0, 1)))
        row("4-7", per[:, 4:].mean(axis=(0, 1)))
    m = per.mean(axis=(0, 1))
    row("all", m)
    print("  share " + "".join(f"{v / m.sum():10.2f}" for v in m))
