"""Per-wave clocks of the segments of conv_rows_pool_kernel's step at the C5 conv3 + pool launch
shape (development build):
    tools/build_variant.sh crstats conv_rows.hip -DSPECENH_CR_STATS
    SPECENH_LIB=$PWD/tools/variants/libspecenh_crstats.so python tools/cr_stats.py [N] [H]
For each schedule (CONV_ROWS_SCHED = 0, 1) the mean shader clocks per step and wave of: the pool
and store head, the DMA issue, the fragment reads until the first MFMA can issue, the MFMA
block, the vmcnt wait and the barrier wait. Schedule 1 has no separate head or read segment
(both run under its MFMA block). A stamp is an s_memtime and two lgkmcnt waits: read the
shares, not the totals. Waves 0-3 move the rows (LDS-DMA); wave w shares a SIMD with w + 4."""
import ctypes
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "spectrogram-enhancement_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import specenh  # noqa: E402,F401
from specenh import _lib  # noqa: E402

SEGS = ["head", "dma", "reads", "mfma", "vmcnt", "barrier"]
N = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
H = int(sys.argv[2]) if len(sys.argv) > 2 else 32
C, CO, W, K = 32, 64, 32, 5
dev = torch.device("cuda", 0)
x = (torch.rand(N, H, W, C, device=dev) * 0.5).half()
w = (torch.randn(CO, K, K, C, device=dev) * 0.05).half()
b = torch.randn(CO, device=dev) * 0.1
out = torch.empty(N, H // 2, W // 2, CO, dtype=torch.float16, device=dev)
L = _lib.lib()
if not hasattr(L, "specenh_cr_stats"):
    sys.exit("this library has no step clocks: build it with -DSPECENH_CR_STATS (see above)")


def launch():
    torch.ops.specenh.conv2d_out(x, w, b, K, K, CO, 1, K // 2, K // 2, 1, H, W, 1, None, None,
                                 out, True, None)


for sched in (0, 1):
    _lib.set_variant("CONV_ROWS_SCHED", sched)
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
    print(f"CONV_ROWS_SCHED={sched}  N={N} H={H}  {ev[0].elapsed_time(ev[1]) / 10:.4f} ms per launch "
          f"(stamped build), {G} workgroups, {steps.mean():.0f} steps each")
    print(f"  {name}")
    print("  wave " + "".join(s.rjust(9) for s in SEGS) + "    total")
    for wv in range(8):
        m = per[:, wv].mean(axis=0)
        print(f"  {wv:4d} " + "".join(f"{v:9.0f}" for v in m) + f"{m.sum():9.0f}")
    m = per.mean(axis=(0, 1))
    print("   all " + "".join(f"{v:9.0f}" for v in m) + f"{m.sum():9.0f}")
    print("  share" + "".join(f"{v / m.sum():9.2f}" for v in m))
