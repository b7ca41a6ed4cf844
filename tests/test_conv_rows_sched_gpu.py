"""conv_rows_pool_kernel's two step schedules (csrc/conv_rows.hip; variant CONV_ROWS_SCHED).

Schedule 1 (the default for the 32 -> 64 conv3 on 32-wide maps) reads a step's B fragments one
step ahead into a second register buffer, issues the MFMAs of the accumulators that were not
just pooled first, with the pool and its store in their shadow, and lets only the DMA waves
wait on vmcnt. Every accumulator keeps its (row, tap column, tap row) order of MFMAs, so it is
BITWISE equal to schedule 0 (CONV_ROWS_SCHED=0, the earlier step). Heights 2 .. 12 give
S = H/2 + 2 = 3 .. 8 steps: every residue of the step count modulo the unroll's 3 accumulator
phases and 2 fragment buffers, and the one-pair image; N = 1100 gives the persistent
workgroups unequal image counts and image boundaries at every phase; H = 32 is the flagship's.
The other three shapes keep schedule 0 in both modes and are checked the same way."""
import re

import pytest
import torch
import torch.nn.functional as F

import specenh  # noqa: F401  (registers torch.ops.specenh.*)
from specenh import _lib

pytestmark = pytest.mark.gpu

# (C, CO, W, K) of tests/test_conv_rows_gpu.py
SHAPES = [(16, 32, 64, 5), (32, 64, 32, 5), (32, 32, 64, 5), (32, 32, 64, 3)]
FLAGSHIP = (32, 64, 32, 5)


def _sched(name):
    """The SCHED template argument (the last one) of the launched conv_rows_pool_kernel."""
    assert "conv_rows_pool_kernel" in name, name
    m = re.search(r"Li(\d)EEEv", name) or re.search(r", (\d)>\(", name)
    assert m, name
    return int(m.group(1))


def _inputs(dev, dtype, C, CO, W, K, N, H):
    g = torch.Generator(device=dev)
    g.manual_seed(1000 * N + 10 * H + C + CO + K)
    x = torch.randn((N, H, W, C), generator=g, device=dev).to(dtype)
    w = (torch.randn((CO, K, K, C), generator=g, device=dev) * 0.1).to(dtype)
    bias = torch.randn((CO,), generator=g, device=dev) * 0.5
    return x, w, bias


def _run(x, w, bias, CO, K):
    N, H, W, C = x.shape
    out = torch.full((N, H // 2, W // 2, CO), float("nan"), dtype=x.dtype, device=x.device)
    torch.ops.specenh.conv2d_out(x, w, bias, K, K, CO, 1, K // 2, K // 2, 1, H, W, 1, None, None,
                                 out, True, None)
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C,CO,W,K", SHAPES)
@pytest.mark.parametrize("N,H", [(1, 2), (1, 4), (1, 6), (1, 8), (1, 10), (1, 12), (1100, 4),
                                 (1100, 6), (3, 32)])
def test_schedules_bitwise(gpu_device, kernel_variant, dtype, C, CO, W, K, N, H):
    x, w, bias = _inputs(gpu_device, dtype, C, CO, W, K, N, H)
    assert _lib.get_variant("CONV_ROWS_SCHED") == 1  # the default
    new = _run(x, w, bias, CO, K)
    assert _sched(_lib.last_kernel_name()) == (1 if (C, CO, W, K) == FLAGSHIP else 0)
    kernel_variant("CONV_ROWS_SCHED", 0)
    old = _run(x, w, bias, CO, K)
    assert _sched(_lib.last_kernel_name()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(new).all()) and bool(torch.isfinite(old).all())
    assert torch.equal(new.view(torch.int16), old.view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("C,CO,W,K", SHAPES)
def test_default_schedule_vs_float64(gpu_device, dtype, C, CO, W, K):
    """The bound of test_conv_rows_gpu.py's test_rows_vs_float64: products of 16-bit values are
    exact in fp32, so the kernel differs from a float64 conv + bias + ReLU + max-pool of the
    same operands by the fp32 summation (1e-5 of the pooled window's sum of |products|) and one
    rounding to the 16-bit type (2^-11 fp16, 2^-8 bf16)."""
    N, H = 5, 18
    x, w, bias = _inputs(gpu_device, dtype, C, CO, W, K, N, H)
    out = _run(x, w, bias, CO, K)
    torch.cuda.synchronize()
    assert _sched(_lib.last_kernel_name()) == (1 if (C, CO, W, K) == FLAGSHIP else 0)
    xd = x.double().cpu().permute(0, 3, 1, 2)
    wd = w.double().cpu().permute(0, 3, 1, 2)
    b = bias.double().cpu().view(1, -1, 1, 1)
    ref = F.max_pool2d(torch.relu(F.conv2d(xd, wd, padding=K // 2) + b), 2).permute(0, 2, 3, 1)
    mag = F.max_pool2d(F.conv2d(xd.abs(), wd.abs(), padding=K // 2) + b.abs(), 2).permute(0, 2, 3, 1)
    got = out.double().cpu()
    assert bool(torch.isfinite(got).all())
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    assert torch.all((got - ref).abs() <= eps * ref.abs() + 1e-5 * mag + 1e-30)
