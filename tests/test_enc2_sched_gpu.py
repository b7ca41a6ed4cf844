"""enc2_rows_kernel's two step schedules (csrc/conv_rows.hip; variant ENC2_SCHED).

Schedule 1 (the default of the two-workgroups-per-CU build) keeps the pooled store's base and
the DMA's source row as scalar pointers advanced by adds, folds a step's wave-uniform tests
into one flag word computed under the step before, and stages the pooled row in an LDS tile
that leaves as two whole-line stores one step later. Every accumulator keeps its order of
MFMAs and every value its roundings, so for finite values it is BITWISE equal to schedule 0
(ENC2_SCHED=0, the earlier step; a NaN accumulator, which schedule 0's fmaxf drops, is outside
that claim). Heights 4 .. 32 give SPI = H/4 + 1 = 2 .. 9 steps per image: every residue of
the step count modulo the 3 accumulator phases, the 2 tile buffers and the 8-step ring
period, and the one-pair image; N = 1100 gives workgroups of a 512-slot grid 2 or 3 images
each, so image boundaries fall at every phase; H = 128 is the flagship's height, N = 1300 its
image-to-image hand-over."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import specenh  # noqa: F401  (registers torch.ops.specenh.*)
from specenh import _lib

pytestmark = pytest.mark.gpu

SHAPES = [(1, 4), (1, 8), (1, 12), (1, 16), (1, 20), (1, 24), (1, 28), (1, 32), (1100, 8),
          (1100, 12), (3, 128), (1300, 128)]


def _template_args(name):
    """(WPE, SCHED) of the launched enc2_rows_kernel<T, WPE, SCHED>, mangled or demangled."""
    assert "enc2_rows_kernel" in name, name
    m = re.search(r"enc2_rows_kernelI\w+?Li(\d)ELi(\d)EEE", name) or \
        re.search(r"enc2_rows_kernel<[^,>]+, (\d), (\d)>", name)
    assert m, name
    return int(m.group(1)), int(m.group(2))


def _inputs(dev, dtype, N, H, seed=0):
    rng = np.random.default_rng(N + 3 * H + seed)
    x = torch.tensor(rng.uniform(0, 1, (N, H, 128, 1)), dtype=dtype, device=dev)
    w1 = torch.tensor(rng.standard_normal((16, 5, 5, 1)) * 0.3, dtype=dtype, device=dev)
    b1 = torch.tensor(rng.standard_normal(16) * 0.2, dtype=torch.float32, device=dev)
    w2 = torch.tensor(rng.standard_normal((32, 5, 5, 16)) * 0.08, dtype=dtype, device=dev)
    b2 = torch.tensor(rng.standard_normal(32) * 0.2, dtype=torch.float32, device=dev)
    return x, w1, b1, w2, b2


def _run(x, w1, b1, w2, b2, out=None):
    N, H = x.shape[:2]
    if out is None:
        out = torch.full((N, H // 4, 32, 32), float("nan"), dtype=x.dtype, device=x.device)
    torch.ops.specenh.encoder2_out(x, w1, b1, 16, w2, b2, 32, 5, out)
    return out


def _both(kernel_variant, args):
    """The outputs of schedule 1 (the default) and schedule 0 on the same operands."""
    assert _lib.get_variant("ENC2_SCHED") == 1
    new = _run(*args)
    assert _template_args(_lib.last_kernel_name()) == (4, 1)
    kernel_variant("ENC2_SCHED", 0)
    old = _run(*args)
    assert _template_args(_lib.last_kernel_name()) == (4, 0)
    torch.cuda.synchronize()
    return new, old


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N,H", SHAPES)
def test_schedules_bitwise(gpu_device, kernel_variant, dtype, N, H):
    new, old = _both(kernel_variant, _inputs(gpu_device, dtype, N, H))
    assert bool(torch.isfinite(new).all()) and bool(torch.isfinite(old).all())
    assert torch.equal(new.view(torch.int16), old.view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_schedules_bitwise_signed_zeros(gpu_device, kernel_variant, dtype):
    """Sums that are exactly -0, +0 or just below zero (weights and biases of -0, and a second
    layer whose weights are all negative on non-negative inputs): the ReLU of the packed pool
    must give the +0 that fmaxf(., 0) gives."""
    x, w1, b1, w2, b2 = _inputs(gpu_device, dtype, 3, 12, seed=7)
    for case in range(3):
        w2c, b2c, w1c, b1c = w2, b2, w1, b1
        if case == 0:
            w2c, b2c = torch.zeros_like(w2) * -1.0, torch.zeros_like(b2) * -1.0
        elif case == 1:
            w2c, b2c = -w2.abs(), torch.zeros_like(b2)
        else:
            w1c, b1c = torch.zeros_like(w1) * -1.0, torch.zeros_like(b1) * -1.0
        new, old = _both(kernel_variant, (x, w1c, b1c, w2c, b2c))
        kernel_variant("ENC2_SCHED", 1)
        assert torch.equal(new.view(torch.int16), old.view(torch.int16)), case
        if case < 2:
            assert bool((new.view(torch.int16) == 0).all()), case  # all +0, no sign bit


def test_kernel_selection(gpu_device, kernel_variant):
    args = _inputs(gpu_device, torch.float16, 2, 8)
    _run(*args)
    assert _template_args(_lib.last_kernel_name()) == (4, 1)  # the default
    kernel_variant("ENC2_WPE2", 1)
    _run(*args)
    assert _template_args(_lib.last_kernel_name()) == (2, 0)  # one workgroup per CU: the old step
    kernel_variant("ENC2_WPE2", 0)
    kernel_variant("ENC2_SCHED", 0)
    _run(*args)
    assert _template_args(_lib.last_kernel_name()) == (4, 0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N,H", [(1, 4), (3, 12), (1100, 8), (5, 128)])
def test_bounds_with_sentinels(gpu_device, dtype, N, H):
    """One sentinel image (NaN bit pattern) before and one after the output: the staged
    store's tile-to-address map must leave both untouched and fill every real element."""
    args = _inputs(gpu_device, dtype, N, H)
    buf = torch.full((N + 2, H // 4, 32, 32), float("nan"), dtype=dtype, device=gpu_device)
    sentinel = buf[0].view(torch.int16).clone()
    _run(*args, out=buf[1:-1])
    torch.cuda.synchronize()
    assert _template_args(_lib.last_kernel_name()) == (4, 1)
    assert torch.equal(buf[0].view(torch.int16), sentinel)
    assert torch.equal(buf[-1].view(torch.int16), sentinel)
    assert bool(torch.isfinite(buf[1:-1]).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_default_schedule_vs_float64(gpu_device, dtype):
    """The bound of test_encoder2_equals_two_launches at (5, 20): the second layer in float64
    on the stored intermediate (conv1_rows_pool_kernel's output, which the fused launch
    reproduces bit for bit in LDS), eps |ref| + 1e-5 mag."""
    N, H = 5, 20
    x, w1, b1, w2, b2 = _inputs(gpu_device, dtype, N, H)
    out = _run(x, w1, b1, w2, b2)
    torch.cuda.synchronize()
    assert _template_args(_lib.last_kernel_name()) == (4, 1)
    h1 = torch.empty((N, H // 2, 64, 16), dtype=dtype, device=gpu_device)
    torch.ops.specenh.conv2d_out(x, w1, b1, 5, 5, 16, 1, 2, 2, 1, H, 128, 1, None, None, h1, True,
                                 None)
    torch.cuda.synchronize()
    xd = h1.double().cpu().permute(0, 3, 1, 2)
    wd = w2.double().cpu().permute(0, 3, 1, 2)
    b = b2.double().cpu().view(1, -1, 1, 1)
    ref = F.max_pool2d(torch.relu(F.conv2d(xd, wd, padding=2) + b), 2).permute(0, 2, 3, 1)
    mag = F.max_pool2d(F.conv2d(xd.abs(), wd.abs(), padding=2) + b.abs(), 2).permute(0, 2, 3, 1)
    got = out.double().cpu()
    assert bool(torch.isfinite(got).all())
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    assert torch.all((got - ref).abs() <= eps * ref.abs() + 1e-5 * mag + 1e-30)
