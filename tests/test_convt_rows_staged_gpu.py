"""convT1's staged row sweep (csrc/conv_rows.hip convt_rows_pw_kernel: the step's outputs in an
LDS tile, stored as whole cache lines, one input ring per workgroup) against the kernels it
replaces and against float64.

Bitwise against the per-wave-ring kernel with 8-byte stores (CONVT_STORE8) and the shared-ring
kernel (CONVT_SHARED_RING): the per-phase MFMA order is the same. The 16-byte stores must stay
inside the output: guard images in front of and behind it keep their sentinel. Against a
float64 transposed convolution of the same 16-bit operands the kernel differs by the fp32
summation (1e-5 of the sum of |products|) and one rounding to the 16-bit type.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import specenh  # noqa: F401  (registers torch.ops.specenh.*)
from specenh import _lib

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# (N, H, ROWS_BANDS or None): one step; one image; one-row images; odd sizes; three images on
# some workgroups (zero rows between images, the tile double buffer across an image boundary);
# row bands off and forced to 8 per image (bubble steps)
BITWISE = [(1, 1, None), (1, 16, None), (3, 1, None), (5, 7, None), (1100, 3, None),
           (128, 16, -1), (128, 16, 3)]


def _inputs(N, H, dtype, dev, seed):
    rng = np.random.default_rng(seed)
    x = torch.tensor(np.maximum(rng.standard_normal((N, H, 16, 64)), 0), dtype=dtype, device=dev)
    w = torch.tensor(rng.standard_normal((64, 5, 5, 64)) * 0.05, dtype=dtype, device=dev)
    bias = torch.tensor(rng.standard_normal(64) * 0.3, dtype=torch.float32, device=dev)
    return x, w, bias


def _run(x, w, bias, out):
    N, H, W, C = x.shape
    torch.ops.specenh.conv2d_out(x, w, bias, 5, 5, 64, 1, 3, 3, 2, 2 * H, 2 * W, 1, None, None,
                                 out, False, None)


def _ref(x, w, bias):
    """Conv2DTranspose(64, 5, s2, relu, same) in float64: the stride-1 conv of the
    zero-interleaved input (pad 3 top/left, 2 bottom/right) with the [CO][5][5][64] GEMM
    weights; mag = the sum of |products| + |bias|."""
    N, H, W, C = x.shape
    xd = torch.zeros((N, C, 2 * H - 1, 2 * W - 1), dtype=torch.float64)
    xd[:, :, ::2, ::2] = x.double().cpu().permute(0, 3, 1, 2)
    xd = F.pad(xd, (3, 2, 3, 2))
    wd = w.double().cpu().permute(0, 3, 1, 2)
    b = bias.double().cpu().view(1, -1, 1, 1)
    ref = torch.relu(F.conv2d(xd, wd) + b)
    mag = F.conv2d(xd.abs(), wd.abs()) + b.abs()
    return ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,bands", BITWISE)
def test_staged_bitwise(gpu_device, kernel_variant, dtype, N, H, bands):
    x, w, bias = _inputs(N, H, dtype, gpu_device, 31 + N + H)
    if bands is not None:
        kernel_variant("ROWS_BANDS", bands)
    a = torch.full((N, 2 * H, 32, 64), float("nan"), dtype=dtype, device=gpu_device)
    b = torch.full_like(a, float("nan"))
    c = torch.full_like(a, float("nan"))
    _run(x, w, bias, a)
    assert "convt_rows_pw_kernel" in _lib.last_kernel_name()
    kernel_variant("CONVT_STORE8", 1)
    _run(x, w, bias, b)
    assert "convt_rows_pw_store8_kernel" in _lib.last_kernel_name()
    kernel_variant("CONVT_STORE8", 0)
    kernel_variant("CONVT_SHARED_RING", 1)
    _run(x, w, bias, c)
    assert "convt_rows_kernel" in _lib.last_kernel_name()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
    assert torch.equal(a, c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H", [(1, 1), (3, 1), (1100, 3)])
def test_staged_no_stray_bytes(gpu_device, dtype, N, H):
    """The output is the middle of a tensor with one more image in front and one behind."""
    x, w, bias = _inputs(N, H, dtype, gpu_device, 47 + N + H)
    sentinel = -1234.0
    big = torch.full((N + 2, 2 * H, 32, 64), sentinel, dtype=dtype, device=gpu_device)
    guards = torch.stack([big[0], big[-1]]).clone()
    out = big[1:-1]
    assert out.is_contiguous()
    _run(x, w, bias, out)
    torch.cuda.synchronize()
    assert "convt_rows_pw_kernel" in _lib.last_kernel_name()
    assert torch.equal(torch.stack([big[0], big[-1]]).view(torch.int16), guards.view(torch.int16))
    # (ReLU outputs: the sentinel is negative, so no output element can still hold it)
    assert bool((out >= 0).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H", [(5, 7), (1100, 3)])
def test_staged_vs_float64(gpu_device, dtype, N, H):
    x, w, bias = _inputs(N, H, dtype, gpu_device, 59 + N + H)
    out = torch.full((N, 2 * H, 32, 64), float("nan"), dtype=dtype, device=gpu_device)
    _run(x, w, bias, out)
    torch.cuda.synchronize()
    assert "convt_rows_pw_kernel" in _lib.last_kernel_name()
    ref, mag = _ref(x, w, bias)
    got = out.double().cpu()
    assert bool(torch.isfinite(got).all())
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    assert torch.all((got - ref).abs() <= eps * ref.abs() + 1e-5 * mag + 1e-30)
