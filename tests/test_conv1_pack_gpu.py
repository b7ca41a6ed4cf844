"""The packed conv1 row sweep on the GPU (csrc/conv_rows.hip: conv1_rows_pool_kernel and the
conv1 part of enc2_rows_kernel; VAE/manual_scan_3layers.py:187-191): all 25 taps of the first
Conv2D(16, 5, relu, same) in one K = 32 MFMA per (output row, column parity), the B fragment
gathered as four 32-bit words from singly staged rows (tests/test_conv1_pack_mapping.py
restates the map on the CPU).

Exact tap test: one-hot weights (channel c has a single 1 at tap (ky, kx); 25 taps over 16
channels are two weight sets), bias 0, images of distinct small integers exact in fp16 and bf16.
Every product is then exact and 24 of the 25 are zeros, so the output must equal the shifted
image, pooled, bit for bit: a tap in a wrong K slot, a word gathered from a wrong row or column
or a zero-weight slot that is not excluded shows as an unequal element. The spiked image carries
2040 at scattered pixels, so most windows hold a large value at the window column of the other
parity (0 or 5) or in the row below the kernel, where the weight is zero. Through the fused
encoder the second convolution is an identity (centre-tap one-hot on channels 0-15), so its
output is the conv1 result pooled once more.

Float64 bound: as tests/test_conv_rows_gpu.py (products of 16-bit values are exact in fp32; the
kernel differs from float64 by the fp32 summation, bounded by 1e-5 of the sum of |products| of
the pooled window, and one rounding to the 16-bit type, eps = 2^-11 / 2^-8).

Shapes: H = 2 is the one-pair image, (3, 4) and (2, 10) reach every slot of the 16-row ring,
both halos and the hand-over from image to image; N = 4200 and 1100 give every persistent
workgroup several images with bubbles at every phase. Outputs start NaN-filled."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import specenh  # noqa: F401  (registers torch.ops.specenh.*)
from specenh import _lib

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]


def _conv(x, w, bias, CO, pool_out):
    N, H, W, C = x.shape
    torch.ops.specenh.conv2d_out(x, w, bias, 5, 5, CO, 1, 2, 2, 1, H, W, 1, None, None,
                                 pool_out, True, None)


def _ref(x, w, bias):
    xd = x.double().cpu().permute(0, 3, 1, 2)
    wd = w.double().cpu().permute(0, 3, 1, 2)
    b = bias.double().cpu().view(1, -1, 1, 1)
    ref = F.max_pool2d(torch.relu(F.conv2d(xd, wd, padding=2) + b), 2)
    mag = F.max_pool2d(F.conv2d(xd.abs(), wd.abs(), padding=2) + b.abs(), 2)
    return ref.permute(0, 2, 3, 1), mag.permute(0, 2, 3, 1)


def _within(got, ref, mag, dtype):
    eps = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    return bool(torch.all((got - ref).abs() <= eps * ref.abs() + 1e-5 * mag + 1e-30))


# ---------------------------------------------------------------- exact taps
def _image(N, H, spiked):
    """Distinct small integers (1 .. 251: exact in bf16), optionally 2040 at scattered pixels."""
    n, y, x = np.meshgrid(np.arange(N), np.arange(H), np.arange(128), indexing="ij")
    img = (7 * x + 13 * y + 29 * n) % 251 + 1
    if spiked:
        img = np.where((x + 5 * y + 3 * n) % 11 == 0, 2040, img)
    return img.astype(np.float64)


def _onehot_w1(wset):
    """[16][5][5][1]: channel c's single 1 at tap 16 wset + c (row-major (ky, kx)); the channels
    past the 25th tap repeat taps from the start."""
    w = np.zeros((16, 5, 5, 1))
    for c in range(16):
        t = (16 * wset + c) % 25
        w[c, t // 5, t % 5, 0] = 1.0
    return w


def _taps_pooled(img, wset):
    """[N][H/2][64][16]: the image shifted by each channel's tap, ReLU, 2 x 2 max."""
    N, H, _ = img.shape
    pad = np.zeros((N, H + 4, 132))
    pad[:, 2:-2, 2:-2] = img
    out = np.empty((N, H // 2, 64, 16))
    for c in range(16):
        t = (16 * wset + c) % 25
        sh = np.maximum(pad[:, t // 5:t // 5 + H, t % 5:t % 5 + 128], 0.0)
        out[..., c] = sh.reshape(N, H // 2, 2, 64, 2).max(axis=(2, 4))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spiked", [False, True])
@pytest.mark.parametrize("wset", [0, 1])
@pytest.mark.parametrize("N,H", [(1, 2), (3, 4), (2, 10)])
def test_conv1_rows_exact_taps(gpu_device, dtype, spiked, wset, N, H):
    img = _image(N, H, spiked)
    x = torch.tensor(img[..., None], dtype=dtype, device=gpu_device)
    assert np.array_equal(x.double().cpu().numpy()[..., 0], img)
    w = torch.tensor(_onehot_w1(wset), dtype=dtype, device=gpu_device)
    bias = torch.zeros(16, dtype=torch.float32, device=gpu_device)
    out = torch.full((N, H // 2, 64, 16), float("nan"), dtype=dtype, device=gpu_device)
    _conv(x, w, bias, 16, out)
    torch.cuda.synchronize()
    assert "conv1_rows_pool_kernel" in _lib.last_kernel_name()
    want = torch.tensor(_taps_pooled(img, wset), dtype=dtype)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("spiked", [False, True])
@pytest.mark.parametrize("wset", [0, 1])
@pytest.mark.parametrize("N,H", [(1, 4), (3, 12)])
def test_encoder2_exact_taps(gpu_device, dtype, spiked, wset, N, H):
    img = _image(N, H, spiked)
    x = torch.tensor(img[..., None], dtype=dtype, device=gpu_device)
    w1 = torch.tensor(_onehot_w1(wset), dtype=dtype, device=gpu_device)
    b1 = torch.zeros(16, dtype=torch.float32, device=gpu_device)
    w2n = np.zeros((32, 5, 5, 16))
    for c in range(16):
        w2n[c, 2, 2, c] = 1.0
    w2 = torch.tensor(w2n, dtype=dtype, device=gpu_device)
    b2 = torch.zeros(32, dtype=torch.float32, device=gpu_device)
    out = torch.full((N, H // 4, 32, 32), float("nan"), dtype=dtype, device=gpu_device)
    torch.ops.specenh.encoder2_out(x, w1, b1, 16, w2, b2, 32, 5, out)
    torch.cuda.synchronize()
    assert "enc2_rows_kernel" in _lib.last_kernel_name()
    h1 = _taps_pooled(img, wset)
    want = np.zeros((N, H // 4, 32, 32))
    want[..., :16] = h1.reshape(N, H // 4, 2, 32, 2, 16).max(axis=(2, 4))
    assert torch.equal(out.cpu(), torch.tensor(want, dtype=dtype))


# ---------------------------------------------------------------- float64 bound
def _random_layer1(rng, N, H, dtype, dev):
    x = torch.tensor(rng.uniform(0, 1, (N, H, 128, 1)), dtype=dtype, device=dev)
    w1 = torch.tensor(rng.standard_normal((16, 5, 5, 1)) * 0.3, dtype=dtype, device=dev)
    b1 = torch.tensor(rng.standard_normal(16) * 0.2, dtype=torch.float32, device=dev)
    return x, w1, b1


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv1_rows_vs_float64_many_images(gpu_device, dtype):
    N, H = 4200, 4
    x, w1, b1 = _random_layer1(np.random.default_rng(N + H), N, H, dtype, gpu_device)
    out = torch.full((N, H // 2, 64, 16), float("nan"), dtype=dtype, device=gpu_device)
    _conv(x, w1, b1, 16, out)
    torch.cuda.synchronize()
    assert "conv1_rows_pool_kernel" in _lib.last_kernel_name()
    ref, mag = _ref(x, w1, b1)
    got = out.double().cpu()
    assert bool(torch.isfinite(got).all())
    assert _within(got, ref, mag, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H", [(1100, 8), (5, 20)])
def test_encoder2_vs_float64(gpu_device, dtype, N, H):
    """Both layers against float64: the first on the image, the second on the first layer's
    map as stored (rounded to the 16-bit type), which the fused launch must reproduce."""
    rng = np.random.default_rng(N + 3 * H)
    x, w1, b1 = _random_layer1(rng, N, H, dtype, gpu_device)
    w2 = torch.tensor(rng.standard_normal((32, 5, 5, 16)) * 0.08, dtype=dtype, device=gpu_device)
    b2 = torch.tensor(rng.standard_normal(32) * 0.2, dtype=torch.float32, device=gpu_device)
    out = torch.full((N, H // 4, 32, 32), float("nan"), dtype=dtype, device=gpu_device)
    torch.ops.specenh.encoder2_out(x, w1, b1, 16, w2, b2, 32, 5, out)
    torch.cuda.synchronize()
    assert "enc2_rows_kernel" in _lib.last_kernel_name()
    h1 = torch.full((N, H // 2, 64, 16), float("nan"), dtype=dtype, device=gpu_device)
    _conv(x, w1, b1, 16, h1)
    torch.cuda.synchronize()
    ref1, mag1 = _ref(x, w1, b1)
    assert _within(h1.double().cpu(), ref1, mag1, dtype)
    ref2, mag2 = _ref(h1, w2, b2)
    got = out.double().cpu()
    assert bool(torch.isfinite(got).all())
    assert _within(got, ref2, mag2, dtype)


# ---------------------------------------------------------------- sentinels
@pytest.mark.parametrize("dtype", DTYPES)
def test_sentinel_images_untouched(gpu_device, dtype):
    """One guard image before and one after each output at (3, 12): neither launch writes
    outside its N images."""
    N, H = 3, 12
    rng = np.random.default_rng(12)
    x, w1, b1 = _random_layer1(rng, N, H, dtype, gpu_device)
    w2 = torch.tensor(rng.standard_normal((32, 5, 5, 16)) * 0.08, dtype=dtype, device=gpu_device)
    b2 = torch.tensor(rng.standard_normal(32) * 0.2, dtype=torch.float32, device=gpu_device)
    guard = -7.0
    buf1 = torch.full((N + 2, H // 2, 64, 16), guard, dtype=dtype, device=gpu_device)
    buf2 = torch.full((N + 2, H // 4, 32, 32), guard, dtype=dtype, device=gpu_device)
    buf1[1:-1] = float("nan")
    buf2[1:-1] = float("nan")
    _conv(x, w1, b1, 16, buf1[1:-1])
    torch.cuda.synchronize()
    assert "conv1_rows_pool_kernel" in _lib.last_kernel_name()
    torch.ops.specenh.encoder2_out(x, w1, b1, 16, w2, b2, 32, 5, buf2[1:-1])
    torch.cuda.synchronize()
    assert "enc2_rows_kernel" in _lib.last_kernel_name()
    for buf in (buf1, buf2):
        assert bool((buf[0] == guard).all()) and bool((buf[-1] == guard).all())
        assert bool(torch.isfinite(buf[1:-1]).all())
    ref1, mag1 = _ref(x, w1, b1)
    assert _within(buf1[1:-1].double().cpu(), ref1, mag1, dtype)
