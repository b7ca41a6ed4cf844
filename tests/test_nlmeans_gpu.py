"""GPU parity of non-local means (csrc/nlmeans.hip) against the numpy restatement of
tests/nlmeans_local.py.

The criterion is the one of include/specenh_nlmeans.h: with q the float64 quotient on the
float32 image and B the per-pixel bound built from the float64 weights (c_d = P^2 + 8, c_e = 4,
constants that depend on the patch size alone), |out - q| <= B at EVERY pixel. Shapes are the
smallest at which tiling and reflection can go wrong: images smaller than the halo (reflection
repeats), one below / at / one above the kernel's tile in either direction, more than two tiles
both ways. Every parameter set runs at every shape: the float64 restatement of (9, 15) at the
largest shape takes about a second for the three images. Each test prints the worst
|out - q| / B and the worst absolute error."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bilateral_local as bl
import nlmeans_local as nl

pytestmark = pytest.mark.gpu

from specenh import _lib  # noqa: E402

TR, TC = _lib.NLMEANS_TILE_ROWS, _lib.NLMEANS_TILE_COLS
# (P, D, h, sigma): skimage's defaults; sigma active; single-pixel patch; weights underflow;
# both limits; identity
PARAMS = [(7, 11, 0.1, 0.0), (5, 6, 0.08, 0.05), (1, 1, 0.5, 0.0), (3, 2, 0.02, 0.0),
          (9, 15, 0.3, 0.2), (7, 0, 0.1, 0.0)]
SHAPES = [(1, 1), (1, 9), (9, 1), (5, 3), (16, 16), (TR - 1, TC + 1), (TR, TC), (TR + 1, TC - 1),
          (2 * TR + 3, 2 * TC + 5), (64, 48)]
PAD = 13  # elements between the images of a strided batch
SENTINEL = -7.25


@functools.lru_cache(maxsize=None)
def images(shape):
    """Three float32 images of a shape: noise, smooth, a ridge on noise; read-only."""
    rows, cols = shape
    seed = 1000 * rows + cols
    b = np.stack([nl.noise_image(rows, cols, seed), nl.smooth_image(rows, cols, seed + 1),
                  nl.ridge_image(rows, cols, seed + 2)])
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def truth(shape, params):
    """(q, B) float64 [3, rows, cols] of images(shape); read-only."""
    q, B = nl.quotient64_and_bound(images(shape), *params)
    q.setflags(write=False)
    B.setflags(write=False)
    return q, B


def strided(batch, pad, dev, fill=0.5):
    """(buffer [B, rows*cols + pad], view [B, rows, cols]) of `batch` on the device, the
    images `pad` elements apart and the padding filled with `fill`."""
    t = torch.as_tensor(np.array(batch))
    B, rows, cols = t.shape
    buf = torch.full((B, rows * cols + pad), fill, dtype=t.dtype, device=dev)
    buf[:, :rows * cols] = t.to(dev).reshape(B, -1)
    return buf, buf[:, :rows * cols].view(B, rows, cols)


def run_c(view, params):
    """specenh_nlmeans on a batch-strided view; out gets the same stride, its padding pre-filled
    with SENTINEL. Returns (out buffer, out view)."""
    B, rows, cols = view.shape
    stride = view.stride(0) if B > 1 else rows * cols
    obuf = torch.full((B, stride), SENTINEL, dtype=view.dtype, device=view.device)
    code = {torch.float32: 0, torch.float64: 3}[view.dtype]
    st = ctypes.c_void_p(torch.cuda.current_stream(view.device).cuda_stream)
    _lib.check(_lib.lib().specenh_nlmeans(code, ctypes.c_void_p(view.data_ptr()), B, rows, cols,
                                          stride, int(params[0]), int(params[1]),
                                          float(params[2]), float(params[3]),
                                          ctypes.c_void_p(obuf.data_ptr()), st), "nlmeans")
    return obuf, obuf[:, :rows * cols].view(B, rows, cols)


def run_op(t, params):
    return torch.ops.specenh.nl_means(t, int(params[0]), int(params[1]), float(params[2]),
                                      float(params[3]))


def assert_every_pixel(out, q, B, what):
    err = np.abs(out.astype(np.float64) - q)
    with np.errstate(invalid="ignore", divide="ignore"):   # B is 0 where D = 0 meets a zero pixel
        ratio = np.where(err == 0, 0.0, err / B)
    print(f"\n[nlmeans {what}] worst |out - q| / B = {float(ratio.max()):.4f}, "
          f"worst |out - q| = {float(err.max()):.3e} (B there {float(B.flat[err.argmax()]):.3e})")
    bad = np.argwhere(~(err <= B))
    assert bad.size == 0, (what, bad[:5].tolist(), float(ratio.max()))


def pid(p):
    return f"P{p[0]}-D{p[1]}-h{p[2]:g}-s{p[3]:g}"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("params", PARAMS, ids=pid)
def test_parity_every_pixel(gpu_device, params, shape):
    """Batch 3 (noise, smooth, ridge) with a padded stride, float32. Measured on an MI355X:
    the worst |out - q| / B over the 60 cases is 0.17."""
    u = images(shape)
    _, view = strided(u, PAD, gpu_device)
    _, out = run_c(view, params)
    assert out.shape == u.shape and out.dtype == torch.float32
    q, B = truth(shape, params)
    assert_every_pixel(out.cpu().numpy(), q, B, f"{params} {shape}")


@pytest.mark.parametrize("params", [PARAMS[0], PARAMS[1], PARAMS[4]], ids=pid)
def test_float64_entry_is_the_float32_call_on_the_cast_image(gpu_device, params):
    rng = np.random.default_rng(3)
    for shape in ((TR + 1, TC + 3), (5, 3)):
        S = rng.random((2,) + shape)                    # float64 values float32 cannot hold
        t64 = torch.from_numpy(S).to(gpu_device)
        got = run_op(t64, params)
        want = run_op(t64.float(), params)
        assert got.dtype == torch.float64 and want.dtype == torch.float32
        assert torch.equal(got, want.double())
        _, view = strided(S, PAD, gpu_device)
        assert torch.equal(run_c(view, params)[1], got)


@pytest.mark.parametrize("params", [PARAMS[0], PARAMS[3], PARAMS[4]], ids=pid)
def test_deterministic_across_batch_position_stride_and_runs(gpu_device, params):
    """The same image at batch positions 0, 1, 2 and at three strides gives identical bits,
    alone or beside other images; two runs give identical bits."""
    for shape in ((2 * TR + 3, 2 * TC + 5), (5, 3), (TR + 1, TC - 1)):
        u = images(shape)
        same = np.stack([u[2], u[2], u[2]])
        a = run_c(strided(same, PAD, gpu_device)[1], params)[1]
        b = run_c(strided(same, 0, gpu_device)[1], params)[1]
        c = run_c(strided(same, 4096 + 1, gpu_device)[1], params)[1]
        assert torch.equal(a[0], a[1]) and torch.equal(a[0], a[2])
        assert torch.equal(a, b) and torch.equal(a, c)
        mixed = strided(u, PAD, gpu_device)[1]
        m1, m2 = run_c(mixed, params)[1], run_c(mixed, params)[1]
        assert torch.equal(m1, m2)
        assert torch.equal(m1[2], a[0])           # alone or beside other images
        single = run_op(torch.from_numpy(np.array(u[2:3])).to(gpu_device), params)
        assert torch.equal(single[0], a[0])


def test_distance_zero_returns_the_input_bit_for_bit(gpu_device):
    for shape in ((TR + 1, TC + 1), (1, 1), (5, 3)):
        u = np.array(images(shape))
        u[0].flat[0] = -0.0                            # the sign of zero is a bit too
        _, view = strided(u, PAD, gpu_device)
        for P, h, sigma in ((7, 0.1, 0.0), (1, 0.5, 0.3), (9, 0.02, 0.0)):
            out = run_c(view, (P, 0, h, sigma))[1]
            assert torch.equal(out.view(torch.int32), view.view(torch.int32).contiguous())
            assert np.array_equal(run_op(view, (P, 0, h, sigma)).cpu().numpy().view(np.int32),
                                  u.view(np.int32))


def test_memory_outside_the_output_is_untouched(gpu_device):
    """The input, the padding between its images and the padding of out stay as they were."""
    for shape, params in (((TR + 1, TC + 1), PARAMS[0]), ((5, 3), PARAMS[4]),
                          ((2 * TR + 3, 2 * TC + 5), PARAMS[1])):
        u = images(shape)
        buf, view = strided(u, PAD, gpu_device, fill=123.0)
        before = buf.clone()
        obuf, out = run_c(view, params)
        n = shape[0] * shape[1]
        assert torch.equal(buf, before)
        assert (buf[:, n:] == 123.0).all()
        assert (obuf[:, n:] == SENTINEL).all()
        q, B = truth(shape, params)
        assert_every_pixel(out.cpu().numpy(), q, B, f"padding {params} {shape}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_python_entries_give_identical_bits(gpu_device, dtype):
    """filters.nl_means on a batch equals the per-image calls, the operator,
    restoration.denoise_nl_means and numpy input, with gaussblr's dtype rule for numpy."""
    from specenh import filters, restoration

    for shape, params in (((40, 70), (7, 11, 0.1, 0.0)), ((TR + 1, TC + 3), (5, 6, 0.08, 0.05)),
                          ((9, 1), (3, 2, 0.02, 0.0))):
        S = np.array(images(shape)).astype(dtype)
        t = torch.from_numpy(S).to(gpu_device)
        want = run_c(strided(S, PAD, gpu_device)[1], params)[1].cpu().numpy()
        got = filters.nl_means(t, *params)
        assert got.dtype == t.dtype and got.shape == t.shape and got.device == t.device
        assert got.is_contiguous() and np.array_equal(got.cpu().numpy(), want)
        assert np.array_equal(run_op(t, params).cpu().numpy(), want)
        kw = dict(patch_size=params[0], patch_distance=params[1], h=params[2], sigma=params[3])
        assert np.array_equal(restoration.denoise_nl_means(t, **kw).cpu().numpy(), want)
        for b in range(3):                       # a batch equals the per-image calls
            one = filters.nl_means(t[b], *params)
            assert one.shape == shape and np.array_equal(one.cpu().numpy(), want[b])
            assert np.array_equal(run_op(t[b], params).cpu().numpy(), want[b])
        for f in (filters.nl_means, restoration.denoise_nl_means):
            host = f(S[0], **kw)
            # float32 numpy is computed and returned in float32, all else in float64
            assert isinstance(host, np.ndarray) and host.dtype == dtype and host.shape == shape
            assert np.array_equal(host, want[0])
    ints = (np.array(images((12, 20)))[0] * 255).astype(np.int32)
    host = filters.nl_means(ints, h=20.0)
    assert host.dtype == np.float64
    dev = filters.nl_means(torch.from_numpy(ints.astype(np.float64)).to(gpu_device), h=20.0)
    assert np.array_equal(host, dev.cpu().numpy())
    # the defaults are scikit-image's
    s = np.array(images((40, 70)))[2]
    assert np.array_equal(restoration.denoise_nl_means(s), filters.nl_means(s, 7, 11, 0.1, 0.0))


def test_errors_and_the_empty_batch(gpu_device):
    from specenh import filters, restoration

    t = torch.rand(2, 8, 8, device=gpu_device)
    with pytest.raises(NotImplementedError, match="limit of 9"):
        run_op(t, (11, 11, 0.1, 0.0))
    with pytest.raises(NotImplementedError, match="limit of 15"):
        filters.nl_means(t, patch_distance=16)
    with pytest.raises(ValueError, match="odd"):
        restoration.denoise_nl_means(t[0], patch_size=4)
    with pytest.raises(ValueError, match="h must be finite and positive"):
        filters.nl_means(t, h=0)
    with pytest.raises(ValueError, match="sigma must be finite and not negative"):
        run_op(t, (7, 11, 0.1, -1.0))
    with pytest.raises(NotImplementedError, match="fast_mode=True"):
        restoration.denoise_nl_means(t[0], fast_mode=False)
    for dt in (torch.float32, torch.float64):
        e = run_op(t[:0].to(dt), PARAMS[0])
        assert e.shape == (0, 8, 8) and e.dtype == dt
    with pytest.raises(TypeError):
        run_op(t.half(), PARAMS[0])


def test_denoising_a_ridge_beats_the_noisy_input_and_the_bilateral_filter(gpu_device):
    """A ridge plus Gaussian noise of sigma 0.08 at 64 x 96, denoised with (7, 11, 0.8 sigma,
    sigma): the mean squared error against the clean ridge is lower than the noisy input's and
    lower than filters.bilateral's on the same input. The float64 restatements of both filters
    satisfy both inequalities (1.3e-4 against 6.5e-3 and 3.9e-3)."""
    from specenh import filters

    sigma = 0.08
    clean = nl.clean_ridge(64, 96)
    noisy = (clean + sigma * np.random.default_rng(5).standard_normal(clean.shape)).astype(
        np.float32)
    params = (7, 11, 0.8 * sigma, sigma)

    def mse(x):
        return float(((np.asarray(x, dtype=np.float64) - clean) ** 2).mean())

    q, B = nl.quotient64_and_bound(noisy, *params)
    assert mse(q) < mse(noisy) and mse(q) < mse(bl.bilateral(noisy.astype(np.float64)))
    out = filters.nl_means(noisy, *params)
    bil = filters.bilateral(noisy)
    print(f"\n[nlmeans denoising] mse noisy {mse(noisy):.3e}, nl_means {mse(out):.3e} "
          f"(restatement {mse(q):.3e}), bilateral {mse(bil):.3e}")
    assert_every_pixel(out, q, B, "ridge 64x96")
    assert mse(out) < mse(noisy)
    assert mse(out) < mse(bil)


def test_opcheck(gpu_device):
    for dt in (torch.float32, torch.float64):
        S = torch.rand(2, 16, 24, device=gpu_device, dtype=dt)
        torch.library.opcheck(torch.ops.specenh.nl_means, (S, 5, 3, 0.1, 0.05))
        torch.library.opcheck(torch.ops.specenh.nl_means, (S[0], 7, 2, 0.1, 0.0))
