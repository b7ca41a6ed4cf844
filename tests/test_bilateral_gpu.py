"""GPU parity of the bilateral label filter (csrc/bilateral.hip) against the numpy restatement
of tests/bilateral_local.py.

The criterion is the one of include/specenh_bilateral.h: with q64 the quotient in float64 over
the float32 tables and n the tap count, |out - q64| <= 0.5 + 255 (2 n + 3) 2^-24 at EVERY
pixel. Shapes are the smallest at which tiling and reflection can go wrong: images smaller than
the radius (reflection repeats), one below / at / one above the kernel's tile in either
direction, more than two tiles both ways. The composition (quantise, filter, rescale) is
checked bit for bit against the 8-bit filter's own output."""
import functools

import numpy as np
import pytest
import torch

import bilateral_local as bl
from oracle import filters as of

pytestmark = pytest.mark.gpu

from specenh import _lib  # noqa: E402

TR, TC = _lib.BILATERAL_TILE_ROWS, _lib.BILATERAL_TILE_COLS
PARAMS = [(15, 75.0, 75.0), (5, 10.0, 2.0), (0, 30.0, 3.0), (9, 200.0, 1.5), (1, 50.0, 50.0),
          (15, 0.0, -1.0), (31, 75.0, 10.0)]
SHAPES = [(1, 1), (1, 9), (9, 1), (5, 3), (16, 16), (TR - 1, TC + 1), (TR, TC), (TR + 1, TC - 1),
          (2 * TR + 3, 2 * TC + 5), (64, 48)]
PAD = 13  # bytes between the images of a strided batch


@functools.lru_cache(maxsize=None)
def images(shape):
    """Three images of a shape: noise, smooth, noise; read-only."""
    rows, cols = shape
    seed = 1000 * rows + cols
    b = np.stack([bl.noise_image(rows, cols, seed), bl.smooth_image(rows, cols, seed + 1),
                  bl.noise_image(rows, cols, seed + 2)])
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def truth(shape, params):
    q = np.stack([bl.quotient64(u, *params) for u in images(shape)])
    q.setflags(write=False)
    return q


def strided(batch, pad, dev):
    """The images of `batch` [B, rows, cols] uint8 on the device, `pad` bytes apart."""
    B, rows, cols = batch.shape
    buf = torch.full((B, rows * cols + pad), 255, dtype=torch.uint8, device=dev)
    buf[:, :rows * cols] = torch.from_numpy(np.array(batch)).to(dev).reshape(B, -1)
    return buf[:, :rows * cols].view(B, rows, cols)


def run_u8(img, params):
    return torch.ops.specenh.bilateral_u8(img, int(params[0]), float(params[1]), float(params[2]))


def assert_every_pixel(out, q64, n, what):
    err = np.abs(out.astype(np.float64) - q64)
    worst = float(err.max()) - 0.5
    print(f"\n[bilateral {what}] worst |out - q64| - 0.5 = {worst:.3e} (bound {bl.delta(n):.3e}), "
          f"{int((out != np.rint(q64)).sum())} of {out.size} pixels differ from rint(q64)")
    bad = np.argwhere(err > 0.5 + bl.delta(n))
    assert bad.size == 0, (what, bad[:5].tolist(), worst)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("params", PARAMS, ids=lambda p: f"d{p[0]}-sc{p[1]:g}-ss{p[2]:g}")
def test_u8_parity_every_pixel(gpu_device, params, shape):
    """Batch 3 with a padded stride."""
    u = images(shape)
    out = run_u8(strided(u, PAD, gpu_device), params)
    assert out.shape == u.shape and out.dtype == torch.uint8 and out.is_contiguous()
    n = bl.taps(params[0], params[2])[1]
    assert_every_pixel(out.cpu().numpy(), truth(shape, params), n, f"{params} {shape}")


@pytest.mark.parametrize("params", [(15, 75.0, 75.0), (0, 30.0, 3.0), (31, 75.0, 10.0)],
                         ids=lambda p: f"d{p[0]}")
def test_u8_is_deterministic_across_batch_position_stride_and_runs(gpu_device, params):
    """The same image at batch positions 0, 1, 2 and at two strides gives identical bytes; two
    runs give identical bytes."""
    for shape in ((2 * TR + 3, 2 * TC + 5), (5, 3), (TR + 1, TC - 1)):
        u = images(shape)
        same = np.stack([u[1], u[1], u[1]])
        a = run_u8(strided(same, PAD, gpu_device), params)
        b = run_u8(strided(same, 0, gpu_device), params)
        c = run_u8(strided(same, 4096 + 1, gpu_device), params)
        assert torch.equal(a[0], a[1]) and torch.equal(a[0], a[2])
        assert torch.equal(a, b) and torch.equal(a, c)
        mixed = strided(u, PAD, gpu_device)
        m1, m2 = run_u8(mixed, params), run_u8(mixed, params)
        assert torch.equal(m1, m2)
        assert torch.equal(m1[1], a[0])           # alone or beside other images
        single = run_u8(torch.from_numpy(np.array(u[1:2])).to(gpu_device), params)
        assert torch.equal(single[0], a[0])


def test_u8_does_not_touch_the_padding_or_the_input(gpu_device):
    shape = (TR + 1, TC + 1)
    u = images(shape)
    img = strided(u, PAD, gpu_device)
    before = img.clone()
    out = run_u8(img, PARAMS[0])
    assert torch.equal(img, before)
    assert_every_pixel(out.cpu().numpy(), truth(shape, PARAMS[0]), 149, "padding")


def _spectrogram(rows, cols, seed):
    """A ridge on noise, like a mode on a spectrogram's background."""
    rng = np.random.default_rng(seed)
    r = np.arange(rows)[:, None]
    c = np.arange(cols)[None, :]
    ridge = np.exp(-0.5 * ((r - rows * (0.3 + 0.4 * c / cols)) / 2.0) ** 2)
    return ridge + 0.3 * rng.random((rows, cols))


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_composition_is_rescale_of_the_filtered_quantisation(gpu_device, dtype):
    """specenh_bilateral = rescale_u8(bilateral_u8(to_u8(src))) bit for bit, per image of a
    batch and through every Python entry."""
    from specenh import filters, pipeline_data

    for shape, params in (((40, 70), (15, 75.0, 75.0)), ((TR + 1, TC + 3), (5, 10.0, 2.0)),
                          ((9, 1), (0, 30.0, 3.0))):
        S = np.stack([_spectrogram(*shape, seed=s) for s in (1, 2, 3)]).astype(dtype)
        q = np.stack([of.to_u8(s) for s in S])
        f = run_u8(torch.from_numpy(q).to(gpu_device), params).cpu().numpy()
        want = np.stack([of.rescale_u8(x) for x in f]).astype(dtype)
        t = torch.from_numpy(S).to(gpu_device)
        got = filters.bilateral(t, *params)
        assert got.dtype == t.dtype and got.shape == t.shape and got.device == t.device
        assert np.array_equal(got.cpu().numpy(), want)
        for b in range(3):                       # a batch equals the per-image calls
            one = filters.bilateral(t[b], *params)
            assert one.shape == shape and np.array_equal(one.cpu().numpy(), want[b])
        op = torch.ops.specenh.bilateral(t, int(params[0]), params[1], params[2])
        assert np.array_equal(op.cpu().numpy(), want)
        host = pipeline_data.bilateral(S[0], d=params[0], sigma_color=params[1],
                                       sigma_space=params[2])
        # as for gaussblr, float32 numpy is computed and returned in float32, all else in float64
        assert host.dtype == dtype and host.shape == shape
        assert np.array_equal(host, want[0])
    s = _spectrogram(40, 70, seed=4)
    assert np.array_equal(pipeline_data.bilateral(s),
                          filters.bilateral(torch.from_numpy(s).to(gpu_device)).cpu().numpy())


def test_constant_image_gives_nan_like_gaussblr(gpu_device):
    from specenh import filters, pipeline_data

    c = np.full((12, 20), 3.25)
    with np.errstate(invalid="ignore"):
        out = pipeline_data.bilateral(c)
        blur = pipeline_data.gaussblr(c)
    assert out.shape == c.shape and np.isnan(out).all() and np.isnan(blur).all()
    # a constant 8-bit image passes the filter unchanged
    u = torch.full((2, 12, 20), 77, dtype=torch.uint8, device=gpu_device)
    assert torch.equal(run_u8(u, PARAMS[0]), u)
    # beside a constant image the others are unaffected
    S = np.stack([_spectrogram(12, 20, seed=1), c])
    got = filters.bilateral(torch.from_numpy(S).to(gpu_device)).cpu().numpy()
    assert np.isnan(got[1]).all()
    assert np.array_equal(got[0], pipeline_data.bilateral(S[0]))


@pytest.mark.parametrize("shape", [(128, 128), (256, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_reference_defaults_against_the_restatement(gpu_device, shape):
    """pipeline_data.bilateral(s) with the reference's (15, 75, 75), at the uint8 level: the
    level is recovered as out (max - min) + min of the restated image where the two images'
    minima and maxima agree, and read from bilateral_u8 otherwise."""
    from specenh import pipeline_data

    s = _spectrogram(*shape, seed=7)
    out = pipeline_data.bilateral(s)
    assert out.dtype == np.float64 and out.shape == shape
    u = of.to_u8(s)
    q64 = bl.quotient64(u)
    R = np.rint(q64).astype(np.uint8)
    G = run_u8(torch.from_numpy(u[None]).to(gpu_device), (15, 75.0, 75.0))[0].cpu().numpy()
    if (G.min(), G.max()) == (R.min(), R.max()):
        mn, mx = float(R.min()), float(R.max())
        level = out * (mx - mn) + mn
        assert np.abs(level - np.rint(level)).max() < 1e-9     # a level is an integer
        level = np.rint(level)
    else:
        level = G.astype(np.float64)
    assert_every_pixel(level, q64, 149, f"defaults {shape}")
    assert np.array_equal(out, of.rescale_u8(G))
    restated = bl.bilateral(s)
    print(f"[bilateral defaults {shape}] max |out - restatement| = "
          f"{np.abs(out - restated).max():.3e}")


def test_unsupported_radius_and_bad_input_raise(gpu_device):
    from specenh import filters

    u = torch.zeros((1, 8, 8), dtype=torch.uint8, device=gpu_device)
    with pytest.raises(NotImplementedError, match="limit of 15"):
        run_u8(u, (33, 75.0, 75.0))
    with pytest.raises(NotImplementedError, match="limit of 15"):
        filters.bilateral(torch.rand(8, 8, device=gpu_device), d=0, sigma_space=11.0)
    with pytest.raises(ValueError, match="finite"):
        run_u8(u, (15, float("nan"), 75.0))
    assert run_u8(u[:0], PARAMS[0]).shape == (0, 8, 8)


def test_opcheck(gpu_device):
    u = torch.from_numpy(np.array(images((16, 16)))).to(gpu_device)
    torch.library.opcheck(torch.ops.specenh.bilateral_u8, (u, 15, 75.0, 75.0))
    S = torch.rand(2, 16, 24, device=gpu_device, dtype=torch.float64)
    torch.library.opcheck(torch.ops.specenh.bilateral, (S, 5, 10.0, 2.0))
