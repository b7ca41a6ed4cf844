"""The SVD denoiser stays inside the workspace its size query promises, on every layout the
host dispatch of svd_denoise.hip has: specenh_svd_denoise_ex called through ctypes with a
workspace of exactly specenh_svd_denoise_workspace_bytes, uninitialised like the one ops.py
allocates, followed by a guard that must come back untouched; the output must equal the same
call through specenh.svd bit for bit."""
import pytest

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5
BATCH = 3

# (m, n, start, stop); None = denoiseSignal's default range [1, r)
CASES = [
    (16, 16, None, None),    # top-1, flags and fallback region of the subspace layout
    (128, 128, None, None),
    (4, 4, None, None),      # top-1, r too small for a subspace: eigen region, then the flags
    (40, 24, 0, 4),          # subspace, X = A, direct
    (40, 24, 2, 24),         # subspace, X = A, complement
    (24, 40, 0, 4),          # subspace, X = A^T, direct
    (24, 40, 2, 24),         # subspace, X = A^T, complement
    (20, 12, 0, 10),         # eigen path
    (40, 24, 3, 3),          # empty range: zeros, no workspace use
    (40, 24, 0, 24),         # whole range: copy, no workspace use
]


@pytest.mark.parametrize("out_dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("m,n,start,stop", CASES)
def test_svd_stays_inside_its_workspace(gpu_device, m, n, start, stop, out_dtype):
    import torch

    from specenh import _lib, svd

    odt = getattr(torch, out_dtype)
    g = torch.Generator().manual_seed(1000 * m + n)
    A = torch.randn(BATCH, m, n, generator=g).to(gpu_device)
    want = svd.denoise_batch(A, start, stop,
                             out=torch.empty(BATCH, m, n, dtype=odt, device=gpu_device))

    s, e = svd._resolve(min(m, n), start, stop)
    L = _lib.lib()
    nbytes = int(L.specenh_svd_denoise_workspace_bytes(BATCH, m, n, s, e))
    buf = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=gpu_device)
    buf[nbytes:].fill_(FILL)
    got = torch.empty(BATCH, m, n, dtype=odt, device=gpu_device)
    _lib.check(L.specenh_svd_denoise_ex(A.data_ptr(), BATCH, m, n, m * n, s, e, got.data_ptr(),
                                        svd._OUT_DTYPES[odt], buf.data_ptr(),
                                        _lib.current_stream_handle(A.device)), "svd_denoise_ex")
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == FILL).all()), "wrote past the workspace"
    assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))
