"""GPU tests of top1_kernel_reg (svd_denoise.hip): the top-1 complement with X held in
registers, which the default kept range [1, r) takes for matrices up to 128 x 128 whose rows
are contiguous in X and in the output (m >= n, output rows aligned for 4-element stores). The
other orientation, and everything under the switch SVD_TOP1_LDS=1, stays on top1_kernel.

Tolerance as tests/test_svd_top1_gpu.py: 1e-5 relative (Frobenius) against the float64 oracle
for fp32 outputs. An fp16 output is the same fp32 value rounded once more, so it must equal
the fp32 output's own rounding bit for bit; against the oracle its bound is TOL plus fp16's
half-ulp 2^-11 per element (2^-25 absolute for subnormal elements).

The C ABI takes dense m x n matrices (row pitch n) with a batch stride, so a row pitch or an
output pitch larger than r cannot be reached from here; the batch stride, the guards at the
padding edges and the neighbours of the output are what these tests can see."""
import ctypes
import os
import sys

import numpy as np
import pytest

from oracle import svd as ref

pytestmark = pytest.mark.gpu
TOL = 1e-5
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

SHAPES = [(4, 128), (128, 4), (8, 8), (124, 128), (128, 124), (64, 64), (128, 128)]


def _err(got, want, A):
    nw, na = np.linalg.norm(want), np.linalg.norm(A)
    return np.linalg.norm(got - want) / max(nw, 0.01 * na, 1e-300)


def _tol16(want, A):
    """TOL + fp16 rounding of every element, relative to _err's denominator."""
    den = max(np.linalg.norm(want), 0.01 * np.linalg.norm(A), 1e-300)
    return TOL + 2.0 ** -11 * (1 + TOL) * np.linalg.norm(want) / den + np.sqrt(want.size) * 2.0 ** -25 / den


def _capi(At, m, n, a_stride=None, out=None):
    """specenh_svd_denoise_ex, default range, on the device tensor At (flat or [B, m, n]) ->
    (out tensor, kernel symbols, top1 flags or None). `out`: a device tensor whose first
    B*m*n elements are written (fp32 or fp16)."""
    import torch

    from specenh import _lib

    L = _lib.lib()
    a_stride = a_stride or m * n
    B = At.numel() // a_stride
    r = min(m, n)
    if out is None:
        out = torch.empty((B, m, n), dtype=torch.float32, device=At.device)
    odt = {torch.float32: 0, torch.float16: 2}[out.dtype]
    nb = int(L.specenh_svd_denoise_workspace_bytes(B, m, n, 1, r))
    ws = torch.zeros(nb, dtype=torch.uint8, device=At.device)
    n0 = _lib.launch_count()
    _lib.check(L.specenh_svd_denoise_ex(ctypes.c_void_p(At.data_ptr()), B, m, n, a_stride, 1, r,
                                        ctypes.c_void_p(out.data_ptr()), odt,
                                        ctypes.c_void_p(ws.data_ptr()), None))
    torch.cuda.synchronize()
    names = _lib.kernel_names(n0, _lib.launch_count())
    flags = None
    if r >= 8:  # the subspace workspace layout: G, V, theta, then the flags (256-byte aligned)
        off = ((B * r * r + B * r + B) * 4 + 255) // 256 * 256
        flags = ws[off:off + 4 * B].view(torch.int32).cpu().numpy()
    return out, names, flags


def _which(names):
    if any("top1_kernel_reg" in s for s in names):
        return "reg"
    return "lds" if any("top1_kernel" in s for s in names) else None


@pytest.mark.parametrize("shape", SHAPES)
def test_reg_and_lds_kernels_match_oracle(gpu_device, shape, kernel_variant):
    import torch

    from make_golden import gapped_matrix

    m, n = shape
    A = np.stack([gapped_matrix(300 + i, m, n, k=min(16, min(m, n)), dtype=np.float32)
                  for i in range(5)])
    At = torch.as_tensor(A, device=gpu_device)
    want = [ref.denoiseSignal(A[b].astype(np.float64)) for b in range(len(A))]
    res = {}
    for lds in (0, 1):
        kernel_variant("SVD_TOP1_LDS", lds)
        o32, names, _ = _capi(At, m, n)
        assert _which(names) == ("reg" if m >= n and not lds else "lds"), names
        o16, names16, _ = _capi(At, m, n, out=torch.empty((5, m, n), dtype=torch.float16,
                                                          device=gpu_device))
        assert _which(names16) == _which(names)
        assert torch.equal(o16, o32.half())  # rounded once more, from the same fp32 value
        res[lds] = o32.double().cpu().numpy()
        g16 = o16.double().cpu().numpy()
        for b in range(len(A)):
            e32, e16 = _err(res[lds][b], want[b], A[b]), _err(g16[b], want[b], A[b])
            print(f"{shape} SVD_TOP1_LDS={lds} matrix {b}: fp32 err {e32:.3e}, fp16 err {e16:.3e}")
            assert e32 <= TOL, (lds, b, e32)
            assert e16 <= _tol16(want[b], A[b]), (lds, b, e16)
    d = max(_err(res[0][b], res[1][b], A[b]) for b in range(len(A)))
    print(f"{shape}: reg vs LDS kernel, max relative difference {d:.3e}")  # reported, not bounded


def test_reg_rank_deficient_zero_and_ties(gpu_device):
    """Rank 1, 2, 3 and the zero matrix (dead basis columns), a near-tie of the top pair
    (theta gap 2e-3) and an exact tie (flagged; compared in singular values)."""
    import torch

    rng = np.random.default_rng(11)
    mats = []
    for k in (1, 2, 3):
        mats.append(((rng.standard_normal((128, k)) * np.array([5.0, 1.0, 0.3][:k]))
                     @ rng.standard_normal((k, 128))).astype(np.float32))
    mats.append(np.zeros((128, 128), dtype=np.float32))
    rng = np.random.default_rng(3)
    u, _ = np.linalg.qr(rng.standard_normal((128, 128)))
    v, _ = np.linalg.qr(rng.standard_normal((128, 128)))
    s = 0.01 * rng.uniform(0.5, 1.0, 128)
    for second in (10.0 * (1 - 1e-3), 10.0):
        s2 = s.copy()
        s2[0], s2[1] = 10.0, second
        mats.append(((u * s2) @ v.T).astype(np.float32))
    A = np.stack(mats)
    out, names, flags = _capi(torch.as_tensor(A, device=gpu_device), 128, 128)
    assert _which(names) == "reg", names
    got = out.double().cpu().numpy()
    assert np.all(np.isfinite(got))
    for b in range(5):
        want = ref.denoiseSignal(A[b].astype(np.float64))
        assert _err(got[b], want, A[b]) <= TOL, (b, _err(got[b], want, A[b]))
    assert not np.any(got[3])
    assert flags[5] == 1  # no gap: left to the fp64 eigen path
    sv_got = np.linalg.svd(got[5], compute_uv=False)
    sv_want = np.linalg.svd(ref.denoiseSignal(A[5].astype(np.float64)), compute_uv=False)
    assert np.max(np.abs(sv_got - sv_want)) <= TOL * sv_want[0]


def test_reg_flags_noise_for_the_fallback(gpu_device):
    """Noise matrices between gapped ones: the kernel flags those that do not converge in 24
    rounds, the one-launch fp64 fallback overwrites exactly them, every output meets the bound."""
    import torch

    from make_golden import gapped_matrix

    rng = np.random.default_rng(23)
    mats = [gapped_matrix(1500 + i, 128, 128, dtype=np.float32) if i % 3 else
            rng.standard_normal((128, 128)).astype(np.float32) for i in range(12)]
    A = np.stack(mats)
    out, names, flags = _capi(torch.as_tensor(A, device=gpu_device), 128, 128)
    assert _which(names) == "reg", names
    assert any("eig_fallback_kernel" in s for s in names), names
    assert set(np.unique(flags)) <= {0, 1}
    assert not np.any(flags[np.arange(12) % 3 != 0])
    assert np.any(flags[::3]), flags
    got = out.double().cpu().numpy()
    for b in range(12):
        want = ref.denoiseSignal(A[b].astype(np.float64))
        assert _err(got[b], want, A[b]) <= TOL, (b, flags[b], _err(got[b], want, A[b]))


@pytest.mark.parametrize("shape", [(128, 124), (124, 124), (8, 8)])
def test_reg_batch_stride_and_output_neighbours(gpu_device, shape):
    """A batch stride larger than the matrix with NaN in the gaps (never read), and an output
    slice between sentinel matrices (never written past the row and column guards)."""
    import torch

    from make_golden import gapped_matrix

    m, n = shape
    B, stride = 6, m * n + 64
    A = np.stack([gapped_matrix(900 + i, m, n, k=min(16, n), dtype=np.float32) for i in range(B)])
    buf = torch.full((B * stride,), float("nan"), dtype=torch.float32, device=gpu_device)
    buf.view(B, stride)[:, :m * n] = torch.as_tensor(A.reshape(B, -1), device=gpu_device)
    big = torch.full((B + 2, m, n), 777.0, dtype=torch.float32, device=gpu_device)
    _, names, _ = _capi(buf, m, n, a_stride=stride, out=big[1:B + 1])
    assert _which(names) == "reg", names
    assert torch.all(big[0] == 777.0) and torch.all(big[B + 1] == 777.0)
    got = big[1:B + 1].double().cpu().numpy()
    for b in range(B):
        want = ref.denoiseSignal(A[b].astype(np.float64))
        assert _err(got[b], want, A[b]) <= TOL, (b, _err(got[b], want, A[b]))


def test_reg_large_batch_is_deterministic(gpu_device):
    """600 matrices (more than the resident workgroups of any device): two runs are bitwise
    equal, and a matrix gives the same bits at batch index 0, 37 and 8 q."""
    import torch

    from make_golden import gapped_matrix

    base = np.stack([gapped_matrix(40 + i, 128, 128, dtype=np.float32) for i in range(8)])
    A = base[np.arange(600) % 8]
    A[37] = base[0]
    At = torch.as_tensor(A, device=gpu_device)
    o1, names, flags = _capi(At, 128, 128)
    o2, _, _ = _capi(At, 128, 128)
    assert _which(names) == "reg", names
    assert not np.any(flags)
    assert torch.equal(o1, o2)
    assert torch.equal(o1[37], o1[0])
    idx = torch.arange(600, device=gpu_device) % 8
    idx[37] = 0
    assert torch.equal(o1, o1[:8][idx])
    got = o1[:8].double().cpu().numpy()
    for b in range(8):
        want = ref.denoiseSignal(base[b].astype(np.float64))
        assert _err(got[b], want, base[b]) <= TOL, (b, _err(got[b], want, base[b]))


def test_dispatch(gpu_device, kernel_variant):
    """Contiguous orientation -> top1_kernel_reg; transposed orientation, an output that is not
    aligned for the 16-byte stores, and SVD_TOP1_LDS=1 -> top1_kernel."""
    import torch

    from make_golden import gapped_matrix

    tall = torch.as_tensor(gapped_matrix(5, 128, 96, dtype=np.float32)[None], device=gpu_device)
    wide = torch.as_tensor(gapped_matrix(6, 96, 128, dtype=np.float32)[None], device=gpu_device)
    assert _which(_capi(tall, 128, 96)[1]) == "reg"
    assert _which(_capi(wide, 96, 128)[1]) == "lds"
    shifted = torch.empty(128 * 96 + 4, dtype=torch.float32, device=gpu_device)
    o, names, _ = _capi(tall, 128, 96, out=shifted[1:])
    assert _which(names) == "lds", names
    want = _capi(tall, 128, 96)[0]
    assert _err(o[:128 * 96].view(128, 96).double().cpu().numpy(),
                want[0].double().cpu().numpy(), tall[0].cpu().numpy()) <= TOL
    kernel_variant("SVD_TOP1_LDS", 1)
    assert _which(_capi(tall, 128, 96)[1]) == "lds"
    assert _which(_capi(wide, 96, 128)[1]) == "lds"


def test_reg_c5_spectrograms(gpu_device, kernel_variant):
    """64 spectrograms of the C5 chain (128 x 128 log spectrograms of the synthetic plasma
    chirps): none flagged by either kernel, oracle parity for both. (The rounds each kernel
    needs on them: tools/top1_stats.py on the stats build.)"""
    import torch

    import bench
    from specenh import pipeline_data
    from specenh.synthetic import plasma_chirps_torch

    x = plasma_chirps_torch(64, bench.L5, seed=1000, device=gpu_device).to(torch.float16)
    S = torch.empty((64, 128, 128), dtype=torch.float32, device=gpu_device)
    pipeline_data.specgr_batch(x, bench.SPEC5, out=S)
    A = S.cpu().numpy()
    want = [ref.denoiseSignal(A[b].astype(np.float64)) for b in range(64)]
    for lds in (0, 1):
        kernel_variant("SVD_TOP1_LDS", lds)
        out, names, flags = _capi(S, 128, 128)
        assert _which(names) == ("lds" if lds else "reg")
        assert not np.any(flags)
        got = out.double().cpu().numpy()
        for b in range(64):
            assert _err(got[b], want[b], A[b]) <= TOL, (lds, b, _err(got[b], want[b], A[b]))
