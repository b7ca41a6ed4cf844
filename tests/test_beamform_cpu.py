"""Host-side checks of the steered-response spectra (no GPU): the extension header, ctypes
table, exports, operators and constants in sync; the call contract of specenh_array_spectrum
against the table the five averaging entries share, and the argument errors of
specenh_steered_power, all raised before the device is touched (host stand-in plan, pointers
never followed); the argument errors of the tensor and numpy layers; meta shapes; the steering
tables against the float64 formula; and the fp64 restatement (tests/beamform_local.py) against
itself: Bartlett from eigenpairs against a^T S conj(a) / |a|^4 on scipy.signal.csd matrices
(measured 2.1e-15 at 5 channels and 4.2e-15 at 40, normwise; allowed 1e-13: some hundred
roundings of float64 in the C^2 terms of the quadratic form and in eigh), the peaks of the three estimators at the injected
mode numbers."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import beamform_local as bl
from conftest import REPO
from test_averaging_contract_cpu import COMMON, FAULTS, L, P, run

HEADER = os.path.join(REPO, "include", "specenh_beamform.h")
LIB = os.path.join(REPO, "spectrogram-enhancement_amd", "specenh", "libspecenh.so")

ORDER = ("plan", "x", "batch", "channels", "length", "channel_stride", "batch_stride", "navg", "a",
         "nsteer", "a_per_bin", "out", "workspace", "workspace_bytes", "stream")
VALID = dict(x=P, channels=5, channel_stride=L, batch_stride=5 * L, a=P, nsteer=7, a_per_bin=0,
             out=P)
BYTES = ("plan", "batch", "channels", "length", "navg")


def entry(**change):
    return run("specenh_array_spectrum", ORDER, **dict(VALID, **change))


def nbytes(**change):
    return run("specenh_array_spectrum_workspace_bytes", BYTES, **dict(VALID, **change))


def declared_functions():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(specenh_[a-z0-9_]+)\s*\(", src)))


def test_header_ctypes_table_exports_and_operators_agree():
    from specenh import _lib, ops  # noqa: F401  (ops registers the operators)

    names = declared_functions()
    assert names == ["specenh_array_spectrum", "specenh_array_spectrum_workspace_bytes",
                     "specenh_steered_power"]
    assert sorted(_lib.SIGNATURES_BEAMFORM) == names
    for table in (_lib.SIGNATURES, _lib.SIGNATURES_STFT_COMPLEX, _lib.SIGNATURES_SPECTRAL,
                  _lib.SIGNATURES_CSM, _lib.SIGNATURES_MODES, _lib.SIGNATURES_BISPECTRUM,
                  _lib.SIGNATURES_WAVENUMBER, _lib.SIGNATURES_CORRELATION):
        assert not set(_lib.SIGNATURES_BEAMFORM) & set(table)
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\bT (specenh_[a-z0-9_]+)", out))
    assert not [n for n in names if n not in exported]
    lib = _lib.lib()
    for n, (res, args) in _lib.SIGNATURES_BEAMFORM.items():
        assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == args
    # the argument lists of the header, type by type
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    ctype = {"long long": ctypes.c_longlong, "int": ctypes.c_int, "double": ctypes.c_double,
             "size_t": ctypes.c_size_t}
    for n, (_, args) in _lib.SIGNATURES_BEAMFORM.items():
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % n, src).group(1)
        want = []
        for arg in decl.split(","):
            arg = " ".join(arg.split())
            want.append(ctypes.c_void_p if "*" in arg else ctype[arg.rsplit(" ", 1)[0]])
        assert want == args, n
    for op in ("steered_power", "steered_power_out", "array_spectrum_out"):
        assert getattr(torch.ops.specenh, op).default._schema.name == f"specenh::{op}"
    text = open(HEADER).read()
    assert '#include "specenh.h"' in text
    for name, value in (("MAX_CHANNELS", _lib.STEER_MAX_CHANNELS),
                        ("MAX_NSTEER", _lib.STEER_MAX_NSTEER), ("SUM", _lib.STEER_SUM),
                        ("BARTLETT", _lib.STEER_BARTLETT), ("INVERSE", _lib.STEER_INVERSE),
                        ("MUSIC", _lib.STEER_MUSIC)):
        assert int(re.search(r"#define SPECENH_STEER_%s (\d+)" % name, text).group(1)) == value
    assert (_lib.STEER_MAX_CHANNELS, _lib.STEER_MAX_NSTEER) == (64, 4096)


def test_the_valid_call_is_valid_up_to_the_launch():
    from specenh import _lib

    assert not set(VALID) & set(COMMON) and set(ORDER) == set(VALID) | set(COMMON)
    assert entry(batch=0)[0] == _lib.SPECENH_OK
    assert nbytes()[0] > 0 and nbytes(batch=0)[0] == 0
    # the bytes of specenh_csm_workspace_bytes
    assert nbytes()[0] == run("specenh_csm_workspace_bytes", BYTES, **VALID)[0]
    assert nbytes(channels=64)[0] == run("specenh_csm_workspace_bytes", BYTES,
                                         **dict(VALID, channels=64))[0]


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_shared_fault_reads_as_from_the_averaging_entries(fault):
    from specenh import _lib

    change, code, text, in_bytes = FAULTS[fault]
    if change == "need - 1":
        change = dict(workspace_bytes=nbytes()[0] - 1)
    assert entry(**change) == (getattr(_lib, code), text)
    if in_bytes:
        assert nbytes(**change) == (0, text)


def test_array_spectrum_argument_errors():
    from specenh import _lib

    E = _lib.SPECENH_EINVAL
    assert entry(channel_stride=L - 1) == (E, "channel_stride < length")
    assert entry(batch_stride=5 * L - 1) == (E, "batch_stride < channels * channel_stride")
    assert entry(x=None) == (E, "null x")
    assert entry(a=None) == (E, "null a")
    assert entry(a=ctypes.c_void_p(4100)) == (E, "a must be 8-byte aligned")
    assert entry(out=None) == (E, "null out")
    for ns in (0, -1, 4097):
        assert entry(nsteer=ns) == (E, "nsteer must be in [1, 4096]")
    for ch in (0, 65):
        assert entry(channels=ch, batch_stride=65 * L) == (E, "channels must be in [1, 64]")
        assert nbytes(channels=ch) == (0, "channels must be in [1, 64]")
    # nothing to do: OK with the workspace null; a fault of the call is still a fault
    assert entry(batch=0, workspace=None)[0] == _lib.SPECENH_OK
    assert entry(batch=0, workspace=None, navg=129)[0] == E
    assert entry(batch=0, workspace=None, nsteer=0)[0] == E
    assert entry(batch=0, a=None)[0] == E


def test_steered_power_argument_errors():
    from specenh import _lib

    lib = _lib.lib()
    E = _lib.SPECENH_EINVAL

    def call(v=P, w=None, a=P, count=6, rows=4, channels=5, nsteer=7, vms=20, vrs=5, a_count=1,
             a_inner=1, conj_a=0, scale=1.0, scale_table=None, post=0, out=P):
        rc = lib.specenh_steered_power(v, w, a, count, rows, channels, nsteer, vms, vrs, a_count,
                                       a_inner, conj_a, scale, scale_table, post, out, None)
        return rc, _lib.last_error()

    assert call(v=None) == (E, "null v")
    assert call(a=None) == (E, "null a")
    assert call(v=ctypes.c_void_p(4100)) == (E, "v must be 8-byte aligned")
    assert call(a=ctypes.c_void_p(4100)) == (E, "a must be 8-byte aligned")
    assert call(count=-1) == (E, "count must be >= 0")
    for rows in (0, -2):
        assert call(rows=rows) == (E, "rows must be >= 1")
    assert call(rows=(1 << 30) + 1, vms=1 << 40) == (E, "too many rows")
    for ch in (0, 65):
        assert call(channels=ch, vrs=65, vms=400) == (E, "channels must be in [1, 64]")
    for ns in (0, 4097):
        assert call(nsteer=ns) == (E, "nsteer must be in [1, 4096]")
    assert call(vrs=4) == (E, "v_row_stride < channels")
    assert call(vms=19) == (E, "v_matrix_stride < (rows - 1) * v_row_stride + channels")
    for ac, ai in ((0, 1), (1, 0), (-3, 2)):
        assert call(a_count=ac, a_inner=ai) == (E, "a_count and a_inner must be >= 1")
    for ac, ai in ((4, 1), (3, 4), (2, 6)):  # 6 matrices are not whole [.., a_count, a_inner]
        assert call(a_count=ac, a_inner=ai) == (E, "count must be a multiple of a_count * a_inner")
    for post in (-1, 4):
        assert call(post=post) == (E, "post must be in [0, 3]")
    assert call(out=None) == (E, "null out")
    # nothing to do, nothing touched
    assert call(count=0)[0] == _lib.SPECENH_OK
    assert call(count=0, a_count=3, a_inner=2)[0] == _lib.SPECENH_OK
    assert call(count=0, post=4)[0] == E


def test_python_argument_errors():
    from specenh import beamform, signal

    x = torch.zeros(2, 5, 4096)
    A = beamform.steering_vectors(np.linspace(0, 1, 5), np.arange(-3, 4))
    assert A.shape == (7, 5) and A.dtype == torch.complex64
    with pytest.raises(ValueError, match="method must be one of"):
        beamform.array_spectrum(x, A, method="esprit")
    for ns in (0, 5, -1):
        with pytest.raises(ValueError, match=r"nsources must be in \[1, 4\]"):
            beamform.array_spectrum(x, A, method="music", nsources=ns)
    for ld in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="loading must be >= 0"):
            beamform.array_spectrum(x, A, method="capon", loading=ld)
    with pytest.raises(TypeError, match="torch.Tensor"):
        beamform.array_spectrum(x, A.numpy())
    with pytest.raises(ValueError, match="A must be complex"):
        beamform.array_spectrum(x, torch.zeros(7, 5))
    with pytest.raises(ValueError, match="A must be complex"):
        beamform.array_spectrum(x, torch.zeros(7, 4, dtype=torch.complex64))
    with pytest.raises(ValueError, match="A must be complex"):
        beamform.array_spectrum(x, torch.zeros(100, 7, 5, dtype=torch.complex64))  # F = 129
    with pytest.raises(ValueError, match="A must be complex"):
        beamform.array_spectrum(x, torch.zeros(5, dtype=torch.complex64))
    with pytest.raises(ValueError, match="K must be in"):
        beamform.array_spectrum(x, torch.zeros(4097, 5, dtype=torch.complex64))
    with pytest.raises(ValueError, match="noverlap must be less than nperseg."):
        beamform.array_spectrum(x, A, nperseg=256, noverlap=256)
    with pytest.raises(NotImplementedError, match="power of two"):
        beamform.array_spectrum(x, A, nperseg=200)
    with pytest.raises(ValueError, match="shorter than nperseg"):
        beamform.array_spectrum(torch.zeros(2, 5, 100), A)
    with pytest.raises(ValueError, match="navg"):
        beamform.array_spectrum(x, A, navg=32)  # T = 31
    with pytest.raises(ValueError, match="channels must be in"):
        beamform.array_spectrum(torch.zeros(2, 1, 4096), A[:, :1])
    with pytest.raises(TypeError, match="torch.Tensor"):
        beamform.array_spectrum(np.zeros((5, 4096)), A)
    with pytest.raises(ValueError, match="nmax"):
        beamform.mode_number_spectrum(x, np.linspace(0, 1, 5), -1)
    V = torch.zeros(3, 4, 5, dtype=torch.complex64)
    with pytest.raises(ValueError, match="post must be one of"):
        beamform.steered_power(V, None, A, post="capon")
    with pytest.raises(ValueError, match="V must be complex"):
        beamform.steered_power(torch.zeros(3, 4, 5), None, A)
    with pytest.raises(ValueError, match="w must be a tensor"):
        beamform.steered_power(V, torch.zeros(3, 5), A)
    with pytest.raises(ValueError, match="positions must be"):
        beamform.steering_vectors(np.zeros((2, 2)), [1.0])
    with pytest.raises(ValueError, match="delays"):
        beamform.delay_steering([1.0, 2.0], np.zeros(5))

    xn = np.zeros((5, 4096))
    with pytest.raises(ValueError, match="method must be one of"):
        signal.array_spectrum(xn, A, method="esprit")
    with pytest.raises(ValueError, match="A must be complex"):
        signal.array_spectrum(xn, np.zeros((7, 5)))
    with pytest.raises(ValueError, match="at least 2-D"):
        signal.array_spectrum(np.zeros(4096), A)
    with pytest.raises(NotImplementedError, match="median"):
        signal.array_spectrum(xn, A, average="median")
    with pytest.raises(NotImplementedError, match="nfft"):
        signal.array_spectrum(xn, A, nperseg=256, nfft=512)
    with pytest.raises(NotImplementedError, match="two-sided"):
        signal.array_spectrum(xn, A, return_onesided=False)
    with pytest.raises(NotImplementedError, match="complex"):
        signal.array_spectrum(np.zeros((5, 4096), dtype=np.complex64), A)


def test_cpu_tensors_are_refused_after_validation():
    from specenh import beamform

    x = torch.zeros(2, 5, 4096)
    A = beamform.steering_vectors(np.linspace(0, 1, 5), np.arange(-3, 4))
    for method in beamform.METHODS:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            beamform.array_spectrum(x, A, method=method, nsources=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        beamform.mode_number_spectrum(x[0], np.linspace(0, 1, 5), 3, navg=4)
    V = torch.zeros(3, 4, 5, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        beamform.steered_power(V, None, A)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.steered_power(V, None, A, 0, 1.0, False, None)
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.steered_power_out(V, None, A, 0, 1.0, False, None, torch.zeros(3, 7))
    with pytest.raises(NotImplementedError):
        torch.ops.specenh.array_spectrum_out(x, 256, 128, "hann", 1.0, 0, 1, 0, A,
                                             torch.zeros(2, 129, 1, 7), None)


def test_meta_shapes():
    m = torch.device("meta")
    V = torch.empty(2, 5, 3, 8, 6, dtype=torch.complex64, device=m)
    A = torch.empty(7, 6, dtype=torch.complex64, device=m)
    q = torch.ops.specenh.steered_power(V, None, A, 0, 1.0, False, None)
    assert q.shape == (2, 5, 3, 7) and q.dtype == torch.float32
    w = torch.empty(2, 5, 3, 8, device=m)
    Af = torch.empty(5, 7, 6, dtype=torch.complex64, device=m)
    q = torch.ops.specenh.steered_power(V, w, Af, 3, 1.0, False, None)
    assert q.shape == (2, 5, 3, 7) and q.dtype == torch.float32
    q = torch.ops.specenh.steered_power(torch.empty(8, 6, dtype=torch.complex64, device=m), None,
                                        A, 2, 2.0, True, None)
    assert q.shape == (7,)


def test_steering_tables_equal_the_float64_formula_rounded_once():
    from specenh import beamform

    rng = np.random.default_rng(3)
    p = np.sort(rng.uniform(0, 2 * np.pi, 11))
    kappa = np.concatenate((np.arange(-20, 21), rng.uniform(-40, 40, 9)))
    a = beamform.steering_vectors(p, kappa)
    want = np.exp(1j * kappa[:, None] * p[None, :]).astype(np.complex64)
    assert a.shape == (50, 11) and a.dtype == torch.complex64 and a.is_contiguous()
    assert np.array_equal(a.numpy().view(np.float32), want.view(np.float32))
    assert np.array_equal(want, bl.steering(p, kappa).astype(np.complex64))
    f = np.fft.rfftfreq(64, 1 / 5e5)
    tau = rng.uniform(-2e-5, 2e-5, (9, 11))
    d = beamform.delay_steering(f, tau)
    want = np.exp(-2j * np.pi * f[:, None, None] * tau[None]).astype(np.complex64)
    assert d.shape == (33, 9, 11) and d.dtype == torch.complex64 and d.is_contiguous()
    assert np.array_equal(d.numpy().view(np.float32), want.view(np.float32))
    assert np.array_equal(d[0].numpy(), np.ones((9, 11), np.complex64))  # f = 0


N_MODES = bl.N_MODES
CPU32_Q, CPU32_INV = 5.12e-7, 9.59e-7  # what tests/test_beamform_gpu.py takes 4 x of


def test_channel_cases_visit_every_instantiation_and_channel_count():
    """steered_power_kernel<KH> is picked by (C - 1) / 8: eight kernels, eight channel counts
    each, both boundaries of each (C = 1 and 0 mod 8), one to four row tiles with a partial
    last one, K at one wave, a full workgroup and a second one."""
    src = open(os.path.join(REPO, "spectrogram-enhancement_amd", "csrc",
                            "steered_power.hip")).read()
    assert "kernels[(p.C - 1) / 8]" in src  # the rule bl.instantiation restates
    assert [int(k) for k in re.findall(r"steered_power_kernel<(\d+)>", src)] == \
        [4 * (i + 1) for i in range(8)]
    cases = bl.CHANNEL_CASES
    assert [c[1] for c in cases] == list(range(1, 65))
    by_kernel = {}
    for M, C, K, count, per_bin in cases:
        by_kernel.setdefault(bl.instantiation(C), []).append(C)
        assert M > 1 and M % 32 and count == 3
    assert sorted(by_kernel) == list(range(8))
    for i, cs in by_kernel.items():
        assert cs == list(range(8 * i + 1, 8 * i + 9))
    assert {-(-c[0] // 32) for c in cases} == {1, 2, 3, 4}
    assert {-(-c[2] // 128) for c in cases} == {1, 2} and {c[2] for c in cases} >= {1, 129, 130}
    assert {c[4] for c in cases} == {False, True}
    # what KERNEL_CASES visits of the channel axis, as its comment says
    assert sorted({bl.instantiation(c[1]) for c in bl.KERNEL_CASES}) == [0, 3, 4, 7]


def test_float32_restatement_on_the_channel_cases_is_within_the_recorded_error():
    """The precondition for holding the kernel to TOL_Q and TOL_INV (4 x the fp32 restatement's
    error on KERNEL_CASES) at every channel count: on CHANNEL_CASES the fp32 restatement is no
    further from fp64 than on KERNEL_CASES. Measured 4.27e-7, 4.58e-7, 5.23e-7, 4.24e-7; the
    recorded 5.12e-7 and 9.59e-7 are recomputed on KERNEL_CASES."""
    worst = bl.restatement32_error(bl.CHANNEL_CASES)
    print("[channel cases, fp32 restatement] SUM %.2e BARTLETT %.2e (allowed %.2e) INVERSE %.2e "
          "MUSIC %.2e (allowed %.2e)" % (worst[0], worst[1], CPU32_Q, worst[2], worst[3],
                                         CPU32_INV))
    assert max(worst[:2]) <= CPU32_Q and max(worst[2:]) <= CPU32_INV
    rec = bl.restatement32_error(bl.KERNEL_CASES)
    print("[kernel cases, fp32 restatement] SUM %.3e BARTLETT %.3e INVERSE %.3e MUSIC %.3e"
          % tuple(rec))
    assert "%.2e" % max(rec[:2]) == "%.2e" % CPU32_Q
    assert "%.2e" % max(rec[2:]) == "%.2e" % CPU32_INV


@pytest.mark.parametrize("C", bl.E2E_CHANNELS)
def test_chain32_holds_what_the_procedure_computes(C):
    """CHAIN32 (the end-to-end bound of Capon and MUSIC against scipy matrices is 8 x it) is
    bl.chain32 on this machine to two significant digits: within half a unit of the second
    digit of the recorded value."""
    got = bl.chain32(C)
    for method in ("capon", "music"):
        rec = bl.CHAIN32[(C, method)]
        half_unit = 0.05 * 10.0 ** np.floor(np.log10(rec))
        print(f"[C={C} {method}] fp32 solver + fp64 projection against all fp64: "
              f"{got[method]:.3e} (recorded {rec:.2e})")
        assert abs(got[method] - rec) <= half_unit


def test_the_restatement_without_power():
    """No power and no loading: the Capon terms have no weight, q = 0, P = 1 / 0 = inf; Bartlett
    is 0, MUSIC C / (C - p). A term with a zero denominator beside live ones is dropped, as the
    pseudo-inverse does; any loading keeps every term."""
    C = 5
    A = bl.steering(bl.angles(C), N_MODES)
    Z = np.zeros((C, C), np.complex128)
    assert np.isposinf(bl.estimate(Z, A, "capon", 2, 1e-2)).all()
    assert (bl.estimate(Z, A, "bartlett") == 0).all()
    assert np.allclose(bl.estimate(Z, A, "music", 2), C / (C - 2), rtol=1e-12)
    lam, v = np.array([2.0, 1.0, 0.0, 0.0, 0.0]), np.eye(C)
    got = bl.from_eigenpairs(lam, v, A, "capon", loading=0.0)
    assert np.allclose(got, 1.0 / (np.abs(A[:, 0]) ** 2 / 2.0 + np.abs(A[:, 1]) ** 2), rtol=1e-12)
    loaded = bl.from_eigenpairs(lam, v, A, "capon", loading=1e-2)
    d = lam + 1e-2 * 3.0 / C
    assert np.allclose(loaded, 1.0 / (np.abs(A) ** 2 / d).sum(-1), rtol=1e-12)


@pytest.mark.parametrize("C", [5, 40])
def test_the_restatement_is_self_consistent(C):
    x = bl.signals(1, C, 64 + 16 * 39)  # T = 40 frames of 64 / 48
    S = bl.scipy_csm(x, 64, 48, "hann", "constant", 0)  # [1, 33, 1, C, C]
    A = bl.steering(bl.angles(C), N_MODES)
    lam, v = bl.eigenpairs(S)
    direct = bl.bartlett(S, A)
    err = bl.normwise(bl.from_eigenpairs(lam, v, A, "bartlett"), direct)
    print(f"[C={C}] Bartlett from eigenpairs vs a^T S conj(a) / |a|^4: {err:.2e} (allowed 1e-13)")
    assert err <= 1e-13
    # the raw sum against a plain loop, per bin tables too
    V, At, w = bl.kernel_case(3, 4, 5, 7, True)
    q = bl.raw_q(V, w, At)
    for j in range(7):
        P = V[j, 0].astype(np.complex128) @ At[j].astype(np.complex128).T
        assert np.allclose(q[j, 0], (w[j, 0][:, None] * np.abs(P) ** 2).sum(0), rtol=1e-13)
    # all three peak at n = 3 in both bands; MUSIC (2 sources) resolves {3, -2}
    for k in bl.BINS:
        for method in ("bartlett", "capon", "music"):
            p = bl.estimate(S[0, k, 0], A, method, 2, 1e-2)
            assert N_MODES[np.argmax(p)] == 3, (k, method)
        p = bl.estimate(S[0, k, 0], A, "music", 2)
        assert p.min() >= 1 - 1e-12
        assert set(N_MODES[bl.local_maxima(p)[:2]]) == {3, -2}, k
    # the gap nsources = 2 relies on
    gap = min(float(lam[0, k, 0, 1] / lam[0, k, 0, 2]) for k in bl.BINS)
    print(f"[C={C}] lambda_2 / lambda_3 in the bands: {gap:.1f}")
    assert gap >= 9
