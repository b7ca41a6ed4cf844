"""The complex FIR filter bank and the Morlet wavelet transform on the GPU
(csrc/filterbank.hip) against the float64 direct-sum restatement of tests/wavelet_local.py on
the fp32 samples widened.

The error of an FFT convolution scales with the largest output of a row, so it is measured per
(b, s) row on the row-max scale (wavelet_local.compare): max_j |out - ref| <= 1e-5 max_j |ref|
for the complex output, twice that for the power modes; tests/test_wavelet_cpu.py asserts that
a float32 run of the same formulation stays within a quarter of it. The inputs are seeded and
broadband; every signal row is strided with NaN in its padding and every output buffer is
NaN-filled before the launch. The tests print their measured values (pytest -s); DESIGN.md
5.14 records them.
"""
import numpy as np
import pytest
import torch

import wavelet_local as wl

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 13
DTYPES = {wl.COMPLEX: torch.complex64, wl.POWER: torch.float32, wl.MEAN: torch.float32}


def strided(dev, x):
    """x[B, L] on the device as rows of a [B, L + PAD] buffer whose padding is NaN."""
    x = np.atleast_2d(x)
    buf = torch.full((x.shape[0], x.shape[1] + PAD), NAN, device=dev)
    buf[:, :x.shape[1]] = torch.from_numpy(np.array(x)).to(dev)
    return buf[:, :x.shape[1]]


def launch(x, bank, hop, mode):
    """torch.ops.specenh.filterbank_out into a NaN-filled buffer."""
    To = wl.n_out(x.shape[1], hop, mode)
    fill = complex(NAN, NAN) if mode == wl.COMPLEX else NAN
    out = torch.full((x.shape[0], bank.nscales, To), fill, dtype=DTYPES[mode], device=x.device)
    torch.ops.specenh.filterbank_out(x, bank.tables, bank.lmax, hop, mode, out)
    assert not torch.isnan(torch.view_as_real(out) if mode == wl.COMPLEX else out).any(), \
        "an output element was not written"
    return out


def bank_of(dev, name):
    from specenh import wavelet as wv

    nfft, lmax = wl.CONFIGS[name][:2]
    bank = wv.FilterBank(wl.taps_of(name), nfft=nfft, device=dev, lmax=lmax)
    assert (bank.nfft, bank.lmax, bank.nscales) == (nfft, lmax, len(wl.taps_of(name)))
    return bank


@pytest.mark.parametrize("name", list(wl.CONFIGS))
def test_parity_with_the_fp64_restatement(gpu_device, name):
    """Every nfft at its largest Lmax and with a single tap, lengths around the block seams
    (every output compared: the first and last Lmax test the zero extension), hops 1, 3, 7, 37
    and V under both To rules, filter counts 1, 5, 33 of mixed lengths, random non-Hermitian
    and Morlet taps, in all three modes; and at every nfft the hops 1, 16, 17, 37 and V
    (hop{nfft}: the hop mean in one run and in two levels, whose partial sums go to the
    buffer the transform's pass count leaves free)."""
    dev = gpu_device
    bank = bank_of(dev, name)
    x = strided(dev, wl.signal_of(name))
    W = wl.reference(name)
    worst = {}
    for hop, mode in wl.cases(name):
        out = launch(x, bank, hop, mode).cpu().numpy()
        ref = wl.decimate(W, hop, mode)
        assert out.shape == ref.shape
        err = wl.compare(out, ref, mode)
        worst[mode] = max(worst.get(mode, 0.0), err)
        assert err <= wl.bound(mode), (hop, mode, err)
        if wl.CONFIGS[name][2] == ("one",) and mode == wl.COMPLEX:
            # a single tap [1]: the output is x itself, a zero imaginary part included
            xs = wl.signal_of(name).astype(np.float64)[:, None, :]
            assert np.abs(out - xs).max() <= wl.TOL * np.abs(xs).max()
    print(f"\n[filter bank {name}] max row error / row max: "
          + ", ".join(f"mode {m}: {e:.2e}" for m, e in worst.items())
          + f" (bounds {wl.TOL:.0e}, {2 * wl.TOL:.0e})")


@pytest.mark.parametrize("mode", (wl.COMPLEX, wl.POWER, wl.MEAN))
def test_batch_stride_and_position_do_not_change_a_bit(gpu_device, mode):
    """Row b of a batch of 5 with stride length + 13 equals the same shot run alone from a
    contiguous buffer (which also changes how the filters are split over workgroups)."""
    dev = gpu_device
    bank = bank_of(dev, "S33")
    length = wl.CONFIGS["S33"][3]
    x = wl.signal("white", 5, length, seed=77)
    hop = 1 if mode == wl.COMPLEX else 5
    full = launch(strided(dev, x), bank, hop, mode)
    for b in (0, 3, 4):
        alone = launch(torch.from_numpy(np.array(x[b:b + 1])).to(dev), bank, hop, mode)
        assert torch.equal(alone[0], full[b]), b


@pytest.mark.parametrize("mode", (wl.COMPLEX, wl.POWER, wl.MEAN))
def test_splitting_the_bank_does_not_change_a_bit(gpu_device, mode):
    """33 filters equal the rows of the same filters run as two banks of 16 and 17 with the
    same nfft and Lmax."""
    from specenh import wavelet as wv

    dev = gpu_device
    nfft, lmax = wl.CONFIGS["S33"][:2]
    taps = wl.taps_of("S33")
    x = strided(dev, wl.signal_of("S33"))
    hop = 1 if mode == wl.COMPLEX else 7
    whole = launch(x, bank_of(dev, "S33"), hop, mode)
    lo = launch(x, wv.FilterBank(taps[:16], nfft=nfft, device=dev, lmax=lmax), hop, mode)
    hi = launch(x, wv.FilterBank(taps[16:], nfft=nfft, device=dev, lmax=lmax), hop, mode)
    assert lo.shape[1] == 16 and hi.shape[1] == 17
    assert torch.equal(whole, torch.cat([lo, hi], dim=1))


@pytest.mark.parametrize("hop,mode", wl.CHUNK_CASES)
def test_filters_per_workgroup_do_not_change_a_bit(gpu_device, hop, mode):
    """The filter loop at 16, 8 and 4 filters a workgroup (SC): 33 filters, three chunks of 16
    with a single filter in the last. The kernel gives no way to observe SC, so the test rests
    on wavelet_local.filters_per_workgroup, the restatement of the rule specenh_filterbank
    plans by (csrc/filterbank_block.hpp) that tests/test_wavelet_cpu.py holds against the host code's text:
    with the device's CU count it gives the smallest batch B16 that keeps SC = 16, a batch B8
    that runs at SC = 8, and two shots at SC = 4. The first B8 and the first two shots run
    alone equal the rows of the B16 run bit for bit, and rows 0, 1 and the last of the B16 run
    are compared with the float64 direct sum: a loop of 16 filters, each with the next table
    row loaded under its transform, against a reference and not only against itself."""
    from specenh import wavelet as wv

    dev = gpu_device
    cfg = wl.CHUNK_CFG
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    B16, B8, B4 = wl.chunk_batches(hop, mode, cus)

    def sc(B):
        return wl.filters_per_workgroup(cfg["nfft"], cfg["lmax"], hop, mode, cfg["length"],
                                        cfg["S"], B, cus)

    assert (sc(B16), sc(B8), sc(B4)) == (16, 8, 4) and B4 < B8 < B16
    taps = wl.chunk_taps()
    bank = wv.FilterBank(taps, nfft=cfg["nfft"], device=dev, lmax=cfg["lmax"])
    assert (bank.nfft, bank.lmax, bank.nscales) == (256, 32, 33)
    x = wl.chunk_signal(B16)
    xd = strided(dev, x)
    full = launch(xd, bank, hop, mode)
    assert full.numel() * full.element_size() < 10e6
    for B, chunk in ((B8, 8), (B4, 4)):
        part = launch(xd[:B], bank, hop, mode)
        same = torch.equal(part, full[:B])
        print(f"\n[filters per workgroup, hop {hop} mode {mode}, {cus} CUs] {B} shots at SC = "
              f"{chunk} against {B16} shots at SC = 16: "
              f"{'bit-identical' if same else 'DIFFERENT'} (allowed: bit-identical)")
        assert same, (B, chunk)
    rows = [0, 1, B16 - 1]
    ref = wl.filter_bank_direct(x[rows], taps, hop, mode)
    err = wl.compare(full[rows].cpu().numpy(), ref, mode)
    print(f"[filters per workgroup, hop {hop} mode {mode}] SC = 16, rows {rows}: max row error "
          f"/ row max {err:.2e} (bound {wl.bound(mode):.0e})")
    assert err <= wl.bound(mode)


@pytest.mark.parametrize("hop,mode", ((1, wl.COMPLEX), (2, wl.POWER)))
def test_batches_above_the_grid_limit_are_sliced(gpu_device, hop, mode):
    """65,537 shots of 5 samples: the shots past the 65,535 of one launch equal the same shots
    run alone, and the restatement."""
    from specenh import wavelet as wv

    dev = gpu_device
    B, L = 65535 + 2, 5
    taps = wl.random_bank([1], seed=4)
    bank = wv.FilterBank(taps, nfft=256, device=dev)
    x = wl.signal("white", B, L, seed=8)
    full = launch(strided(dev, x), bank, hop, mode)
    assert full.shape == (B, 1, wl.n_out(L, hop, mode))
    tail = launch(strided(dev, x[65534:]), bank, hop, mode)
    assert torch.equal(full[65534:], tail)
    rows = [0, 65534, 65535, 65536]
    ref = wl.filter_bank_direct(x[rows], taps, hop, mode)
    assert wl.compare(full[rows].cpu().numpy(), ref, mode) <= wl.bound(mode)


def chirp_case():
    """A chirp plus noise, [2, 3000], and 11 Morlet scales from 2 to 64 samples, two an octave
    (the longest wavelet has L = 257: nfft 2048)."""
    from specenh import wavelet as wv

    x = wl.signal("chirp", 2, 3000, seed=5)
    scales = wv.morlet_scales(0.968 / 64.0, 0.968 / 2.0, 1.0, voices_per_octave=2)
    return x, scales


def test_cwt_against_the_restatement(gpu_device):
    from specenh import wavelet as wv

    x, scales = chirp_case()
    ref = wl.filter_bank_direct(x, wl.morlet(scales))
    xd = strided(gpu_device, x)
    W = wv.cwt(xd, scales)
    assert W.shape == ref.shape == (2, len(scales), 3000) and W.dtype == torch.complex64
    err = wl.compare(W.cpu().numpy(), ref)
    W4 = wv.cwt(xd.reshape(2, 1, 3000), scales, hop=4)   # leading axes, decimation
    assert W4.shape == (2, 1, len(scales), 750)
    err4 = wl.compare(W4[:, 0].cpu().numpy(), ref[..., ::4])
    one = wv.cwt(xd[1], scales)                          # 1-D input
    assert one.shape == (len(scales), 3000) and torch.equal(one, W[1])
    print(f"\n[cwt chirp + noise, {len(scales)} scales] max row error / row max: hop 1 "
          f"{err:.2e}, hop 4 {err4:.2e} (bound {wl.TOL:.0e})")
    assert err <= wl.TOL and err4 <= wl.TOL


def test_scalogram_is_the_hop_mean_of_the_cwt_power(gpu_device):
    from specenh import wavelet as wv

    x, scales = chirp_case()
    xd = strided(gpu_device, x)
    bank = wv.FilterBank(wv.morlet_filters(scales), device="cuda")  # no index: the current device
    assert bank.device == xd.device
    W = wv.cwt(xd, scales, bank=bank).cpu().numpy().astype(np.complex128)
    for hop in (16, 37):
        S = wv.scalogram(xd, scales, hop=hop, bank=bank)
        To = 3000 // hop
        assert S.shape == (2, len(scales), To) and S.dtype == torch.float32
        err = wl.compare(S.cpu().numpy(), wl.decimate(W, hop, wl.MEAN), wl.MEAN)
        P = wv.scalogram(xd, scales, hop=hop, mean=False, bank=bank)
        assert P.shape == (2, len(scales), (3000 - 1) // hop + 1)
        errp = wl.compare(P.cpu().numpy(), wl.decimate(W, hop, wl.POWER), wl.POWER)
        print(f"\n[scalogram hop {hop}] against the cwt's own power: mean {err:.2e}, sampled "
              f"{errp:.2e} (bound {2 * wl.TOL:.0e})")
        assert err <= 2 * wl.TOL and errp <= 2 * wl.TOL


def test_signal_cwt_returns_numpy(gpu_device):
    from specenh import signal
    from specenh import wavelet as wv

    x, scales = chirp_case()
    fs = 5e5
    want_f = wv.scale_to_frequency(scales, fs)
    f, t, W = signal.cwt(x.astype(np.float64), fs=fs, freqs=want_f, hop=2)
    assert isinstance(W, np.ndarray) and W.dtype == np.complex128 and W.shape == (2, len(scales), 1500)
    assert f.dtype == np.float64 and np.allclose(f, want_f, rtol=1e-14)
    assert np.array_equal(t, np.arange(1500) * 2 / fs)
    ref = wl.filter_bank_direct(x, wl.morlet(scales))[..., ::2]
    assert wl.compare(W, ref) <= wl.TOL
    # the default scales: 16 voices an octave from fs / 4 down to the longest wavelet allowed
    f2, t2, W2 = signal.cwt(x[0, :512], fs=fs)
    assert W2.shape == (f2.size, 512) and t2.size == 512
    assert abs(f2[0] - fs / 4) < 1e-6 and np.allclose(f2[:-1] / f2[1:], 2 ** (1 / 16))
    assert np.ceil(4.0 * wv.frequency_to_scale(f2[-1:], fs))[0] <= 1024


def test_ridge_of_a_linear_chirp(gpu_device):
    """The argmax over the scales of a linear chirp's scalogram follows the chirp's
    instantaneous frequency to within one scale step, outside the cone of influence."""
    from specenh import wavelet as wv

    L, f0, f1, hop = 8192, 0.02, 0.10, 8
    n = np.arange(L, dtype=np.float64)
    x = np.cos(2 * np.pi * (f0 * n + 0.5 * (f1 - f0) / L * n * n)).astype(np.float32)
    scales = wv.morlet_scales(0.015, 0.13, 1.0, voices_per_octave=16)
    P = wv.scalogram(torch.from_numpy(x).to(gpu_device), scales, hop=hop, mean=False)
    assert P.shape == (len(scales), L // hop)
    ridge = P.argmax(0).cpu().numpy()
    finst = f0 + (f1 - f0) / L * n[::hop]
    want = np.abs(np.log(wv.scale_to_frequency(scales)[:, None] / finst[None, :])).argmin(0)
    inside = ~wv.cone_of_influence(scales, L, hop)[want, np.arange(want.size)]
    assert inside.sum() > 0.9 * want.size
    off = np.abs(ridge - want)[inside]
    print(f"\n[ridge] {inside.sum()} columns outside the cone: |ridge - expected| max "
          f"{off.max()} scale steps, mean {off.mean():.3f}")
    assert off.max() <= 1


def test_opcheck(gpu_device):
    from specenh import wavelet as wv

    dev = gpu_device
    bank = wv.FilterBank(wl.random_bank([0, 9, 40], seed=3), nfft=256, device=dev)
    x = torch.from_numpy(np.array(wl.signal("white", 2, 500, seed=9))).to(dev)
    op, op_out = torch.ops.specenh.filterbank.default, torch.ops.specenh.filterbank_out.default
    for hop, mode in ((1, wl.COMPLEX), (3, wl.POWER), (20, wl.MEAN)):
        torch.library.opcheck(op, (x, bank.tables, bank.lmax, hop, mode))
        out = torch.empty((2, 3, wl.n_out(500, hop, mode)), dtype=DTYPES[mode], device=dev)
        torch.library.opcheck(op_out, (x, bank.tables, bank.lmax, hop, mode, out))
