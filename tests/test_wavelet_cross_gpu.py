"""The cross spectrum of a pair through a filter bank and wavelet coherence on the GPU
(csrc/filterbank_cross.hip) against the float64 direct-sum restatement of
tests/wavelet_cross_local.py on the fp32 samples widened.

Per (b, s) row: max_j |sxx - ref| <= 2e-5 max_j ref (syy likewise), and max_j |sxy - ref| <=
2e-5 sqrt(max_j Sxx_ref max_j Syy_ref); coherence per element within the first-order propagation
of those three (wavelet_cross_local.coherence_allowance). tests/test_wavelet_cross_cpu.py
asserts that a float32 run of the same formulation stays within a quarter of each. The inputs
are seeded pairs with coherence from near 1 to near 0.1; every signal row is strided with NaN in
its padding and every output buffer is NaN-filled before the launch. The tests print their
measured values (pytest -s); DESIGN.md 5.15 records them.
"""
import numpy as np
import pytest
import torch

import wavelet_cross_local as xl
import wavelet_local as wl

pytestmark = pytest.mark.gpu

NAN = float("nan")
PAD = 13


def strided(dev, x, pad=PAD):
    """x[B, L] on the device as rows of a [B, L + pad] buffer whose padding is NaN."""
    x = np.atleast_2d(x)
    buf = torch.full((x.shape[0], x.shape[1] + pad), NAN, device=dev)
    buf[:, :x.shape[1]] = torch.from_numpy(np.array(x)).to(dev)
    return buf[:, :x.shape[1]]


def launch(x, y, bank, hop, mode, autos=True):
    """torch.ops.specenh.filterbank_cross_out into NaN-filled buffers: (sxy, sxx, syy)."""
    shape = (x.shape[0], bank.nscales, xl.n_out(x.shape[1], hop, mode))
    sxy = torch.full(shape, complex(NAN, NAN), dtype=torch.complex64, device=x.device)
    sxx = torch.full(shape, NAN, device=x.device) if autos else None
    syy = torch.full(shape, NAN, device=x.device) if autos else None
    torch.ops.specenh.filterbank_cross_out(x, y, bank.tables, bank.lmax, hop, mode, sxy, sxx, syy)
    for o in (torch.view_as_real(sxy), sxx, syy):
        assert o is None or not torch.isnan(o).any(), "an output element was not written"
    return sxy, sxx, syy


def to_numpy(out):
    return tuple(o.cpu().numpy() for o in out)


def bank_of(dev, name):
    from specenh import wavelet as wv

    nfft, lmax = wl.CONFIGS[name][:2]
    bank = wv.FilterBank(wl.taps_of(name), nfft=nfft, device=dev, lmax=lmax)
    assert (bank.nfft, bank.lmax, bank.nscales) == (nfft, lmax, len(wl.taps_of(name)))
    return bank


@pytest.mark.parametrize("name", list(wl.CONFIGS))
def test_parity_with_the_fp64_restatement(gpu_device, name):
    """Both modes at every configuration of wavelet_local: hop{nfft} at hops 1, 16, 17, 37 and V
    (the hop mean in one run and in two levels, a partial run, one output a block), every nfft
    at its largest Lmax and with a single tap, the seam lengths at 256 and 4096, 1, 5 and 33
    filters, the three Morlet banks (y delayed by 3 samples). x and y have different strides."""
    dev = gpu_device
    bank = bank_of(dev, name)
    x, y = xl.pair_of(name)
    xd, yd = strided(dev, x), strided(dev, y, PAD + 4)
    Wx, Wy = xl.reference(name)
    worst = np.zeros(3)
    for hop, mode in xl.cases(name):
        out = to_numpy(launch(xd, yd, bank, hop, mode))
        ref = xl.cross(Wx, Wy, hop, mode)
        errs = xl.compare(out, ref)
        worst = np.maximum(worst, errs)
        assert max(errs) <= xl.BOUND, (hop, mode, errs)
        if wl.CONFIGS[name][2] == ("one",) and mode == xl.POINT and hop == 1:
            # a single tap [1]: sxy = x y with a zero imaginary part, sxx = x^2
            x64, y64 = x.astype(np.float64)[:, None, :], y.astype(np.float64)[:, None, :]
            top = np.sqrt((x64 ** 2).max(-1) * (y64 ** 2).max(-1))[..., None]
            assert (np.abs(out[0] - x64 * y64) <= xl.BOUND * top).all()
            assert (np.abs(out[1] - x64 ** 2) <= xl.BOUND * (x64 ** 2).max(-1)[..., None]).all()
    print(f"\n[cross spectrum {name}] max row error: sxy / sqrt(max sxx max syy) {worst[0]:.2e}, "
          f"sxx {worst[1]:.2e}, syy {worst[2]:.2e} (bound {xl.BOUND:.0e})")


@pytest.mark.parametrize("name", ("hop256", "hop4096", "morlet1024-dc50"))
def test_x_passed_as_y(gpu_device, name):
    """The same tensor as x and y: Im sxy = 0 and Re sxy = sxx = syy within the sxy bound."""
    dev = gpu_device
    bank = bank_of(dev, name)
    xd = strided(dev, xl.pair_of(name)[0])
    worst = 0.0
    for hop, mode in xl.cases(name):
        sxy, sxx, syy = to_numpy(launch(xd, xd, bank, hop, mode))
        top = sxx.astype(np.float64).max(-1, keepdims=True)
        err = max((np.abs(sxy.imag) / top).max(), (np.abs(sxy.real - sxx) / top).max(),
                  (np.abs(syy - sxx) / top).max())
        worst = max(worst, float(err))
        assert err <= xl.BOUND, (hop, mode, err)
    print(f"\n[x as y, {name}] max(|Im sxy|, |Re sxy - sxx|, |syy - sxx|) / row max sxx "
          f"{worst:.2e} (bound {xl.BOUND:.0e})")


@pytest.mark.parametrize("mode", (xl.POINT, xl.MEAN))
def test_batch_stride_and_position_do_not_change_a_bit(gpu_device, mode):
    """Row b of a batch of 5 with strides length + 13 and length + 17 equals the same pair run
    alone from contiguous buffers (which also changes the split of the filters)."""
    dev = gpu_device
    bank = bank_of(dev, "S33")
    length = wl.CONFIGS["S33"][3]
    x, y = wl.signal("white", 5, length, seed=77), wl.signal("chirp", 5, length, seed=78)
    hop = 1 if mode == xl.POINT else 37
    full = launch(strided(dev, x), strided(dev, y, PAD + 4), bank, hop, mode)
    for b in (0, 3, 4):
        alone = launch(torch.from_numpy(np.array(x[b:b + 1])).to(dev),
                       torch.from_numpy(np.array(y[b:b + 1])).to(dev), bank, hop, mode)
        for a, f in zip(alone, full):
            assert torch.equal(a[0], f[b]), b


@pytest.mark.parametrize("mode", (xl.POINT, xl.MEAN))
def test_splitting_the_bank_does_not_change_a_bit(gpu_device, mode):
    """33 filters equal the rows of the same filters run as two banks of 16 and 17 with the
    same nfft and Lmax."""
    from specenh import wavelet as wv

    dev = gpu_device
    nfft, lmax = wl.CONFIGS["S33"][:2]
    taps = wl.taps_of("S33")
    x, y = xl.pair_of("S33")
    xd, yd = strided(dev, x), strided(dev, y)
    hop = 1 if mode == xl.POINT else 17
    whole = launch(xd, yd, bank_of(dev, "S33"), hop, mode)
    lo = launch(xd, yd, wv.FilterBank(taps[:16], nfft=nfft, device=dev, lmax=lmax), hop, mode)
    hi = launch(xd, yd, wv.FilterBank(taps[16:], nfft=nfft, device=dev, lmax=lmax), hop, mode)
    assert lo[0].shape[1] == 16 and hi[0].shape[1] == 17
    for w, a, b in zip(whole, lo, hi):
        assert torch.equal(w, torch.cat([a, b], dim=1))


@pytest.mark.parametrize("hop,mode", xl.CHUNK_CASES)
def test_filters_per_workgroup_do_not_change_a_bit(gpu_device, hop, mode):
    """The filter loop at 16, 8 and 4 filters a workgroup: 33 filters, three chunks of 16 with a
    single filter in the last. specenh_filterbank_cross_chunk (cus = 0: this device) gives the
    smallest batch that keeps 16, the smallest that runs at 8, and two pairs run at 4: every
    value the host rule can produce. The first rows agree bit for bit across them, and rows 0,
    1 and the last of the largest run are compared with the float64 direct sum."""
    from specenh import ops
    from specenh import wavelet as wv

    dev = gpu_device
    cfg = wl.CHUNK_CFG

    def sc(nb):
        return ops.filterbank_cross_chunk(cfg["S"], cfg["nfft"], cfg["lmax"], nb, cfg["length"],
                                          hop, mode, cus=0)

    B16 = next(nb for nb in range(1, 4096) if sc(nb) == 16)
    B8 = next(nb for nb in range(1, B16) if sc(nb) == 8)
    B4 = 2
    assert (sc(B16), sc(B8), sc(B4)) == (16, 8, 4) and B4 < B8 < B16
    assert {sc(nb) for nb in range(1, B16 + 1)} == {4, 8, 16}
    taps = wl.chunk_taps()
    bank = wv.FilterBank(taps, nfft=cfg["nfft"], device=dev, lmax=cfg["lmax"])
    x, y = xl.chunk_pair(B16)
    xd, yd = strided(dev, x), strided(dev, y)
    full = launch(xd, yd, bank, hop, mode)
    assert sum(o.numel() * o.element_size() for o in full) < 32e6
    for nb, chunk in ((B8, 8), (B4, 4)):
        part = launch(xd[:nb], yd[:nb], bank, hop, mode)
        same = all(torch.equal(p, f[:nb]) for p, f in zip(part, full))
        print(f"\n[filters per workgroup, hop {hop} mode {mode}] {nb} pairs at {chunk} filters a "
              f"workgroup against {B16} pairs at 16: "
              f"{'bit-identical' if same else 'DIFFERENT'} (allowed: bit-identical)")
        assert same, (nb, chunk)
    rows = [0, 1, B16 - 1]
    Wx, Wy = wl.filter_bank_direct(x[rows], taps), wl.filter_bank_direct(y[rows], taps)
    errs = xl.compare(tuple(o[rows].cpu().numpy() for o in full), xl.cross(Wx, Wy, hop, mode))
    print(f"[filters per workgroup, hop {hop} mode {mode}] 16 a workgroup, rows {rows}: max row "
          f"error sxy {errs[0]:.2e}, sxx {errs[1]:.2e}, syy {errs[2]:.2e} (bound {xl.BOUND:.0e})")
    assert max(errs) <= xl.BOUND


@pytest.mark.parametrize("name,hop,mode", (("hop256", 1, xl.POINT), ("hop1024", 16, xl.MEAN),
                                           ("hop4096", 37, xl.MEAN)))
def test_cross_spectrum_alone_has_the_same_bits(gpu_device, name, hop, mode):
    """sxx = syy = None: the same sxy."""
    dev = gpu_device
    bank = bank_of(dev, name)
    x, y = xl.pair_of(name)
    xd, yd = strided(dev, x), strided(dev, y)
    both = launch(xd, yd, bank, hop, mode)
    alone = launch(xd, yd, bank, hop, mode, autos=False)
    assert alone[1] is None and alone[2] is None
    assert torch.equal(torch.view_as_real(alone[0]), torch.view_as_real(both[0]))


@pytest.mark.parametrize("name", ("hop256", "hop1024"))
def test_autos_have_the_bits_of_the_single_signal_kernel(gpu_device, name):
    """sxx and syy equal filterbank's power (point) and mean power (mean) of x and of y bit for
    bit, at every hop and mode of the configuration: the two kernels take the block load, the
    product and the hop mean's summation order from csrc/filterbank_block.hpp. hop256 runs
    fft_lds::stockham (NI = 1), hop1024 BlockFft (NI = 4)."""
    dev = gpu_device
    bank = bank_of(dev, name)
    x, y = xl.pair_of(name)
    xd, yd = strided(dev, x), strided(dev, y, PAD + 4)
    for hop, mode in xl.cases(name):
        _, sxx, syy = launch(xd, yd, bank, hop, mode)
        for auto, v in ((sxx, xd), (syy, yd)):
            alone = torch.ops.specenh.filterbank(v, bank.tables, bank.lmax, hop, xl.fb_mode(mode))
            assert torch.equal(auto, alone), (hop, mode)


def test_batches_above_the_grid_limit_are_sliced(gpu_device):
    """65,537 pairs of 5 samples: the pairs past the 65,535 of one launch equal the same pairs
    run alone, and the restatement."""
    from specenh import wavelet as wv

    dev = gpu_device
    nb, L = 65535 + 2, 5
    taps = wl.random_bank([1], seed=4)
    bank = wv.FilterBank(taps, nfft=256, device=dev)
    x, y = wl.signal("white", nb, L, seed=8), wl.signal("white", nb, L, seed=9)
    full = launch(strided(dev, x), strided(dev, y), bank, 2, xl.MEAN)
    assert full[0].shape == (nb, 1, 2)
    tail = launch(strided(dev, x[65534:]), strided(dev, y[65534:]), bank, 2, xl.MEAN)
    for f, t in zip(full, tail):
        assert torch.equal(f[65534:], t)
    rows = [0, 65534, 65535, 65536]
    ref = xl.cross(wl.filter_bank_direct(x[rows], taps), wl.filter_bank_direct(y[rows], taps),
                   2, xl.MEAN)
    assert max(xl.compare(tuple(o[rows].cpu().numpy() for o in full), ref)) <= xl.BOUND


def test_wavelet_coherence_end_to_end(gpu_device):
    """wavelet_coherence on hop1024 at hop 16 (the bank passed in; the scales only count its
    filters) with no smoothing, five windows, and a width per filter: coherence within the
    propagated bound of the float64 restatement, applied to the smoothed spectra; the phase
    within |dSxy| / |Sxy| where the coherence is not small."""
    from specenh import wavelet as wv

    dev = gpu_device
    name, hop = "hop1024", 16
    bank = bank_of(dev, name)
    x, y = xl.pair_of(name)
    xd, yd = strided(dev, x), strided(dev, y, PAD + 4)
    raw = xl.cross(*xl.reference(name), hop, xl.MEAN)
    scales = np.arange(1.0, bank.nscales + 1.0)
    for smooth in (1, 5, [1, 3, 5, 9, 33]):
        coh, phase, sxy = wv.wavelet_coherence(xd, yd, scales, hop=hop, smooth=smooth, bank=bank)
        assert coh.shape == phase.shape == sxy.shape == (xl.B, 5, x.shape[1] // hop)
        assert coh.dtype == phase.dtype == torch.float32 and sxy.dtype == torch.complex64
        coh, phase = coh.cpu().numpy().astype(np.float64), phase.cpu().numpy().astype(np.float64)
        widths = np.full(5, smooth) if np.isscalar(smooth) else np.asarray(smooth)
        ref, ref_phase, rxy, rxx, ryy = xl.coherence(*raw, widths)
        allow = xl.coherence_allowance(ref, rxx, ryy)
        used = np.abs(coh - ref) / allow
        strong = ref > 0.25
        dphi = np.abs(np.angle(np.exp(1j * (phase - ref_phase))))
        print(f"\n[wavelet coherence {name} hop {hop} smooth {smooth}] range {ref.min():.3f} .. "
              f"{ref.max():.3f}; |coh - ref| max {np.abs(coh - ref).max():.2e}, at most "
              f"{used.max():.1%} of the allowed error (which peaks at {allow.max():.2e}); phase "
              f"error where coh > 0.25: {dphi[strong].max():.2e} rad")
        assert allow.max() <= xl.COH_ALLOWED_MAX
        assert (used <= 1.0).all() and coh.max() <= 1.0 and coh.min() >= 0.0
        # |d angle| <= asin(|dSxy| / |Sxy|), |dSxy| <= 2 TOL sqrt(Mxx Myy); the float32 phase
        # adds its own rounding, 2^-23 of pi
        top = np.sqrt(rxx.max(-1, keepdims=True) * ryy.max(-1, keepdims=True))
        assert (dphi <= 1.01 * xl.BOUND * top / np.abs(rxy) + np.pi * 2.0 ** -23)[strong].all()


def test_wavelet_coherence_of_a_delayed_pair(gpu_device):
    """The public functions on a Morlet bank with the default smoothing: y is x (white) delayed
    by 3 samples plus noise. Coherence against the restatement; where it is above 0.9 in the
    least noisy pair, inside the cone of influence, the phase is minus the scale's frequency
    times the delay: to the 1.4 % by which the Fourier-equivalent frequency exceeds the
    response's peak w0 / s (0.02 rad of the 1.5 at the shortest scale) and the scatter of a
    coherence estimate, sqrt((1 - c) / (2 c n)) < 0.1 rad for c > 0.9 and n >= 3 windows."""
    from specenh import signal
    from specenh import wavelet as wv

    dev = gpu_device
    L, hop, d = 6000, 16, 3
    x, y = xl.make_pair("white", L, 5, d)
    scales = wv.morlet_scales(0.968 / 64.0, 0.968 / 12.0, 1.0, voices_per_octave=2)
    widths = wv.smoothing_windows(scales, hop)
    assert widths.tolist() == [3, 3, 5, 7, 9, 13]
    coh, phase, sxy = wv.wavelet_coherence(strided(dev, x), strided(dev, y), scales, hop=hop)
    assert coh.shape == phase.shape == sxy.shape == (xl.B, len(scales), L // hop)
    assert coh.dtype == phase.dtype == torch.float32 and sxy.dtype == torch.complex64
    taps = wl.morlet(scales)
    raw = xl.cross(wl.filter_bank_direct(x, taps), wl.filter_bank_direct(y, taps), hop, xl.MEAN)
    ref, ref_phase, rxy, rxx, ryy = xl.coherence(*raw, widths)
    allow = xl.coherence_allowance(ref, rxx, ryy)
    got = coh.cpu().numpy().astype(np.float64)
    used = np.abs(got - ref) / allow
    print(f"\n[wavelet coherence, delayed pair] range {ref.min():.3f} .. {ref.max():.3f}, at "
          f"most {used.max():.1%} of the allowed error (which peaks at {allow.max():.2e})")
    assert (used <= 1.0).all() and got.max() <= 1.0 and got.min() >= 0.0
    w = 2 * np.pi * wv.scale_to_frequency(scales)
    sel = ~wv.cone_of_influence(scales, L, hop)[:, :L // hop] & (ref[0] > 0.9)
    assert sel.mean() > 0.5
    off = np.abs(np.angle(np.exp(1j * (phase[0].cpu().numpy() + w[:, None] * d))))[sel]
    print(f"[wavelet coherence, delayed pair] {sel.sum()} elements above 0.9: |phase + w d| max "
          f"{off.max():.3f} rad, mean {off.mean():.3f} (allowed 0.5, 0.15)")
    assert off.mean() < 0.15 and off.max() < 0.5
    # the numpy front end: the same numbers, window centres as times
    fs = 5e5
    f, t, c2, p2 = signal.wavelet_coherence(x, y, fs=fs, freqs=wv.scale_to_frequency(scales, fs),
                                            hop=hop)
    assert np.allclose(f, wv.scale_to_frequency(scales, fs), rtol=1e-14)
    assert np.array_equal(t, (np.arange(L // hop) + 0.5) * hop / fs)
    assert c2.dtype == np.float64 and p2.dtype == np.float64
    assert np.abs(c2 - ref).max() <= np.abs(got - ref).max() + 1e-6 and c2.shape == got.shape


def test_broadcasting_of_the_leading_dimensions(gpu_device):
    """One reference channel against three: x [L] with y [3, L] equals x repeated."""
    from specenh import wavelet as wv

    dev = gpu_device
    bank = bank_of(dev, "S5")
    x, y = xl.pair_of("S5")
    xd, yd = strided(dev, x), strided(dev, y)
    a = wv.cross_filter_bank(xd[0], yd, bank, hop=7)
    b = wv.cross_filter_bank(xd[:1].expand(3, -1).contiguous(), yd, bank, hop=7)
    c = wv.cross_filter_bank(xd[0].reshape(1, 1, -1), yd.reshape(3, 1, -1), bank, hop=7)
    for u, v, w in zip(a, b, c):
        assert u.shape == (3, 5, 1041 // 7) and torch.equal(u, v)
        assert w.shape == (3, 1, 5, 1041 // 7) and torch.equal(w[:, 0], u)


@pytest.mark.parametrize("name,hop,mode", (("hop512", 1, xl.POINT), ("hop4096", 37, xl.MEAN)))
def test_graph_capture_replays_the_same_bits(gpu_device, name, hop, mode):
    """No allocation and no synchronisation at launch: captured on one stream and replayed once,
    the outputs equal the eager run bit for bit."""
    dev = gpu_device
    bank = bank_of(dev, name)
    x, y = xl.pair_of(name)
    xd, yd = strided(dev, x), strided(dev, y)
    eager = launch(xd, yd, bank, hop, mode)
    out = [torch.full_like(e, NAN) for e in eager]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            torch.ops.specenh.filterbank_cross_out(xd, yd, bank.tables, bank.lmax, hop, mode, *out)
    for o in out:
        o.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    for o, e in zip(out, eager):
        assert torch.equal(torch.view_as_real(o) if o.is_complex() else o,
                           torch.view_as_real(e) if e.is_complex() else e)


def test_opcheck(gpu_device):
    from specenh import wavelet as wv

    dev = gpu_device
    bank = wv.FilterBank(wl.random_bank([0, 9, 40], seed=3), nfft=256, device=dev)
    x = torch.from_numpy(np.array(wl.signal("white", 2, 500, seed=9))).to(dev)
    y = torch.from_numpy(np.array(wl.signal("white", 2, 500, seed=10))).to(dev)
    op = torch.ops.specenh.filterbank_cross.default
    op_out = torch.ops.specenh.filterbank_cross_out.default
    for hop, mode in ((3, xl.POINT), (20, xl.MEAN)):
        torch.library.opcheck(op, (x, y, bank.tables, bank.lmax, hop, mode))
        shape = (2, 3, xl.n_out(500, hop, mode))
        sxy = torch.empty(shape, dtype=torch.complex64, device=dev)
        torch.library.opcheck(op_out, (x, y, bank.tables, bank.lmax, hop, mode, sxy,
                                       torch.empty(shape, device=dev),
                                       torch.empty(shape, device=dev)))
        torch.library.opcheck(op_out, (x, y, bank.tables, bank.lmax, hop, mode, sxy, None, None))
