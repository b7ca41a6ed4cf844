"""The inputs of the localised-error tests of tests/test_stft_complex_gpu.py are fair (no GPU,
numpy and scipy only): a plain emulation of the paired-frame algorithm of csrc/stft_complex.hip
(tests/stft_local.py) stays below 1e-6 under both metrics on every case and in both
directions, a tenth of the 1e-5 the kernels are held to, while the level within a shot spreads
over more than three decades, which is what the normwise metric cannot see."""
import numpy as np
import pytest

import stft_local as sl

EMU_TOL = 1e-6


@pytest.mark.parametrize("reverse", [False, True], ids=["falling", "rising"])
@pytest.mark.parametrize("case", sl.LOCAL, ids=sl.LOCAL_IDS)
def test_emulated_pairs_keep_the_local_bounds(case, reverse):
    Z, Z32, xi = sl.reference(case, reverse)
    L, n, nov, w = case
    # padded=True: the inverse is the signal and the padding, at most one hop more
    assert Z.shape[:2] == (sl.BATCH, n // 2 + 1) and L <= xi.shape[1] < L + n - nov
    fwd = float(sl.frame_error(sl.emulate_forward(case, reverse), Z).max())
    inv = float(sl.sample_error(sl.emulate_inverse(case, reverse), xi, case).max())
    fs, ss = sl.spread(sl.frame_levels(Z)), sl.spread(sl.sample_levels(xi, case))
    print(f"[stft_local] {n}/{nov} {w} {'rising' if reverse else 'falling'}: emulated forward "
          f"{fwd:.2e}, inverse {inv:.2e}; frame levels spread {fs:.1e}, local levels {ss:.1e}")
    assert fwd <= EMU_TOL and inv <= EMU_TOL, (fwd, inv)  # also fails on NaN
    assert fs >= 1e3 and ss >= 1e3, (fs, ss)


def test_metrics_see_an_error_in_a_quiet_frame():
    """An error of 1 % of one quiet frame (or of the samples under it) is below 1e-5 of the
    shot's maximum and far above 1e-5 under the local metrics; an error of 5e-7 of the louder
    frame of a pair, put on either frame of the pair, measures 5e-7."""
    case = sl.LOCAL[2]
    L, n, nov, w = case
    Z, Z32, xi = sl.reference(case, False)
    T = Z.shape[2]
    bad = Z.copy()
    bad[:, :, T - 3] *= 1.01
    assert np.abs(bad - Z).max() / np.abs(Z).max() < 1e-5
    e = sl.frame_error(bad, Z)
    assert e[:, T - 3].min() > 1e-3 and np.delete(e, T - 3, axis=1).max() == 0.0
    pair = Z.copy()
    pair[:, :, 11] += 5e-7 * np.abs(Z[:, :, 10:12]).max(axis=(1, 2))[:, None]
    assert 4e-7 < sl.frame_error(pair, Z).max() <= 1e-6
    xb = xi.copy()
    xb[:, L - 300:L - 200] *= 1.01
    assert np.abs(xb - xi).max() / np.abs(xi).max() < 1e-5
    assert sl.sample_error(xb, xi, case).max() > 1e-3
