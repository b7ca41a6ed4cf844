"""bench.py --dump-outputs on CPU tensors: the file holds the step's reconstructions in
shot order as float32, a larger batch is cut to the same seeded shots in every call, and the
default cap keeps a dump under 64 MB."""
import numpy as np
import torch

import bench


def _step_output(n, streams):
    """What bench's step() returns: fp16 [n, 128, 128, 1], whole or as per-stream slices."""
    g = torch.Generator().manual_seed(n)
    y = torch.rand((n, bench.HW5, bench.HW5, 1), generator=g).to(torch.float16)
    return y, (y if streams == 1 else list(y.chunk(streams)))


def test_dump_small_batch_is_every_shot_in_order(tmp_path):
    y, outs = _step_output(6, streams=2)
    bench.dump_outputs(str(tmp_path / "d"), outs)
    got = np.load(tmp_path / "d" / "reconstructions.npy")
    assert got.dtype == np.float32 and got.shape == (6, bench.HW5, bench.HW5, 1)
    assert np.array_equal(got, y.float().numpy())


def test_dump_large_batch_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_SHOTS", 5)
    y, outs = _step_output(12, streams=3)
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), y, rank=1)
    a = np.load(tmp_path / "a" / "reconstructions.npy")
    b = np.load(tmp_path / "b" / "reconstructions_rank1.npy")
    assert a.shape == (5, bench.HW5, bench.HW5, 1) and np.array_equal(a, b)
    ref = y.float().numpy()
    rows = [int(np.flatnonzero((ref == s).all(axis=(1, 2, 3)))[0]) for s in a]
    assert rows == sorted(set(rows))  # distinct shots of the batch, in shot order


def test_default_cap_is_under_64_mb():
    assert bench.DUMP_MAX_SHOTS * bench.HW5 * bench.HW5 * 4 <= 64e6
