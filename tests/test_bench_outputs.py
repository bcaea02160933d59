"""bench.py --dump-outputs: the writer of the last timed step's arrays (no GPU): float32 .npy files,
whole when they fit the byte budget, else a fixed sample that is the same from run to run."""
import os

import numpy as np

import bench


def test_arrays_within_budget_are_written_whole(tmp_path):
    tokens = np.arange(2 * 256, dtype=np.int32).reshape(2, 256) % 4096
    pcm = np.linspace(-1, 1, 2 * 320 * 256, dtype=np.float32).reshape(2, -1)
    d = str(tmp_path / "out")  # (created by the writer)
    bench.dump_outputs(d, {"tokens": tokens, "pcm": pcm})
    assert sorted(os.listdir(d)) == ["pcm.npy", "tokens.npy"]
    t, p = np.load(os.path.join(d, "tokens.npy")), np.load(os.path.join(d, "pcm.npy"))
    assert t.dtype == np.float32 and p.dtype == np.float32
    assert np.array_equal(t, tokens) and np.array_equal(p, pcm)  # ids < 4096: exact in float32


def test_larger_arrays_are_cut_to_the_same_sample_every_time(tmp_path):
    a = np.random.default_rng(5).standard_normal(10_000).astype(np.float32)
    b = np.arange(100, dtype=np.float64)
    got = []
    for run in ("one", "two"):
        d = str(tmp_path / run)
        bench.dump_outputs(d, {"a": a, "b": b}, budget=2 * 4 * 1000)  # 1,000 elements per array
        got.append(np.load(os.path.join(d, "a.npy")))
        assert np.array_equal(np.load(os.path.join(d, "b.npy")), b.astype(np.float32))  # fits: whole
        assert sum(os.path.getsize(os.path.join(d, f)) - 128 for f in os.listdir(d)) <= 2 * 4 * 1000
    assert got[0].shape == (1000,) and np.array_equal(got[0], got[1])
    idx = np.sort(np.random.default_rng(0).choice(a.size, size=1000, replace=False))
    assert np.array_equal(got[0], a[idx])  # elements of the array itself, in their order
