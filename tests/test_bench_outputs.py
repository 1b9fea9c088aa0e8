"""``bench.py --dump-outputs DIR``: what the last timed step returned to its caller, written as float32 / float64 ``.npy`` files that two
builds can be compared by, with a fixed, seeded sample in place of arrays past the size limit.  Built from a canned step result
(the shape of ``ParallelFluidEnv.step``'s return) without touching a GPU."""
import os

import numpy as np
import torch

import bench


def _step_result(n=4):
    g = torch.Generator().manual_seed(3)
    obs = {"velocity": torch.randn(n, 2, 8, 16, generator=g), "pressure": torch.randn(n, 8, 16, generator=g, dtype=torch.float64)}
    reward = torch.randn(n, generator=g)
    infos = [{"drag": torch.tensor(0.5 + i), "lift": torch.tensor([i, -i], dtype=torch.float32), "name": "env"} for i in range(n)]
    return obs, reward, [False] * n, [i == n - 1 for i in range(n)], infos


def test_step_arrays_hold_what_the_caller_received():
    obs, reward, term, trunc, infos = _step_result()
    a = bench.step_arrays((obs, reward, term, trunc, infos))
    assert set(a) == {"obs_velocity", "obs_pressure", "reward", "terminated", "truncated", "info_drag", "info_lift"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert a["obs_pressure"].dtype == np.float64 and a["obs_velocity"].dtype == np.float32
    assert np.array_equal(a["obs_velocity"], obs["velocity"].numpy()) and np.array_equal(a["obs_pressure"], obs["pressure"].numpy())
    assert np.array_equal(a["reward"], reward.numpy())
    assert a["terminated"].tolist() == [0, 0, 0, 0] and a["truncated"].tolist() == [0, 0, 0, 1]
    assert a["info_drag"].tolist() == [0.5, 1.5, 2.5, 3.5] and a["info_lift"].shape == (4, 2)


def test_outputs_are_written_whole_below_the_limit(tmp_path):
    arrays = bench.step_arrays(_step_result())
    bench.write_outputs(str(tmp_path / "out"), arrays)
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == sorted(k + ".npy" for k in arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "out" / (k + ".npy"))
        assert got.dtype == v.dtype and np.array_equal(got, v)


def test_outputs_past_the_limit_are_a_fixed_seeded_sample(tmp_path):
    big = np.arange(100_000, dtype=np.float32).reshape(100, 1000)
    small = np.ones(10, np.float64)
    limit = 40_000
    for d in ("a", "b"):
        bench.write_outputs(str(tmp_path / d), {"big": big, "small": small}, limit=limit)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    sample, idx = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big_index.npy")
    assert sample.dtype == np.float32 and idx.dtype == np.float64 and sample.size == idx.size > 1000
    assert np.array_equal(sample, big.reshape(-1)[idx.astype(np.int64)])
    assert np.all(np.diff(idx) > 0)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < limit + 3 * 128
    assert np.array_equal(np.load(tmp_path / "b" / "big_index.npy"), idx)       # the same sample every run
