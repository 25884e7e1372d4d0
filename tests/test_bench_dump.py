"""bench.py --dump-outputs, the writer (no GPU): float32 / float64 files only, at most 64 MB in all, the frames of a fixed sample
of envs when those of the whole batch would not fit."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _sim(n, frame):
    """a batch after step + reset_done (its own game_over codes cleared) and the results-ring row the step wrote"""
    import torch
    g = torch.Generator().manual_seed(n)
    row = torch.stack([torch.rand(n, generator=g), torch.randint(0, 3, (n,), generator=g).float()], dim=1)
    sim = types.SimpleNamespace(num_envs=n, reward=torch.zeros(n), game_over_codes=torch.zeros(n, dtype=torch.uint8),
                                actions=torch.randint(0, 5, (n,), dtype=torch.int32, generator=g),
                                obs=torch.randint(0, 256, (n,) + frame, dtype=torch.uint8, generator=g))
    return sim, row


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_whole_batch_when_it_fits(tmp_path):
    from bench_lib.dump import write_outputs
    sim, row = _sim(64, (3, 12, 12))
    shapes = write_outputs(sim, row, str(tmp_path))
    got = _read(str(tmp_path))
    assert set(got) == {"reward", "game_over", "actions", "obs", "obs_envs"} and {k: list(v.shape) for k, v in got.items()} == shapes
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["obs"], sim.obs.numpy().astype(np.float32)) and np.array_equal(got["obs_envs"], np.arange(64))
    assert np.array_equal(got["reward"], row[:, 0].numpy()) and np.array_equal(got["game_over"], row[:, 1].numpy())
    assert got["game_over"].any()                      # the step's codes, not the batch's buffer that reset_done cleared
    assert np.array_equal(got["actions"], sim.actions.numpy())


def test_fixed_sample_under_the_size_limit(tmp_path):
    from bench_lib.dump import write_outputs
    sim, row = _sim(4096, (3, 84, 84))                 # 4096 x 84 672 bytes of float32 frames: over the limit
    write_outputs(sim, row, str(tmp_path / "a"))
    write_outputs(sim, row, str(tmp_path / "b"))
    a, b = _read(str(tmp_path / "a")), _read(str(tmp_path / "b"))
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a"))) <= 64 * 10**6
    envs = a["obs_envs"].astype(np.int64)
    assert 0 < len(envs) < 4096 and np.all(np.diff(envs) > 0)
    assert np.array_equal(a["obs"], sim.obs.numpy()[envs].astype(np.float32))
    assert all(np.array_equal(a[k], b[k]) for k in a)
