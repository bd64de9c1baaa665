"""bench.py --dump-outputs on the host: the 64 MB limit and its fixed row sample (no GPU needed)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_outputs_are_written_whole(tmp_path):
    arrays = {"rgb_map": torch.rand(3072, 3), "loss": torch.tensor(0.25), "pose_grad": torch.rand(3, 4, dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path), arrays)
    for name, v in arrays.items():
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32
        assert np.array_equal(got.reshape(-1), v.float().numpy().reshape(-1)), name


def test_large_outputs_keep_one_seeded_row_sample_under_the_limit(tmp_path):
    n = 307200
    g = torch.Generator().manual_seed(1)
    rows = torch.arange(n, dtype=torch.float32)
    feat = torch.cat([rows[:, None], torch.rand(n, 63, generator=g)], 1)        # 78.6 MB: over the limit on its own
    arrays = {"feat_map": feat, "rgb_map": rows[:, None].repeat(1, 3), "pose_grad": torch.rand(3, 4, generator=g)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT_BYTES
    fa, ra = np.load(tmp_path / "a" / "feat_map.npy"), np.load(tmp_path / "a" / "rgb_map.npy")
    assert 0 < fa.shape[0] < n and fa.shape[1] == 64
    kept = fa[:, 0]
    assert np.all(np.diff(kept) > 0)                                   # sorted rows of the original, none twice
    assert np.array_equal(ra[:, 0], kept)                              # the same rows in every sampled array
    assert np.array_equal(fa, feat.numpy()[kept.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "pose_grad.npy"), arrays["pose_grad"].numpy())   # small arrays whole
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f        # fixed sample: run to run
