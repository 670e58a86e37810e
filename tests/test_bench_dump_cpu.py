"""bench.py --dump-outputs: the writer's dtypes, its 64 MB bound and the fixed sample it takes of larger outputs."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_outputs_are_written_whole(tmp_path):
    x = torch.randn(3, 5)
    d = torch.arange(4, dtype=torch.float64)
    info = bench.dump_outputs(str(tmp_path), {"x": x, "d": d, "h": x.half()})
    assert np.array_equal(np.load(tmp_path / "x.npy"), x.numpy())
    assert np.load(tmp_path / "d.npy").dtype == np.float64
    assert np.load(tmp_path / "h.npy").dtype == np.float32
    assert all(v["sampled"] is None for v in info.values())


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 6 << 20)
    big = torch.arange(3 << 20, dtype=torch.float32)
    small = torch.ones(10)
    info = [bench.dump_outputs(str(tmp_path / f"r{i}"), {"big": big, "small": small}) for i in range(2)]
    a, b = (np.load(tmp_path / f"r{i}" / "big.npy") for i in range(2))
    assert np.array_equal(a, b) and info[0] == info[1]
    assert a.nbytes + 40 <= 6 << 20 and info[0]["big"]["sampled"]["of"] == big.numel()
    assert np.all(np.diff(a) > 0)                          # sorted distinct indices of arange = the sample itself
    assert np.array_equal(np.load(tmp_path / "r0" / "small.npy"), small.numpy())
