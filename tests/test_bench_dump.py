"""bench.py --dump-outputs on the host: float32 files, and over the size budget a fixed
seeded sample that is the same elements on every run. CPU only."""
import os

import numpy as np
import pytest
import torch

import bench


def test_dump_keeps_whole_arrays_under_the_budget(tmp_path):
    a = torch.arange(6, dtype=torch.bfloat16).reshape(2, 3)
    bench.dump_outputs(str(tmp_path), [("a", a), ("s", torch.tensor(1.5, dtype=torch.float64))])
    got = np.load(tmp_path / "a.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3) and (got == np.arange(6).reshape(2, 3)).all()
    assert np.load(tmp_path / "s.npy").dtype == np.float32 and float(np.load(tmp_path / "s.npy")) == 1.5


def test_dump_samples_the_same_elements_over_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 4 * 3000)
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    small = torch.ones(7)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), [("big", big), ("small", small)])
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert x.dtype == np.float32 and x.ndim == 1 and 0 < x.size <= 3000
    assert (x == y).all() and (np.diff(x) > 0).all()  # same sorted sample of flat indices
    assert np.load(tmp_path / "x" / "small.npy").shape == (7,)
    total = sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x"))
    assert total <= 4 * 3000 + 4 * 7 + 2 * 128


def test_timing_table_needs_full(monkeypatch, capsys):
    monkeypatch.setattr("sys.argv", ["bench.py", "--timing"])
    with pytest.raises(SystemExit):
        bench.parse()
    assert "--full" in capsys.readouterr().err
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
