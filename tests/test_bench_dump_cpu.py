"""bench.py --dump-outputs: arrays are written as float32 .npy; an array above bench.DUMP_SAMPLE
elements is written as a sample whose positions depend only on its name and size, so two builds
of the library can be compared output for output.  --full is off by default."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_is_float32_and_samples_the_same_positions(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 64)
    small = torch.arange(12, dtype=torch.bfloat16).reshape(3, 4)
    big = torch.arange(1000, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big, "count": torch.tensor(7)})
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("small", "big", "count")}
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.array_equal(a["small"], np.arange(12, dtype=np.float32))      # whole, flattened
    assert a["count"].tolist() == [7.0]
    assert a["big"].shape == (64,) and np.all(np.diff(a["big"]) >= 0) and len(set(a["big"])) > 32
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))
    # the positions come from the name and size alone, not from the values
    bench.dump_outputs(str(tmp_path / "c"), {"big": big * 2})
    assert np.array_equal(np.load(tmp_path / "c" / "big.npy"), 2 * a["big"])


def test_full_and_dump_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
