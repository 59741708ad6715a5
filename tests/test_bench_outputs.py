"""bench.py --dump-outputs / --full: the command line and the dump format (CPU only).

dump_outputs writes every array of the last timed step as DIR/<name>.npy in float64: whole up
to DUMP_WHOLE_BYTES, else a seeded sample of DUMP_SAMPLE_ELEMS elements that is the same in
every run, so two builds can be compared output for output."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_has_no_extra_legs(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "d"


def test_dump_whole_and_sampled(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 8 * 1000)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_ELEMS", 256)
    small = torch.arange(600, dtype=torch.float64).reshape(20, 30)
    small[3, 4] = float("nan")
    status = torch.arange(20, dtype=torch.int32)
    big = torch.arange(5000, dtype=torch.float64).reshape(50, 100) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "status": status, "big": big})
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("small", "status", "big")}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in ("small", "status", "big")}
    assert all(v.dtype == np.float64 for v in a.values())
    # the NaN sits in small_nonfinite.npy (code 1) and is 0 in small.npy: every file is finite
    code = np.load(tmp_path / "a" / "small_nonfinite.npy")
    assert code.dtype == np.float32 and code[3, 4] == 1 and code.sum() == 1
    assert np.isfinite(a["small"]).all() and a["small"][3, 4] == 0 and a["small"].shape == (20, 30)
    assert np.array_equal(np.where(code == 1, np.nan, a["small"]), small.numpy(), equal_nan=True)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy", "small_nonfinite.npy", "status.npy"]
    assert np.array_equal(a["status"], np.arange(20.0))
    # the sample: DUMP_SAMPLE_ELEMS elements of the array at increasing flat indices, the same twice
    assert a["big"].shape == (256,) and np.array_equal(a["big"], b["big"])
    assert np.all(np.diff(a["big"]) >= 0) and np.all(np.isin(a["big"], big.numpy().ravel()))
    assert len(np.unique(a["big"])) > 200
