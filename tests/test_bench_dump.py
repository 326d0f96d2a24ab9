"""bench.py --dump-outputs on the host: what it writes, and the seeded sample it keeps of an output above its size limit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_float64_arrays(tmp_path):
    idx = np.array([3, 0, 0xFFFFFFFF], dtype=np.int64)
    cost = np.array([0.5, 1.25, np.inf])
    bench.dump_outputs(str(tmp_path / "out"), {"match_idx": idx, "match_cost": cost})
    assert sorted(os.listdir(tmp_path / "out")) == ["match_cost.npy", "match_idx.npy"]
    got_idx, got_cost = np.load(tmp_path / "out" / "match_idx.npy"), np.load(tmp_path / "out" / "match_cost.npy")
    assert got_idx.dtype == got_cost.dtype == np.float64
    assert np.array_equal(got_idx, idx) and np.array_equal(got_cost, cost)


def test_dump_outputs_samples_the_same_rows_every_run(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3 * 8 * 100)
    n = 1000
    arrays = {"match_idx": np.arange(n) * 2, "match_cost": np.arange(n) * 0.5}
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.size == 100 and np.all(np.diff(rows) > 0) and rows[-1] < n
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "match_idx.npy"), rows * 2)
    assert np.array_equal(np.load(tmp_path / "a" / "match_cost.npy"), rows * 0.5)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 3 * 8 * 100 + 3 * 128          # (+ one .npy header per file)
