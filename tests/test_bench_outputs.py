"""bench.py --dump-outputs: the last timed answer as float64 .npy files, whole
below the size budget, a seeded (run-to-run identical) row sample above it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _answer(nq, k, seed=3):
    rng = np.random.default_rng(seed)
    return np.sort(rng.random((nq, k)), axis=1), rng.integers(1, 10_000_001, (nq, k)).astype(np.uint32)


def test_dump_outputs_writes_the_answer_as_float64(tmp_path):
    import bench
    d, a = _answer(37, 10)
    out = tmp_path / "dump" / "nested"
    bench.dump_outputs(str(out), d, a)
    assert sorted(os.listdir(out)) == ["anns.npy", "dists.npy"]
    gd, ga = np.load(out / "dists.npy"), np.load(out / "anns.npy")
    assert gd.dtype == np.float64 and ga.dtype == np.float64
    assert np.array_equal(gd, d) and np.array_equal(ga, a.astype(np.float64))
    assert np.array_equal(ga.astype(np.uint32), a)  # ids survive the float64 round trip


def test_dump_outputs_samples_rows_above_the_budget(tmp_path, monkeypatch):
    import bench
    d, a = _answer(101, 7)
    monkeypatch.setattr(bench, "DUMP_BYTES", 20 * (2 * 7 * 8 + 8))  # room for 20 rows
    for name in ("one", "two"):
        bench.dump_outputs(str(tmp_path / name), d, a)
    rows = np.load(tmp_path / "one" / "rows.npy")
    assert rows.dtype == np.float64 and rows.shape == (20,)
    idx = rows.astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 101
    total = 0
    for f in ("dists", "anns", "rows"):
        one, two = np.load(tmp_path / "one" / f"{f}.npy"), np.load(tmp_path / "two" / f"{f}.npy")
        assert np.array_equal(one, two)  # the same sample every run
        total += one.nbytes
    assert total <= bench.DUMP_BYTES
    assert np.array_equal(np.load(tmp_path / "one" / "dists.npy"), d[idx])
    assert np.array_equal(np.load(tmp_path / "one" / "anns.npy"), a[idx].astype(np.float64))
