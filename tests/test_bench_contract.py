"""bench.py's arithmetic and JSON contract pieces that do not need a GPU."""
import os

import numpy as np

import bench


def test_throughput_counts_every_timed_step():
    # 65536 QPs per rank per step, 3 steps in 2.0 s on 2 ranks
    assert bench.throughput(2, 65536, 3, 2.0) == 2 * 65536 * 3 / 2.0


def _results(rng, sizes, n=7, m=11):
    import impc
    out = []
    for B in sizes:
        info = np.zeros(B, dtype=impc.INFO_DTYPE)
        info["iter"] = rng.integers(1, 4000, B)
        info["obj_val"] = rng.normal(size=B)
        out.append((rng.normal(size=(B, n)), rng.normal(size=(B, m)), info))
    return out


def test_dump_outputs_small_batches_are_kept_whole(tmp_path):
    """--dump-outputs: float64 .npy files per bucket; everything is kept when it fits the budget."""
    import impc
    res = _results(np.random.default_rng(1), (5, 3))
    bench.dump_outputs(str(tmp_path / "d"), res)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(
        f"bucket{i:02d}_{k}.npy" for i in range(2) for k in ("info", "rows", "x", "y"))
    for i, (x, y, info) in enumerate(res):
        got = {k: np.load(tmp_path / "d" / f"bucket{i:02d}_{k}.npy") for k in ("info", "rows", "x", "y")}
        assert all(a.dtype == np.float64 for a in got.values())
        assert np.array_equal(got["rows"], np.arange(x.shape[0]))
        assert np.array_equal(got["x"], x) and np.array_equal(got["y"], y)
        assert got["info"].shape == (x.shape[0], len(impc.INFO_DTYPE.names))
        assert np.array_equal(got["info"][:, 0], info["iter"]) and np.array_equal(got["info"][:, 4], info["obj_val"])


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    """Past the budget x and y are a seeded sample of the QPs -- the same rows on every run, every
    QP's info record still there -- and the files together stay under the budget."""
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 64 << 10)
    res = _results(np.random.default_rng(2), (300, 500))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res)
    total = 0
    for i, (x, y, info) in enumerate(res):
        rows = np.load(tmp_path / "a" / f"bucket{i:02d}_rows.npy").astype(np.int64)
        assert 0 < rows.size < x.shape[0] and np.all(np.diff(rows) > 0)
        assert np.array_equal(np.load(tmp_path / "a" / f"bucket{i:02d}_x.npy"), x[rows])
        assert np.array_equal(np.load(tmp_path / "a" / f"bucket{i:02d}_y.npy"), y[rows])
        assert np.load(tmp_path / "a" / f"bucket{i:02d}_info.npy").shape[0] == x.shape[0]
        for k in ("info", "rows", "x", "y"):
            f = f"bucket{i:02d}_{k}.npy"
            assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
            total += np.load(tmp_path / "a" / f).nbytes
    assert total <= 64 << 10


def test_algorithmic_bytes_survey_values():
    """SURVEY.md 8(d) B_solve figures: N=20 K=0 14,056 B; K=8 22,568 B; K=10 24,696 B; N=40 K=10 50,136 B."""
    def nm(N, K):
        return 13 * N - 5, 21 * N - 5 + K * (N - 1)
    assert bench.algorithmic_bytes(*nm(20, 0), 0, 20) == 14056
    assert bench.algorithmic_bytes(*nm(20, 8), 8, 20) == 22568
    assert bench.algorithmic_bytes(*nm(20, 10), 10, 20) == 24696
    assert bench.algorithmic_bytes(*nm(40, 10), 10, 40) == 50136
