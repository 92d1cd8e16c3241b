"""bench.py --dump-outputs: what the timed path returned, as float32 .npy files, within the size limit."""
import os

import numpy as np

import bench


def test_dump_outputs_writes_float32_copies(tmp_path):
    acc = np.array([1, 0, 1, 1], dtype=np.uint8)
    st = np.array([0, 16, 0, 0], dtype=np.int32)
    bench.dump_outputs(str(tmp_path), {"accept": acc, "status": st})
    assert sorted(os.listdir(tmp_path)) == ["accept.npy", "status.npy"]
    for name, a in (("accept", acc), ("status", st)):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, a)


def test_dump_outputs_samples_past_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 16 << 10)
    n = 100000
    acc, st = np.arange(n) % 2, np.arange(n)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"accept": acc, "status": st}, "_rank1")
        files = sorted(os.listdir(tmp_path / d))
        assert files == ["accept_rank1.npy", "sample_index_rank1.npy", "status_rank1.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in files) <= bench.DUMP_LIMIT
    idx = np.load(tmp_path / "a" / "sample_index_rank1.npy").astype(np.int64)
    assert len(idx) > 0 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "status_rank1.npy"), st[idx].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "accept_rank1.npy"), acc[idx].astype(np.float32))
    for f in ("sample_index_rank1.npy", "status_rank1.npy"):   # the same sample in every run
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
