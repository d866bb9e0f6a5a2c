"""bench.py's host side without a GPU: the options a plain run and `--full` rest on, and `--dump-outputs`' files (float
arrays, the 64 MB cap, the same sample from run to run)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_dump_outputs_writes_every_array(tmp_path):
    cls = np.arange(3000, dtype=np.float64) % 17
    strand = (np.arange(3000) % 2).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "d"), {"cluster": cls, "strand": strand})
    assert sorted(os.listdir(tmp_path / "d")) == ["cluster.npy", "strand.npy"]
    c, s = np.load(tmp_path / "d" / "cluster.npy"), np.load(tmp_path / "d" / "strand.npy")
    assert c.dtype == np.float64 and s.dtype == np.float32
    assert np.array_equal(c, cls) and np.array_equal(s, strand)


def test_dump_outputs_samples_the_same_entries_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4000)
    cls = np.arange(3000, dtype=np.float64)
    strand = (np.arange(3000) % 2).astype(np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"cluster": cls, "strand": strand})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["cluster.npy", "sample_index.npy", "strand.npy"]
    assert sum(np.load(tmp_path / "a" / f).nbytes for f in files) <= 4000
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    idx = np.load(tmp_path / "a" / "sample_index.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "cluster.npy"), cls[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "strand.npy"), strand[idx])
