"""bench.py --dump-outputs (dump_outputs): the frame of the last timed step
as radiance.npy / sample_count.npy, a frame over the byte budget as a fixed
seeded pixel sample; and the plain / --full split of the argument parser.
CPU only: nothing here touches a GPU."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _frame(h, w):
    rng = np.random.default_rng(7)
    return rng.random((h, w, 3), dtype=np.float32), rng.integers(1, 1 << 31, (h, w), dtype=np.uint32)


def test_whole_frame_is_written(tmp_path):
    acc, cnt = _frame(5, 7)
    bench.dump_outputs(str(tmp_path / "out"), acc, cnt)
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["radiance.npy", "sample_count.npy"]
    a = np.load(tmp_path / "out" / "radiance.npy")
    c = np.load(tmp_path / "out" / "sample_count.npy")
    assert a.dtype == np.float32 and c.dtype == np.float64
    assert np.array_equal(a, acc) and np.array_equal(c, cnt.astype(np.float64))


def test_large_frame_is_a_fixed_sample(tmp_path, monkeypatch):
    acc, cnt = _frame(40, 50)
    budget = 28 * 300
    monkeypatch.setattr(bench, "DUMP_BYTES", budget)
    out = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), acc, cnt)
        out.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    assert sorted(out[0]) == ["pixel_index.npy", "radiance.npy", "sample_count.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in out[0]) <= budget  # the files, headers included
    pix = out[0]["pixel_index.npy"].astype(np.int64)
    assert len(pix) == (budget - 3 * bench.NPY_HEADER_BYTES) // 28 and len(np.unique(pix)) == len(pix)
    assert np.array_equal(out[0]["radiance.npy"], acc.reshape(-1, 3)[pix])
    assert np.array_equal(out[0]["sample_count.npy"], cnt.reshape(-1)[pix].astype(np.float64))
    assert all(np.array_equal(out[0][k], out[1][k]) for k in out[0])  # the same pixels every run
    # a whole-frame dump into a directory that held a sample leaves no stale index
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 * 10**6)
    bench.dump_outputs(str(tmp_path / "a"), acc, cnt)
    assert sorted(os.listdir(tmp_path / "a")) == ["radiance.npy", "sample_count.npy"]


def test_parser_has_full_and_dump_outputs():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
