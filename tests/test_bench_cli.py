"""bench.py's command line on the CPU (no GPU call is made): --full is off by default, and
--dump-outputs' files hold the merged file as float32, within the 64 MB cap, the same from run to run."""
import os

import numpy as np

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    return bench.parse()


def test_full_and_dump_outputs_are_options(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "2")
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (3, 2)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_outputs_whole_file(tmp_path):
    merged = b"a: 1\nbb: 22\n" + "ǆ: 3\n".encode()
    d = tmp_path / "new" / "dir"
    bench.dump_outputs(str(d), merged)
    assert sorted(os.listdir(d)) == ["merged.npy", "merged_size.npy"]
    m, s = np.load(d / "merged.npy"), np.load(d / "merged_size.npy")
    assert m.dtype == np.float32 and m.astype(np.uint8).tobytes() == merged
    assert s.dtype == np.float64 and s.tolist() == [len(merged), 3]


def test_dump_outputs_sample_under_the_cap(tmp_path, monkeypatch):
    assert bench.DUMP_CAP_BYTES == 64 << 20
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 1 << 16)
    merged = bytes(range(251)) * 1200                        # 4.6 times the cap, as float32 18 times
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), merged)
    a, b = np.load(tmp_path / "a" / "merged.npy"), np.load(tmp_path / "b" / "merged.npy")
    assert a.dtype == np.float32 and np.array_equal(a, b) and a.size > 10_000
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 1 << 16
    assert np.load(tmp_path / "a" / "merged_size.npy").tolist() == [len(merged), merged.count(b"\n")]
