"""Querying a merged file, the parts that need no GPU: wcg.check_merged (the host statement of the
rules wcg_index_merged holds a file to) on hand-written vectors, the ABI entries, and the command
line's *-merged verbs.

The vectors and their expected (line, rule) are written down in tests/merged_vectors.py; nothing
here is computed by the code under test.
"""
import ctypes
import os

import pytest

from tests import merged_vectors as mv
from tests import wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WCG_EINVAL = 1
NEW_CALLS = ("wcg_index_merged", "wcg_load_merged", "wcg_load_merged_device")


@pytest.mark.parametrize("name,data,want", mv.REJECTED, ids=[v[0] for v in mv.REJECTED])
def test_check_merged_rejects(built, name, data, want):
    import wcg
    assert want[1] in wcg.MERGED_KINDS
    assert wcg.check_merged(data) == want


def test_check_merged_newline(built):
    import wcg
    for data, want in mv.NO_NEWLINE:
        assert wcg.check_merged(data) == want, data


def test_check_merged_accepts(built):
    import wcg
    for data in mv.VALID:
        assert wcg.check_merged(data) is None, data
    # what the engine itself writes: every count width, every key length class, a tie group
    counts = dict(wire.edge_count_keys())
    for j in range(50):
        counts[mv.TIE17 + wire.letters(j, 2)] = 1 + j
    assert wcg.check_merged(wire.expect(counts)) is None
    assert wcg.check_merged(open(os.path.join(ROOT, "tests", "golden", "mr-testout.txt"), "rb").read()) is not None  # sorted by count, not by key


def test_check_merged_takes_the_first_bad_line(built):
    import wcg
    good = [b"B: 1", b"a: 5", b"b: 7"]
    assert wcg.check_merged(mv.file_of(good + [b"c: 0", b"d: x"])) == (3, "zero")
    assert wcg.check_merged(mv.file_of(good + [b"c: x", b"d: 0"])) == (3, "count")
    # a key of 2^23 bytes is longer than a record can say
    assert wcg.check_merged(b"k" * ((1 << 23) - 1) + b": 1\n") is None
    assert wcg.check_merged(b"k" * (1 << 23) + b": 1\n") == (0, "count")


def test_new_calls_are_exported(built):
    import wcg
    lib = ctypes.CDLL(wcg._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "wcg.h")).read()
    for name in NEW_CALLS:
        assert name in wcg.EXPORTED and hasattr(lib, name)
        assert "WCG_API int %s(" % name in hdr
    for name in ("index_merged", "load_merged", "load_merged_device"):
        assert callable(getattr(wcg.Engine, name))
    from wcg import distributed, wc
    assert callable(distributed.TorchEngine.load_merged_tensor) and callable(distributed.TorchEngine.index_merged)
    for name in ("top_merged", "count_merged", "prefix_merged"):
        assert callable(getattr(wc, name))


def test_null_context(built):
    import wcg
    lib = wcg.load()
    nl = ctypes.c_uint64(7)
    assert lib.wcg_index_merged(None, ctypes.byref(nl)) == WCG_EINVAL
    assert lib.wcg_load_merged(None, b"a: 1\n", 5, ctypes.byref(nl)) == WCG_EINVAL
    assert lib.wcg_load_merged(None, b"a: 1", 4, ctypes.byref(nl)) == WCG_EINVAL
    assert lib.wcg_load_merged_device(None, None, 0, ctypes.byref(nl)) == WCG_EINVAL
    assert nl.value == 7


def test_cli_verbs(built, monkeypatch, capfdbinary):
    """the *-merged verbs reach their functions with the arguments as bytes / int, and no other
    argv[1] of that shape does (the last branch of main() starts a worker)"""
    from wcg import wc
    calls = []
    monkeypatch.setattr(wc, "top_merged", lambda path, n: calls.append(("top", path, n)) or b"the: 9\n")
    monkeypatch.setattr(wc, "count_merged", lambda path, words: calls.append(("count", path, list(words))) or [3, 0, 5])
    monkeypatch.setattr(wc, "prefix_merged", lambda path, p: calls.append(("prefix", path, p)) or b"ab: 1\nabc: 2\n")

    class NoWorker:
        def __init__(self, *a, **k):
            raise AssertionError("a *-merged verb started a worker")
    monkeypatch.setattr(wc.mr, "Worker", NoWorker)

    assert wc.main(["wc", "top-merged", "mrtmp.x", "10"]) == 0
    assert wc.main(["wc", "count-merged", "mrtmp.x", "a", "zz", "ж"]) == 0
    assert wc.main(["wc", "count-merged", "mrtmp.x", "a"]) == 0
    assert wc.main(["wc", "prefix-merged", "mrtmp.x", "ab"]) == 0
    assert calls == [("top", "mrtmp.x", 10), ("count", "mrtmp.x", [b"a", b"zz", "ж".encode()]),
                     ("count", "mrtmp.x", [b"a"]), ("prefix", "mrtmp.x", b"ab")]
    out = capfdbinary.readouterr().out
    assert out == b"the: 9\n" + b"a: 3\nzz: 0\n" + "ж".encode() + b": 5\n" + b"a: 3\n" + b"ab: 1\nabc: 2\n"
    # too few arguments: wc.go's usage note, nothing run
    calls.clear()
    assert wc.main(["wc", "count-merged", "mrtmp.x"]) == 0
    assert wc.main(["wc", "top-merged", "mrtmp.x"]) == 0
    assert calls == []
    assert b"see usage" in capfdbinary.readouterr().out


def test_gather_merge_index_flag(monkeypatch):
    """distributed.gather_merge(index=True): the root indexes after the merge, and only then, and
    only the root"""
    import types
    from wcg import distributed

    class Rank:
        in_library = True

        def __init__(self):
            self.calls = []
            self.e = types.SimpleNamespace(gather_merge=lambda root: self.calls.append(("gather", root)))

        def index_merged(self):
            self.calls.append("index")
            return 2

        def result(self):
            return b"a: 1\nb: 2\n"

    for rank, index, want_calls, want in [(0, False, [("gather", 0)], b"a: 1\nb: 2\n"),
                                          (0, True, [("gather", 0), "index"], b"a: 1\nb: 2\n"),
                                          (1, True, [("gather", 0)], None)]:
        monkeypatch.setattr(distributed, "dist", types.SimpleNamespace(get_rank=lambda group=None, r=rank: r,
                                                                       get_world_size=lambda group=None: 2))
        eng = Rank()
        assert distributed.gather_merge(eng, root=0, index=index) == want
        assert eng.calls == want_calls
