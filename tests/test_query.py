"""The host statements of wcg_lookup and wcg_range (CPU): wcg.lookup_in_merged, wcg.range_of_merged
and wcg.prefix_succ against the plain dict the merged file was made from, Python's own bytes order
(sorted(), <=, startswith), and the ABI entries.

The keys are crafted: prefixes of one another, multi-byte UTF-8, every length class of the record
layout; the bounds and the words asked for also hold NUL and 0xFF bytes, which no key holds.
"""
import ctypes
import os

import pytest

from tests import wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def crafted():
    counts = {b"a": 3, b"ab": 7, b"abc": 2 ** 64 - 1, b"abd": 1, b"b": 10, b"Z": 5,
              "ж".encode(): 4, "жж".encode(): 6, "жз".encode(): 9, "中".encode(): 8, "𝒳".encode(): 2,
              "é".encode(): 11, "éa".encode(): 12}
    for i in range(300):
        counts[wire.mixed_key(i)] = 1 + (i * 7) % 50
    return counts


PROBES = [b"", b"\0", b"a\0", b"ab\0", b"ab\xff", b"\xff", b"\xff" * 20, b"a b", b"abc: 1", b"A", b"zzzz",
          "ж".encode()[:1], "жж".encode()[:3], "中".encode() + b"\0"]

BOUNDS = [None, b"", b"\0", b"a", b"ab", b"ab\0", b"abc", b"abd", b"abe", b"b", b"Z", b"a\xff", b"\xff", b"\xff\xff",
          "ж".encode(), "ж".encode()[:1], "жз".encode(), "中".encode(), "é".encode() + b"\0", wire.mixed_key(7),
          wire.mixed_key(7)[:-1], wire.mixed_key(150) + b"A"]


def test_lookup_in_merged(built):
    import wcg
    counts = crafted()
    merged = wire.expect(counts)
    words = sorted(counts) + PROBES + [k[:-1] for k in counts] + [k + b"a" for k in counts] + [b"ab", b"ab"]
    assert wcg.lookup_in_merged(merged, words) == [counts.get(w, 0) for w in words]
    assert wcg.lookup_in_merged(merged, []) == []
    assert wcg.lookup_in_merged(b"", [b"a", b""]) == [0, 0]
    assert wcg.lookup_in_merged(merged, [b"abc"]) == [2 ** 64 - 1]


@pytest.mark.parametrize("lo", BOUNDS, ids=repr)
def test_range_of_merged(built, lo):
    import wcg
    counts = crafted()
    merged = wire.expect(counts)
    for hi in BOUNDS:
        keys = [k for k in sorted(counts) if (lo is None or lo <= k) and (hi is None or k < hi)]
        want = b"".join(k + b": %d\n" % counts[k] for k in keys)
        assert wcg.range_of_merged(merged, lo, hi) == want, (lo, hi)
        if lo is not None and hi is not None and lo >= hi:
            assert want == b""
    assert wcg.range_of_merged(merged, None, None) == merged
    assert wcg.range_of_merged(b"", lo, None) == b""


def test_range_of_merged_order(built):
    """a prefix sorts before its extensions, an upper bound is exclusive, a lower bound inclusive"""
    import wcg
    merged = wire.expect({b"a": 1, b"ab": 2, b"abc": 3, b"b": 4})
    assert wcg.range_of_merged(merged, b"a", b"ab") == b"a: 1\n"
    assert wcg.range_of_merged(merged, b"ab", b"b") == b"ab: 2\nabc: 3\n"
    assert wcg.range_of_merged(merged, b"ab\0", b"b") == b"abc: 3\n"
    assert wcg.range_of_merged(merged, b"ab", b"ab") == b""
    assert wcg.range_of_merged(merged, b"b", b"a") == b""
    assert wcg.range_of_merged(merged, b"b", None) == b"b: 4\n"
    assert wcg.range_of_merged(merged, None, b"a") == b""


def test_prefix_succ(built):
    import wcg
    assert wcg.prefix_succ(b"") is None
    assert wcg.prefix_succ(b"\xff") is None and wcg.prefix_succ(b"\xff\xff\xff") is None
    assert wcg.prefix_succ(b"a") == b"b"
    assert wcg.prefix_succ(b"ab") == b"ac"
    assert wcg.prefix_succ(b"a\xff") == b"b" and wcg.prefix_succ(b"a\xff\xff") == b"b"
    assert wcg.prefix_succ(b"\0") == b"\x01"
    assert wcg.prefix_succ(b"a\xfe") == b"a\xff"
    assert wcg.prefix_succ("ж".encode()) == b"\xd0\xb7"
    # range(p, succ(p)) is exactly "starts with p"
    counts = crafted()
    merged = wire.expect(counts)
    for p in [b"", b"a", b"ab", b"abc", b"abcd", b"\xd0", "ж".encode(), "жж".encode(), b"\xff", b"a\xff", b"\0",
              wire.mixed_key(12)[:2], wire.mixed_key(13)]:
        want = b"".join(k + b": %d\n" % counts[k] for k in sorted(counts) if k.startswith(p))
        assert wcg.range_of_merged(merged, p, wcg.prefix_succ(p)) == want, p
    assert wcg.range_of_merged(merged, b"ab", wcg.prefix_succ(b"ab")).count(b"\n") == 3


def test_query_calls_are_exported(built):
    import wcg
    lib = ctypes.CDLL(wcg._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "wcg.h")).read()
    for name in ("wcg_lookup", "wcg_lookup_device", "wcg_range"):
        assert name in wcg.EXPORTED and hasattr(lib, name)
        assert "WCG_API int %s(" % name in hdr
    for name in ("lookup", "lookup_device", "range", "range_size", "prefix"):
        assert callable(getattr(wcg.Engine, name))
