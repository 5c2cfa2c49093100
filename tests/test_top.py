"""The host statement of wcg_top (CPU): wcg.top_of_merged against GNU sort itself, wcg.top_merge
against top_of_merged of the whole dict, and the ABI entry.

The reference's acceptance check of word count is `sort -n -k2 mrtmp.kjv12.txt | tail -10`
(src/main/test-wc.sh:2-3).  top_of_merged says the same in Python (a stable sort of the merged
file's lines by count, the last n); here the two are compared on a file no text could produce:
3000 keys of every length class (ASCII and 2-, 3- and 4-byte UTF-8), heavy ties, and counts at the
32- and 64-bit edges, which `sort -n` compares as decimal strings of any length.
"""
import os
import shutil
import subprocess

import pytest

from tests import wire

EDGES = [2 ** 32 - 1, 2 ** 32, 2 ** 63, 10 ** 19, 2 ** 64 - 1]


def mixed_counts(nkeys=3000):
    """ties in bulk (counts 1..40 cycling), each edge count twice (ties at the top), the rest spread"""
    out = {}
    for i in range(nkeys):
        k = wire.mixed_key(i)
        if i % 97 == 5:
            c = EDGES[(i // 97) % len(EDGES)]
        elif i % 3 == 0:
            c = 1 + (i * 7919) % 100000
        else:
            c = 1 + i % 40
        out[k] = c
    assert len(out) == nkeys
    return out


@pytest.fixture(scope="module")
def merged_file(tmp_path_factory):
    counts = mixed_counts()
    merged = wire.expect(counts)
    p = tmp_path_factory.mktemp("top") / "mrtmp.mixed"
    p.write_bytes(merged)
    return counts, merged, str(p)


@pytest.mark.parametrize("n", [0, 1, 10, 64, 1000, 5000])
def test_top_of_merged_is_sort_n_k2_tail(built, merged_file, n):
    import wcg
    if shutil.which("sort") is None or shutil.which("tail") is None:
        pytest.skip("no sort / tail on this machine")
    counts, merged, path = merged_file
    env = dict(os.environ, LC_ALL="C")
    srt = subprocess.run(["sort", "-n", "-k2", path], env=env, check=True, stdout=subprocess.PIPE).stdout
    want = subprocess.run(["tail", "-n", str(n)], input=srt, env=env, check=True, stdout=subprocess.PIPE).stdout
    got = wcg.top_of_merged(merged, n)
    assert got == want
    assert got.count(b"\n") == min(n, len(counts))


def test_top_of_merged_order(built):
    """equal counts keep bytewise key order (a prefix sorts before its extensions); counts compare
    as integers, not as strings"""
    import wcg
    counts = {b"ab": 7, b"a": 7, b"abc": 7, b"b": 10, b"c": 9, b"Z": 2 ** 64 - 1, b"d": 10 ** 19}
    want = b"a: 7\nab: 7\nabc: 7\nc: 9\nb: 10\nd: 10000000000000000000\nZ: 18446744073709551615\n"
    assert wcg.top_of_merged(wire.expect(counts), 100) == want
    assert wcg.top_of_merged(wire.expect(counts), 7) == want
    assert wcg.top_of_merged(wire.expect(counts), 5) == want[len(b"a: 7\nab: 7\n"):]
    assert wcg.top_of_merged(b"", 10) == b""
    assert wcg.top_of_merged(wire.expect(counts), 0) == b""


@pytest.mark.parametrize("W", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 10, 1024])
def test_top_merge(built, W, n):
    """keys split over W owners by ihash % W; every owner's top_of_merged, combined, is the whole
    dict's top.  3000 keys with ties that straddle the owners (counts 1..40 in bulk, the edge counts
    twice each); with W = 8 and n = 1024 every part has fewer than n keys."""
    import wcg
    counts = mixed_counts()
    ihash = wire.wc_ref.ihash
    parts = [{k: c for k, c in counts.items() if ihash(k) % W == p} for p in range(W)]
    assert sum(len(p) for p in parts) == len(counts)
    if W == 8:
        assert all(len(p) < 1024 for p in parts)
    tops = [wcg.top_of_merged(wire.expect(p), n) for p in parts]
    whole = wcg.top_of_merged(wire.expect(counts), n)
    assert wcg.top_merge(tops, n) == whole
    # a tie group cut by n lies across several owners (else the case shows nothing)
    if W > 1 and n >= 10:
        cut = int(whole.split(b"\n")[0].rpartition(b": ")[2])
        owners = {ihash(k) % W for k, c in counts.items() if c == cut}
        assert len(owners) > 1
    # empty parts (a rank that owns nothing) change nothing, wherever they stand
    assert wcg.top_merge([b""] + tops + [b"", b""], n) == whole
    assert wcg.top_merge(tops[::-1], n) == whole


def test_top_merge_small(built):
    import wcg
    assert wcg.top_merge([], 10) == b""
    assert wcg.top_merge([b"", b""], 10) == b""
    assert wcg.top_merge([b"b: 3\n", b"a: 3\nc: 1\n"], 2) == b"a: 3\nb: 3\n"
    assert wcg.top_merge([b"b: 3\n", b"a: 3\nc: 1\n"], 0) == b""


def test_wcg_top_is_exported(built):
    import ctypes
    import wcg
    assert "wcg_top" in wcg.EXPORTED
    lib = ctypes.CDLL(wcg._lib.LIB_PATH)
    assert hasattr(lib, "wcg_top")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wcg.h")).read()
    assert "#define WCG_TOP_MAX %d\n" % wcg.TOP_MAX in hdr
