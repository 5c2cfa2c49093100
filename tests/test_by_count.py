"""The host statements of wcg_by_count / wcg_count_rank (CPU): wcg.by_count_of_merged against GNU
sort itself, wcg.count_rank_of_merged against a brute-force count, wcg.by_count_merge against
by_count_of_merged of the whole dict, and the ABI entries.

The count order is what `LC_ALL=C sort -n -k2 <merged file>` prints (src/main/test-wc.sh:2-3 without
its tail).  by_count_of_merged says the same in Python (a stable sort of the merged file's lines by
count); here the two are compared on a file no text could produce: 3000 keys of every length class
(ASCII and 2-, 3- and 4-byte UTF-8), heavy ties, and counts at the 32- and 64-bit edges, which
`sort -n` compares as decimal strings of any length.
"""
import ctypes
import os
import shutil
import subprocess

import pytest

from tests import wire

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGES = [2 ** 32 - 1, 2 ** 32, 2 ** 63, 10 ** 19, 2 ** 64 - 1]
NAMES = ["wcg_by_count", "wcg_by_count_device", "wcg_count_rank"]


def mixed_counts(nkeys=3000):
    """ties in bulk (counts 1..40 cycling), each edge count several times, the rest spread"""
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
    assert len(out) == nkeys and set(EDGES) <= set(out.values())
    return out


def windows(K):
    return [(0, 1), (0, 10), (1234, 100), (K - 10, 10), (K - 1, 5), (K, 3), (K + 7, 1), (5, 0)]


@pytest.fixture(scope="module")
def merged_file(tmp_path_factory):
    counts = mixed_counts()
    merged = wire.expect(counts)
    p = tmp_path_factory.mktemp("by_count") / "mrtmp.mixed"
    p.write_bytes(merged)
    return counts, merged, str(p)


def test_by_count_of_merged_is_sort_n_k2(built, merged_file):
    import wcg
    if shutil.which("sort") is None:
        pytest.skip("no sort on this machine")
    counts, merged, path = merged_file
    K = len(counts)
    srt = subprocess.run(["sort", "-n", "-k2", path], env=dict(os.environ, LC_ALL="C"), check=True,
                         stdout=subprocess.PIPE).stdout
    assert wcg.by_count_of_merged(merged) == srt
    assert wcg.by_count_of_merged(merged, 0, None) == srt
    lines = srt.splitlines(keepends=True)
    assert len(lines) == K
    for first, n in windows(K):
        assert wcg.by_count_of_merged(merged, first, n) == b"".join(lines[first:first + n]), (first, n)
    assert wcg.by_count_of_merged(merged, 2990) == b"".join(lines[2990:])
    assert wcg.by_count_of_merged(merged, K - 64, 64) == wcg.top_of_merged(merged, 64)
    assert wcg.by_count_of_merged(b"") == b"" and wcg.by_count_of_merged(b"", 3, 5) == b""


def test_count_rank_of_merged(built, merged_file):
    import wcg
    counts, merged, _ = merged_file
    values = list(counts.values())
    qs = sorted({0, 1, 2 ** 64 - 1} | set(values) | {c + 1 for c in values if c < 2 ** 64 - 1})
    want = [sum(1 for v in values if v < q) for q in qs]
    assert wcg.count_rank_of_merged(merged, qs) == want
    assert wcg.count_rank_of_merged(merged, []) == []
    assert wcg.count_rank_of_merged(b"", [0, 1, 7]) == [0, 0, 0]
    # the keys with count >= c are the ranks [rank(c), K); those with exactly c are [rank(c), rank(c + 1))
    K = len(counts)
    for c in (1, 7, 40, 2 ** 32, 2 ** 63):
        r0, r1 = wcg.count_rank_of_merged(merged, [c, c + 1])
        exact = wcg.by_count_of_merged(merged, r0, r1 - r0)
        assert exact.count(b"\n") == values.count(c)
        assert all(l.endswith(b": %d" % c) for l in exact.splitlines())
        assert wcg.by_count_of_merged(merged, r0).count(b"\n") == K - r0 == sum(1 for v in values if v >= c)


@pytest.mark.parametrize("W", [1, 3, 8])
def test_by_count_merge(built, W):
    """keys split over W owners by ihash % W; the owners' count orders, combined, are the whole dict's"""
    import wcg
    counts = mixed_counts()
    ihash = wire.wc_ref.ihash
    parts = [{k: c for k, c in counts.items() if ihash(k) % W == p} for p in range(W)]
    assert sum(len(p) for p in parts) == len(counts)
    outs = [wcg.by_count_of_merged(wire.expect(p)) for p in parts]
    whole = wcg.by_count_of_merged(wire.expect(counts))
    assert wcg.by_count_merge(outs) == whole
    if W > 1:                                           # a tie group lies across several owners
        assert len({ihash(k) % W for k, c in counts.items() if c == 7}) > 1
    assert wcg.by_count_merge([b""] + outs + [b"", b""]) == whole      # empty parts change nothing
    assert wcg.by_count_merge(outs[::-1]) == whole                     # nor does the parts' order
    assert wcg.by_count_merge([]) == b"" and wcg.by_count_merge([b"", b""]) == b""
    assert wcg.by_count_merge([b"b: 3\n", b"c: 1\na: 3\n"]) == b"c: 1\na: 3\nb: 3\n"


def test_abi(built):
    import wcg
    lib = ctypes.CDLL(wcg._lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "wcg.h")).read()
    for name in NAMES:
        assert name in wcg.EXPORTED
        assert hasattr(lib, name)
        assert "WCG_API int %s(wcg_ctx *ctx" % name in hdr
    for name in ("by_count_of_merged", "count_rank_of_merged", "by_count_merge"):
        assert callable(getattr(wcg, name))
