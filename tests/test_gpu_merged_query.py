"""wcg_index_merged and wcg_load_merged* on the MI355X: a merged file ("key: count\\n" lines in key
order) held by a context after a merge, or loaded from bytes, becomes queryable by wcg_top,
wcg_lookup and wcg_range (csrc/wcg_index.h makes the query records on the device).

Every expected value comes from the host: the dict crafted units were made from and its merged
file (wire.expect), the C oracle's merged file of text (ob.merged), wcg.top_of_merged /
lookup_in_merged / range_of_merged / prefix_succ over those, and wcg.check_merged with the
hand-written (line, rule) pairs of tests/merged_vectors.py for the files that must be refused.
"""
import os
import subprocess
import sys

import pytest

from tests import merged_vectors as mv
from tests import oracle_bridge as ob
from tests import wire

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mit-6.824-2015_amd")
WCG_EINVAL, WCG_ESTATE = 1, 5
BIG = 70_000                                     # a key longer than FM_STAGE (32 768) and NL_BLK (65 536)
FAR = [b"\xff" * 20, b"A", b"\xf4\x8f\xbf\xbf" * 5, b"", b"\0", b"\xff", b"a\0", b"\0a"]


@pytest.fixture
def engine(built):
    import wcg
    made = []

    def make(max_keys=1 << 16):
        e = wcg.Engine(device=0, max_input_bytes=4 << 20, max_keys=max_keys)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


def status_of(call):
    import wcg
    with pytest.raises(wcg.WcgError) as ei:
        call()
    return ei.value.status


def queries_refused(eng):
    return [status_of(lambda: eng.top(10)), status_of(lambda: eng.lookup([b"a"])), status_of(lambda: eng.range()),
            status_of(lambda: eng.prefix(b"a"))] == [WCG_ESTATE] * 4


def bump(k, d):
    return k[:-1] + bytes([k[-1] + d])


def probes(keys):
    out = []
    for k in keys:
        out += [k[:-1], k + b"a", k + b"\0", bump(k, 1), bump(k, -1)]
    return out


def check_all(eng, merged, words, tops=(10,), bounds=(), prefixes=()):
    """every query of the engine against the host statements over `merged`"""
    import wcg
    for n in tops:
        want = wcg.top_of_merged(merged, n)
        ob.assert_same(eng.top(n), want)
        assert eng.top_size(n) == (want.count(b"\n"), len(want))
    words = list(words)
    got, want = eng.lookup(words), wcg.lookup_in_merged(merged, words)
    if got != want:
        bad = [(w[:40], g, x) for w, g, x in zip(words, got, want) if g != x]
        raise AssertionError(f"{len(bad)} of {len(words)} counts differ, first (word, got, want): {bad[0]}")
    ob.assert_same(eng.range(), merged)
    assert eng.range_size() == (merged.count(b"\n"), len(merged))
    for lo, hi in bounds:
        ob.assert_same(eng.range(lo, hi), wcg.range_of_merged(merged, lo, hi))
    for p in prefixes:
        ob.assert_same(eng.prefix(p), wcg.range_of_merged(merged, p, wcg.prefix_succ(p)))


# ---------------------------------------------------------------- 1. round trip on crafted units
EDGE_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 32, 33]


def crafted():
    counts = dict(wire.edge_count_keys())           # every digit edge 9, 10, 99, ... 10^19, 2^32, 2^64 - 1
    counts[b"q"] = 1
    for L in EDGE_LENGTHS:
        for i in (3, 4) if L > 1 else (30, 31):
            counts.setdefault(wire.key_of(i, L), 10 * L + i)
    for j in range(200):                              # a tie group: 17 bytes shared
        counts[mv.TIE17 + wire.letters(j, 2) + wire.filler(j % 30, j)] = 1 + (j * 13) % 977
    counts[b"hugekey" + wire.filler(BIG - 7)] = 424242
    assert {1, 9, 10, 99, 2 ** 32, 10 ** 19, 2 ** 64 - 1} <= set(counts.values())
    assert set(EDGE_LENGTHS) <= {len(k) for k in counts} and max(len(k) for k in counts) == BIG
    return counts


def crafted_checks(counts):
    keys = sorted(counts)
    tie = [k for k in keys if k.startswith(mv.TIE17)]
    assert len(tie) == 200
    words = keys + probes(keys[::7]) + probes(tie[::9]) + FAR + [mv.TIE17, mv.TIE17[:16], keys[5], keys[5]]
    bounds = [(mv.TIE17, mv.TIE17 + b"\xff"), (mv.TIE17[:16], tie[100]), (tie[50][:-1], tie[150] + b"\0"),
              (keys[10], keys[300]), (None, keys[40]), (keys[-3], None), (b"z", b"a"), (b"hugekey", b"hugekez")]
    return words, bounds, [mv.TIE17, mv.TIE17[:16], b"h", b"", b"\xff"]


def test_round_trip(engine):
    """a reduced job's merged file, loaded into a fresh engine, answers as the engine that reduced it"""
    counts = crafted()
    merged = wire.expect(counts)
    red = engine()
    red.reset()
    red.import_host(wire.units(counts, seed=1))
    assert red.reduce()[0] == len(counts)
    ob.assert_same(red.result(), merged)
    eng = engine()
    assert eng.load_merged(merged) == len(counts)
    ob.assert_same(eng.result(), merged)
    words, bounds, prefixes = crafted_checks(counts)
    for e in (eng, red):
        check_all(e, merged, words, tops=(0, 1, 10, 1024), bounds=bounds, prefixes=prefixes)
    for n in (1, 10, 1024):
        assert eng.top(n) == red.top(n)
    assert eng.lookup(words) == red.lookup(words)
    assert eng.index_merged() == len(counts)          # a second call: nothing happens
    check_all(eng, merged, words[:50])


# ---------------------------------------------------------------- 2. line counts, and where the long line sits
def lines_file(n, big):
    keys = wire.ordered_keys(n, 6)
    counts = {k: 1 + (i * 7919) % 100003 for i, k in enumerate(keys)}
    if big == "first":
        counts[b"AAAAA" + wire.filler(BIG - 5)] = 77
    elif big == "middle":
        counts[keys[n // 2] + wire.filler(BIG - 6)] = 77
    elif big == "last":
        counts[b"zzzz" + wire.filler(BIG - 4)] = 77
    return counts


@pytest.mark.parametrize("stage", [None, "0"], ids=["staged", "in-place"])
@pytest.mark.parametrize("n,big", [(1, None), (0, "last"), (1023, None), (1024, None), (1025, None), (1024, "first"),
                                   (1025, "middle"), (1023, "last"), (6000, "first"), (6000, "middle"), (6000, "last")])
def test_line_counts(engine, monkeypatch, n, big, stage):
    """1, 1023, 1024, 1025 and 6000 lines (over 64 KiB: lines straddle NL_BLK blocks and 1024-line
    tiles), the 70 000-byte line first, in the middle and last (its tile is read in place, the
    others through LDS; WCG_INDEX_STAGE=0: every tile in place)"""
    if stage is None:
        monkeypatch.delenv("WCG_INDEX_STAGE", raising=False)
    else:
        monkeypatch.setenv("WCG_INDEX_STAGE", stage)
    counts = lines_file(n, big)
    merged = wire.expect(counts)
    if n == 6000:
        assert len(merged) > 65536 + (BIG if big else 0)
    keys = sorted(counts)
    if big == "first":
        assert len(keys[0]) == BIG
    elif big == "middle":
        assert len(keys[n // 2 + 1]) == BIG
    elif big == "last":
        assert len(keys[-1]) == BIG
    eng = engine()
    assert eng.load_merged(merged) == len(counts)
    ob.assert_same(eng.result(), merged)
    step = max(1, len(keys) // 300)
    words = keys[::step] + keys[-2:] + keys[1020:1030] + probes(keys[::max(1, len(keys) // 40)]) + FAR
    check_all(eng, merged, words, tops=(10, 1024) if n <= 1025 else (10,),
              bounds=[(keys[len(keys) // 3], keys[len(keys) // 2] + b"\0"), (keys[-1], None)], prefixes=[keys[len(keys) // 2][:3]])


def test_empty_file(engine):
    eng = engine()
    assert eng.load_merged(b"") == 0
    assert eng.result() == b""
    assert eng.lookup([b"a", b""]) == [0, 0] and eng.top(10) == b"" and eng.range() == b"" and eng.prefix(b"a") == b""
    assert eng.index_merged() == 0


# ---------------------------------------------------------------- 3. grids
def test_small_grids(engine, monkeypatch):
    """WCG_TOP_GRID=2, WCG_LOOKUP_GRID=1, WCG_LOOKUP_LDS_MIN=1: few workgroups with many steps each,
    and k_lookup's LDS form, over indexed records"""
    monkeypatch.setenv("WCG_TOP_GRID", "2")
    monkeypatch.setenv("WCG_LOOKUP_GRID", "1")
    monkeypatch.setenv("WCG_LOOKUP_LDS_MIN", "1")
    counts = crafted()
    merged = wire.expect(counts)
    eng = engine()
    assert eng.load_merged(merged) == len(counts)
    words, bounds, prefixes = crafted_checks(counts)
    check_all(eng, merged, words * 3, tops=(1, 10, 1024), bounds=bounds, prefixes=prefixes)


# ---------------------------------------------------------------- 4. after a real merge
def corpus(seed):
    from wcg.corpus import Generator, ASCII, UTF8
    a = Generator(ASCII, 8_000, 1.0, seed).bytes(1 << 20)
    u = Generator(UTF8, 3_000, 1.0, seed + 1).bytes(1 << 18)
    tail = (b"\n" + b"longkeylongkeylongkey" * 3 + b" " + "ǅ".encode() * 25 + b" zebra "
            + b"abcdefghijklmnopqrstuvwxyz0abcdefghijklmnopqrstuvwxyzA\n")
    return a + u + tail


@pytest.fixture(scope="module")
def text_job(built):
    """the text, its merged file (the oracle's) and words to ask for: computed once"""
    data = corpus(91)
    merged = ob.merged(data)
    keys = [l.rpartition(b": ")[0] for l in merged.split(b"\n") if l]
    assert 8_000 < len(keys) < 20_000
    return data, merged, keys


def owners(data, W, nreduce=7):
    """W engines after map, exchange and reduce: each holds the sorted run of the keys it owns"""
    import wcg
    from wcg.distributed import line_aligned_ranges
    engines = [wcg.Engine(device=0, max_keys=1 << 16) for _ in range(W)]
    for e, (a, b) in zip(engines, line_aligned_ranges(len(data), W, lambda i: data[i])):
        e.reset()
        e.map_host(data[a:b])
    wcg.exchange_local(engines, nreduce)
    for e in engines:
        e.reduce()
    return engines


def text_words(keys):
    return keys[::17] + probes(keys[::301]) + FAR + [b"zebra", b"zebr", b"longkeylongkeylongkey" * 3]


@pytest.mark.parametrize("W", [1, 2, 3])
def test_after_merge_runs(engine, text_job, W):
    import torch
    import wcg
    data, merged, keys = text_job
    engines = owners(data, W)
    try:
        runs = [e.result() for e in engines]
        tops = [e.top(10) for e in engines]
    finally:
        for e in engines:
            e.close()
    t = torch.frombuffer(bytearray(b"".join(runs)), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    eng = engine()
    assert eng.merge_runs(t.data_ptr(), [len(r) for r in runs]) == (len(keys), len(merged))
    assert queries_refused(eng)                       # without the index nothing has changed
    assert eng.index_merged() == len(keys)
    ob.assert_same(eng.result(), merged)
    check_all(eng, merged, text_words(keys), tops=(10,), bounds=[(keys[100], keys[5000])], prefixes=[b"ze", "ǅ".encode()])
    assert eng.top(10) == wcg.top_merge(tops, 10)
    assert status_of(lambda: eng.partitions(3)) == WCG_ESTATE
    assert status_of(lambda: eng.export_count(3, 2)) == WCG_ESTATE


def test_after_gather_merge_local(text_job):
    import wcg
    data, merged, keys = text_job
    engines = owners(data, 3)
    try:
        tops = [e.top(10) for e in engines]
        root = engines[1]
        assert wcg.gather_merge_local(engines, 1) == (len(keys), len(merged))
        assert queries_refused(root)
        assert root.index_merged() == len(keys)
        ob.assert_same(root.result(), merged)
        check_all(root, merged, text_words(keys), tops=(10,), bounds=[(keys[100], keys[5000])], prefixes=[b"ze"])
        assert root.top(10) == wcg.top_merge(tops, 10)
        assert engines[0].top(10) == tops[0]          # the other ranks still answer for their own keys
    finally:
        for e in engines:
            e.close()


def test_load_merged_tensor(engine, text_job):
    import torch
    from wcg.distributed import TorchEngine
    _, merged, keys = text_job
    t = torch.frombuffer(bytearray(merged), dtype=torch.uint8).to("cuda")
    te = TorchEngine(engine())
    assert te.load_merged_tensor(t) == len(keys)
    check_all(te.e, merged, text_words(keys)[:200])
    assert te.index_merged() == len(keys)
    bad = torch.frombuffer(bytearray(merged[:-1]), dtype=torch.uint8).to("cuda")
    assert status_of(lambda: te.load_merged_tensor(bad)) == WCG_EINVAL


# ---------------------------------------------------------------- 5. state
def test_state(engine, text_job):
    import wcg
    a = {wire.mixed_key(i): 1 + (i * 13) % 977 for i in range(3000)}
    b = {wire.mixed_key(i): 5 + (i * 7) % 501 for i in range(1000, 3500)}
    ma, mb = wire.expect(a), wire.expect(b)
    words = sorted(set(a) | set(b))[::5] + FAR
    eng = engine()
    eng.reset()
    assert status_of(eng.index_merged) == WCG_ESTATE                 # before any result
    eng.import_host(wire.units(a, seed=1))
    assert status_of(eng.index_merged) == WCG_ESTATE
    eng.reduce()
    check_all(eng, ma, words)
    assert eng.index_merged() == len(a)                              # after a plain reduce: nothing to do
    check_all(eng, ma, words)
    assert len(eng.partitions(3)) == 3
    eng.reduce()
    # the same engine loads another file; map_json in between disturbs nothing
    assert eng.load_merged(mb) == len(b)
    check_all(eng, mb, words)
    assert sum(len(p) for p in eng.map_json(b"some words some\n", 3)) > 0
    assert eng.index_merged() == len(b)
    check_all(eng, mb, words, tops=(10, 100))
    assert status_of(lambda: eng.partitions(3)) == WCG_ESTATE        # a merged file has no partitions
    assert status_of(lambda: eng.export_count(3, 2)) == WCG_ESTATE
    check_all(eng, mb, words[:100])
    # the merged file is the records' key storage
    ptr, nb = eng.result_device()
    assert nb == len(mb)
    eng.free(ptr)
    assert queries_refused(eng)
    assert status_of(eng.index_merged) == WCG_ESTATE
    # a new job on the same engine: nothing stale
    eng.reset()
    assert status_of(eng.index_merged) == WCG_ESTATE
    eng.import_host(wire.units(a, seed=2))
    eng.reduce()
    check_all(eng, ma, words, tops=(10, 100))
    # load, then map without a reset: the result (and its index) is dropped
    assert eng.load_merged(mb) == len(b)
    check_all(eng, mb, words[:100])
    eng.map_host(b"fresh words\n")
    assert queries_refused(eng)
    assert status_of(eng.index_merged) == WCG_ESTATE
    # load after load
    assert eng.load_merged(ma) == len(a)
    assert eng.load_merged(mb) == len(b)
    check_all(eng, mb, words[:100])
    # a pending asynchronous job is dropped by a load
    eng.reset()
    eng.import_host(wire.units(a, seed=3))
    eng.reduce_async()
    assert eng.load_merged(mb) == len(b)
    check_all(eng, mb, words[:100])


# ---------------------------------------------------------------- 6. files that must be refused
@pytest.mark.parametrize("name,data,want", mv.REJECTED, ids=[v[0] for v in mv.REJECTED])
def test_rejected(engine, name, data, want):
    import wcg
    assert wcg.check_merged(data) == want
    eng = engine()
    with pytest.raises(wcg.WcgError) as ei:
        eng.load_merged(data)
    assert ei.value.status == WCG_EINVAL
    assert mv.kind_line(str(ei.value)) == want, str(ei.value)
    assert eng.result() == data                        # the merged bytes are still there
    assert queries_refused(eng)
    with pytest.raises(wcg.WcgError) as ei:            # asking again gives the same answer
        eng.index_merged()
    assert ei.value.status == WCG_EINVAL and mv.kind_line(str(ei.value)) == want
    assert eng.load_merged(mv.VALID[3]) == 4           # and the engine is fit for a valid file
    check_all(eng, mv.VALID[3], [b"a", b"ab", b"b", b"B", b"c"])


def test_rejected_far_into_a_file(engine, monkeypatch):
    """the defect in line 2500 of 3000 (another tile than the first), staged and in place"""
    import wcg
    keys = wire.ordered_keys(3000, 6)
    lines = [k + b": %d" % (i + 1) for i, k in enumerate(keys)]
    eng = engine()
    for defect, want in [(keys[2500] + b": 0", (2500, "zero")), (keys[2499] + b": 3", (2500, "order")),
                         (keys[2500][:5] + b"\0: 3", (2500, "nul")), (keys[2500] + b": 03", (2500, "count"))]:
        data = mv.file_of(lines[:2500] + [defect] + lines[2501:])
        assert wcg.check_merged(data) == want
        for stage in (None, "0"):
            if stage is None:
                monkeypatch.delenv("WCG_INDEX_STAGE", raising=False)
            else:
                monkeypatch.setenv("WCG_INDEX_STAGE", stage)
            with pytest.raises(wcg.WcgError) as ei:
                eng.load_merged(data)
            assert ei.value.status == WCG_EINVAL and mv.kind_line(str(ei.value)) == want, (str(ei.value), stage)


def test_valid_files(engine):
    import wcg
    eng = engine()
    for data in mv.VALID:
        assert wcg.check_merged(data) is None
        assert eng.load_merged(data) == data.count(b"\n")
        keys = [l.rpartition(b": ")[0] for l in data.split(b"\n") if l]
        check_all(eng, data, keys + FAR, tops=(1, 10))


def test_missing_newline(engine):
    import wcg
    eng = engine()
    eng.reset()
    eng.import_host(wire.units({b"kept": 3}))
    eng.reduce()
    for data, want in mv.NO_NEWLINE:
        assert wcg.check_merged(data) == want
        with pytest.raises(wcg.WcgError) as ei:
            eng.load_merged(data)
        assert ei.value.status == WCG_EINVAL and "newline" in str(ei.value)
        assert eng.lookup([b"kept"]) == [3]            # checked before anything was touched


def test_refused_after_a_merge(engine):
    """a merge of runs that are not disjoint leaves equal adjacent keys: the index says so"""
    import torch
    import wcg
    runs = [b"a: 1\nb: 2\nd: 4\n", b"b: 5\nc: 3\n"]
    t = torch.frombuffer(bytearray(b"".join(runs)), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    eng = engine()
    eng.merge_runs(t.data_ptr(), [len(r) for r in runs])
    merged = eng.result()
    assert sorted(merged.split(b"\n")[:-1]) == sorted(b"".join(runs).split(b"\n")[:-1])
    with pytest.raises(wcg.WcgError) as ei:
        eng.index_merged()
    assert ei.value.status == WCG_EINVAL and mv.kind_line(str(ei.value)) == wcg.check_merged(merged) == (2, "order")
    assert eng.result() == merged and queries_refused(eng)


# ---------------------------------------------------------------- 7. the command line
def test_cli(built, tmp_path):
    from wcg import wc
    text = (b"the cat and the dog and the bird\ncats catsup cat " + "été ǅ ǅ".encode() + b"\n") * 40 + b"zebra\n"
    path = tmp_path / "small.txt"
    path.write_bytes(text)
    merged = wc.run_single(str(path))
    mrtmp = tmp_path / "mrtmp.small.txt"
    assert mrtmp.read_bytes() == merged == ob.merged(text)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "wcg.wc", *args], env=env, check=True, capture_output=True,
                              timeout=120).stdout
    assert cli("top-merged", str(mrtmp), "5") == wc.top(str(path), 5)
    words = [b"the", b"cat", b"nothing", "ǅ".encode()]
    want = b"".join(w + b": %d\n" % n for w, n in zip(words, wc.count(str(path), words)))
    assert cli("count-merged", str(mrtmp), *[os.fsdecode(w) for w in words]) == want
    assert cli("prefix-merged", str(mrtmp), "cat") == wc.prefix(str(path), b"cat") == b"cat: 80\ncats: 40\ncatsup: 40\n"
