"""wcg_lookup and wcg_range on the MI355X: counts of words and key ranges of the merged file, found
by binary search over the sorted records on the device (csrc/wcg_query.h).

Every expected value comes from the host: the plain dict the crafted units were made from and its
merged file (wire.expect) for crafted jobs, the C oracle's merged file (ob.merged) for text, and
wcg.lookup_in_merged / wcg.range_of_merged over those (tests/test_query.py checks them against
Python's own bytes order).  Crafted units (tests/wire.py through Engine.import_host) make counts
free u64 values and keys any letters; a job of a few thousand units costs milliseconds.

Reduce paths as in tests/test_gpu_top.py: a job behind an empty job takes the multi-launch reduce,
a job behind a 2000-key warm-up the one-launch reduce; reduce_path() is asserted.
"""
import os
import random
import re
import subprocess
import sys

import pytest

from tests import oracle_bridge as ob
from tests import wire

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "mit-6.824-2015_amd")
CSRC = os.path.join(PKG, "csrc")


def _const(header, name):
    m = re.search(r"\b%s = (\d+)\b" % name, open(os.path.join(CSRC, header)).read())
    assert m, (header, name)
    return int(m.group(1))


T = _const("wcg_query.h", "LK_TILE")            # queries per workgroup step
LK_S = _const("wcg_query.h", "LK_S")            # splitters the LDS form of k_lookup stages
LK_LDS_MIN = _const("wcg_query.h", "LK_LDS_MIN")   # the batch size from which it is used

MULTI, FUSED = 0, 1
PATHS = [pytest.param(MULTI, id="multi-launch"), pytest.param(FUSED, id="one-launch")]
WARM = dict(zip(wire.ordered_keys(2000, 12, first=52 ** 3), range(1, 2001)))
WCG_EINVAL, WCG_ESTATE = 1, 5


@pytest.fixture
def engine(built):
    import wcg
    made = []

    def make(max_keys=1 << 17):
        e = wcg.Engine(device=0, max_input_bytes=4 << 20, max_keys=max_keys)
        made.append(e)
        return e
    yield make
    for e in made:
        e.close()


@pytest.fixture(params=[pytest.param(str(1 << 62), id="plain"), pytest.param("1", id="lds")])
def variant(request, monkeypatch):
    """k_lookup's two forms, each on every batch: WCG_LOOKUP_LDS_MIN is the batch size from which a
    workgroup stages the splitters in LDS (unset: LK_LDS_MIN, test_default_threshold)"""
    monkeypatch.setenv("WCG_LOOKUP_LDS_MIN", request.param)
    return request.param


def prepare(eng, path):
    """the job before: a 2000-key one (the next reduce is the one-launch one) or an empty one"""
    eng.reset()
    if path == FUSED:
        eng.map_host(b"\n".join(k for k, c in WARM.items() for _ in range(1 + c % 3)) + b"\n")
        assert eng.reduce()[0] == len(WARM)
    else:
        assert eng.reduce() == (0, 0)


def job(eng, counts, path, reduce=True):
    """the dict's units into cleared tables and (unless reduce=False) the reduce; its merged file"""
    prepare(eng, path)
    eng.reset()
    eng.import_host(wire.units(counts, seed=1))
    if reduce:
        nk, _ = eng.reduce()
        assert nk == len(counts)
        if counts:
            assert eng.reduce_path() == path
    return wire.expect(counts)


def status_of(call):
    import wcg
    with pytest.raises(wcg.WcgError) as ei:
        call()
    return ei.value.status


def bump(k, d):
    return k[:-1] + bytes([k[-1] + d])


def absent_probes(k):
    """byte strings next to the key k: shorter, longer, with a NUL, the last byte one off"""
    return [k[:-1], k + b"a", k + b"Z", k + b"\0", bump(k, 1), bump(k, -1)]


# above every key, at or below every key, and bytes no key holds
FAR = [b"\xff" * 20, b"A", b"\xf4\x8f\xbf\xbf" * 5, b"", b"\0", b"\xff"]


def check_lookup(eng, counts, words):
    """Engine.lookup of the words, in their order, against the dict"""
    words = list(words)
    got = eng.lookup(words)
    want = [counts.get(w, 0) for w in words]
    if got != want:
        bad = [(w, g, x) for w, g, x in zip(words, got, want) if g != x]
        raise AssertionError(f"{len(bad)} of {len(words)} counts differ, first (word, got, want): {bad[0]}")


def check_range(eng, merged, lo, hi):
    import wcg
    want = wcg.range_of_merged(merged, lo, hi)
    got = eng.range(lo, hi)
    ob.assert_same(got, want)
    assert eng.range_size(lo, hi) == (want.count(b"\n"), len(want)), (lo, hi)
    assert eng.range(lo, hi) == got, (lo, hi)                 # the cached lines


def check_prefix(eng, merged, p):
    import wcg
    want = b"".join(line + b"\n" for line in merged.split(b"\n") if line and line.rpartition(b": ")[0].startswith(p))
    assert wcg.range_of_merged(merged, p, wcg.prefix_succ(p)) == want
    ob.assert_same(eng.prefix(p), want)
    return want


# ---------------------------------------------------------------- 1. edges
EDGE_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 32, 33, 60]


@pytest.mark.parametrize("path", PATHS)
def test_edges(engine, variant, path):
    eng = engine()
    prepare(eng, path)
    eng.reset()
    assert eng.reduce() == (0, 0)                       # an empty job
    assert eng.lookup([b"a", b"", b"\xff" * 20, wire.key_of(1, 40)]) == [0, 0, 0, 0]
    assert eng.lookup([]) == []
    assert eng.range() == b"" and eng.range_size() == (0, 0) and eng.range(b"a", b"b") == b"" and eng.prefix(b"") == b""
    one = {b"word": 2 ** 64 - 1}
    merged = job(eng, one, path)
    assert eng.lookup([b"word"]) == [2 ** 64 - 1]
    check_lookup(eng, one, [b"word", b"wor", b"words", b"word\0", b"", b"worc", b"wore"] + FAR)
    assert eng.range() == merged == b"word: 18446744073709551615\n"
    assert eng.lookup([]) == [] and eng.lookup([b""]) == [0]
    # present keys of the lengths at which the record layout changes, two of each, and their neighbours
    counts = {}
    for L in EDGE_LENGTHS:
        for i in (3, 4) if L > 1 else (30, 31):
            counts[wire.key_of(i, L)] = 10 * L + i
    assert sorted({len(k) for k in counts}) == EDGE_LENGTHS
    merged = job(eng, counts, path)
    words = list(counts)
    for k in counts:
        words += absent_probes(k)
    words += [wire.key_of(5, L) for L in EDGE_LENGTHS] + FAR
    check_lookup(eng, counts, words)
    check_lookup(eng, counts, [])
    check_range(eng, merged, None, None)


# ---------------------------------------------------------------- 2. record counts at the search's boundaries
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("nrec", [1, 2, 3, 1023, 1024, 1025, LK_S - 1, LK_S, LK_S + 1])
def test_record_counts(engine, variant, path, nrec):
    """every key, and next to each one a key that sorts directly behind it and one directly before;
    with fewer records than splitters (LK_S + 1 and below) several splitters name one record"""
    keys = wire.ordered_keys(nrec, 6)
    counts = {k: 1 + i for i, k in enumerate(keys)}
    eng = engine()
    merged = job(eng, counts, path)
    words = keys + [k + b"\0" for k in keys] + [bump(k, -1) for k in keys] + [k[:-1] for k in keys] + FAR
    check_lookup(eng, counts, words)
    check_range(eng, merged, None, None)
    check_range(eng, merged, keys[0], keys[-1])
    check_range(eng, merged, keys[-1], None)
    check_range(eng, merged, keys[-1] + b"\0", None)


# ---------------------------------------------------------------- 3. the tie group
def tie_keys():
    """tests/test_gpu_top.py's: 200 long keys sharing a 20-byte UTF-8 prefix, of 21..60 bytes, among 2800 others"""
    prefix = "ж".encode() * 10
    keys = set()
    for j in range(200):
        L = 21 + j % 40
        keys.add(prefix + (wire.letters(j // 40, 1) if L == 21 else wire.letters(j, 2) + wire.filler(L - 22, j)))
    assert len(keys) == 200 and {len(k) for k in keys} == set(range(21, 61))
    i = 0
    while len(keys) < 3000:
        keys.add(wire.mixed_key(i))
        i += 1
    return sorted(keys)


TIE_PREFIX = "ж".encode() * 10


@pytest.mark.parametrize("path", PATHS)
def test_tie_group(engine, variant, path):
    keys = tie_keys()
    counts = {k: 1 + (i * 13) % 977 for i, k in enumerate(keys)}
    eng = engine()
    merged = job(eng, counts, path)
    check_lookup(eng, counts, keys)
    tie = [k for k in keys if k.startswith(TIE_PREFIX)]
    assert len(tie) == 200
    words = []
    for k in tie:                                       # they differ from a key only after byte 16
        words += [bump(k, 1), bump(k, -1), k[:-1], k + b"a", k + b"\0"]
    words += [TIE_PREFIX, TIE_PREFIX[:16], TIE_PREFIX[:17], TIE_PREFIX + b"\xff"]
    check_lookup(eng, counts, words)
    # ranges whose bounds fall inside the group
    check_range(eng, merged, TIE_PREFIX, TIE_PREFIX + b"\xff")
    check_range(eng, merged, TIE_PREFIX[:16], tie[100])
    check_range(eng, merged, tie[50][:-1], tie[150] + b"\0")
    assert check_prefix(eng, merged, TIE_PREFIX).count(b"\n") == 200
    assert check_prefix(eng, merged, TIE_PREFIX[:17]).count(b"\n") == 200


# ---------------------------------------------------------------- 4. unsigned 64-bit counts
@pytest.mark.parametrize("path", PATHS)
def test_u64_counts(engine, variant, path):
    counts = wire.edge_count_keys()
    assert 2 ** 64 - 1 in counts.values() and 2 ** 63 in counts.values() and 2 ** 32 in counts.values()
    eng = engine()
    merged = job(eng, counts, path)
    check_lookup(eng, counts, sorted(counts) + FAR)
    check_range(eng, merged, None, None)


# ---------------------------------------------------------------- 5. zero-count records
def test_zero_count_records(built, variant):
    """A two-pass engine logs a record per key and map call; the sort merges a key's records into
    one (the first of the run) and leaves the others with count 0: the searches must land on the
    first, and the ranges must skip the others."""
    import wcg
    rnd = random.Random(6)
    keys = [wire.key_of(i, 3 + i % 13) for i in range(4500)] + [wire.key_of(i, 16 + i % 45) for i in range(500)]
    assert len(set(keys)) == 5000
    toks = [k for i, k in enumerate(keys) for _ in range(1 + i % 7)]
    rnd.shuffle(toks)
    text = b"\n".join(toks) + b"\n"
    counts = {k: 3 * (1 + i % 7) for i, k in enumerate(keys)}
    with wcg.Engine(device=0, max_input_bytes=8 << 20, max_keys=(4 << 20) + 1) as eng:
        eng.reset()
        for _ in range(3):
            eng.map_host(text)
        nk, _ = eng.reduce()
        assert nk == 5000
        assert eng.stats()["emitted"] > nk              # merged duplicates were among the sorted records
        merged = ob.merged(text * 3)
        assert merged == wire.expect(counts)
        check_lookup(eng, counts, keys + [k + b"a" for k in keys[::7]] + [k[:-1] for k in keys[::5]] + FAR)
        ob.assert_same(eng.range(), merged)
        assert eng.range_size()[0] == nk
        assert eng.range_size() == (nk, len(merged))
        check_range(eng, merged, keys[100], keys[4000])
        check_prefix(eng, merged, keys[4700][:2])


# ---------------------------------------------------------------- 6. batch shape
@pytest.mark.parametrize("grid", [2, None], ids=["grid-2", "grid-default"])
@pytest.mark.parametrize("nq", [T - 1, T, T + 1, 20 * T + 37])
def test_batch_shape(engine, monkeypatch, variant, grid, nq):
    """WCG_LOOKUP_GRID=2 and 20 T + 37 queries: workgroup 0 takes tiles 0, 2, .., 20 (the last of 37
    queries), workgroup 1 tiles 1, 3, .., 19.  The answers come back in the order asked."""
    if grid is None:
        monkeypatch.delenv("WCG_LOOKUP_GRID", raising=False)
    else:
        monkeypatch.setenv("WCG_LOOKUP_GRID", str(grid))
    counts = {wire.mixed_key(i): 1 + (i * 13) % 977 for i in range(3000)}
    eng = engine()
    job(eng, counts, FUSED)
    rnd = random.Random(nq)
    present = sorted(counts)
    pool = present + [k + b"q" for k in present[::3]] + [k[:-1] for k in present[::4]] + FAR
    words = [rnd.choice(pool) for _ in range(nq - 3)] + [present[5]] * 3     # repeats of one word, too
    rnd.shuffle(words)
    assert len(words) == nq
    want = [counts.get(w, 0) for w in words]
    assert 0 in want and sum(1 for x in want if x) > nq // 4
    check_lookup(eng, counts, words)


@pytest.mark.parametrize("nq", [LK_LDS_MIN - 1, LK_LDS_MIN])
def test_default_threshold(engine, monkeypatch, nq):
    """no knob set: the largest batch of the plain form and the smallest of the LDS form"""
    monkeypatch.delenv("WCG_LOOKUP_LDS_MIN", raising=False)
    monkeypatch.delenv("WCG_LOOKUP_GRID", raising=False)
    counts = {wire.mixed_key(i): 1 + (i * 13) % 977 for i in range(3000)}
    eng = engine()
    job(eng, counts, FUSED)
    present = sorted(counts)
    pool = present + [k + b"q" for k in present[::3]] + FAR
    words = (pool * (nq // len(pool) + 1))[:nq]
    random.Random(nq).shuffle(words)
    check_lookup(eng, counts, words)


# ---------------------------------------------------------------- 7. ranges
@pytest.mark.parametrize("path", PATHS)
def test_ranges(engine, path):
    keys = tie_keys()
    extra = [b"cat", b"cats", b"catsup", b"cat" + "é".encode()]          # a whole key that has extensions
    counts = {k: 1 + (i * 31) % 8939 for i, k in enumerate(sorted(set(keys + extra)))}
    eng = engine()
    merged = job(eng, counts, path)
    ks = sorted(counts)
    tie = [k for k in ks if k.startswith(TIE_PREFIX)]
    assert eng.range(None, None) == merged and eng.range() == merged
    for lo, hi in [(ks[10], ks[10]), (b"m", b"m"), (ks[20], ks[10]), (b"z", b"a"), (b"", b""), (b"\xff", b"")]:
        assert eng.range(lo, hi) == b"" and eng.range_size(lo, hi) == (0, 0), (lo, hi)
    bounds = [(ks[10], ks[2000]), (ks[0], ks[-1]), (None, ks[1500]), (ks[1500], None),        # present keys
              (ks[10] + b"\0", bump(ks[2000], 1)), (b"B", b"zzzzzz"), (b"", b"\xff"),          # absent keys
              (tie[3][:30], tie[190][:25]), (TIE_PREFIX[:18], None), (None, tie[100][:17]),    # inside the tie group
              (b"cat\0", b"cats\0"), (b"c\0t", b"cat" + "é".encode() + b"\0"), (b"\0", None)]  # a NUL in a bound
    for lo, hi in bounds:
        check_range(eng, merged, lo, hi)
    assert check_prefix(eng, merged, b"c").count(b"\n") >= 4                       # one ASCII letter
    assert check_prefix(eng, merged, b"\xd0").count(b"\n") >= 200                  # a 2-byte lead
    assert check_prefix(eng, merged, b"cat") == b"".join(k + b": %d\n" % counts[k] for k in sorted(extra))
    assert check_prefix(eng, merged, b"\xff") == b""
    assert check_prefix(eng, merged, b"") == merged
    assert check_prefix(eng, merged, ks[-1]).startswith(ks[-1] + b": ")


# ---------------------------------------------------------------- 8. state
def test_state(engine):
    import torch
    import wcg
    eng = engine()
    calls = [lambda: eng.lookup([b"a"]), lambda: eng.range(), lambda: eng.range_size(b"a", b"b"),
             lambda: eng.lookup_device(0, 0, 1, 0)]
    for call in calls:
        assert status_of(call) == WCG_ESTATE                         # before any reduce
    a = {wire.mixed_key(i): 1 + (i * 13) % 977 for i in range(3000)}
    b = {wire.mixed_key(i + 7): 5 + (i * 17) % 1999 for i in range(2500)}
    words = sorted(set(a) | set(b)) + FAR
    job(eng, a, MULTI, reduce=False)
    for call in calls:
        assert status_of(call) == WCG_ESTATE                         # mapped, not reduced
    merged = job(eng, a, FUSED, reduce=False)
    eng.reduce_async()                                               # no wait: lookup waits for the job
    check_lookup(eng, a, words)
    assert eng.reduce_path() == FUSED
    lo, hi = sorted(a)[100], sorted(a)[900]
    check_range(eng, merged, lo, hi)
    parts = eng.partitions(3)                                        # scatters into the other record buffer
    assert sum(len(p) for p in parts) > 0
    check_lookup(eng, a, words)
    check_range(eng, merged, lo, hi)
    blob, per_rank = eng.export_host(64, 4)                          # compacts again: the sorted records stay
    assert sum(per_rank) > 0
    top = eng.top(10)
    assert top == wcg.top_of_merged(merged, 10)
    check_lookup(eng, a, words)
    check_range(eng, merged, lo, hi)
    check_range(eng, merged, None, lo)
    assert eng.top(10) == top and eng.result() == merged and eng.partitions(3) == parts   # and they are undisturbed
    assert eng.stats()["tokens"] >= 0
    # lookup_device: keys, offsets and counts in device memory, asynchronous on the engine's stream
    off, blob = [0], b""
    for w in words:
        blob += w
        off.append(len(blob))
    d_keys = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to("cuda")
    d_off = torch.tensor(off, dtype=torch.int64, device="cuda")
    d_cnt = torch.full((len(words),), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.lookup_device(d_keys.data_ptr(), d_off.data_ptr(), len(words), d_cnt.data_ptr())
    eng.sync()
    assert [x & (2 ** 64 - 1) for x in d_cnt.cpu().tolist()] == [a.get(w, 0) for w in words]
    eng.lookup_device(0, 0, 0, 0)                                    # nq == 0 touches nothing
    # a too-small buffer is an argument error and leaves the job's results alone
    want = wcg.range_of_merged(merged, lo, hi)
    import ctypes
    small = ctypes.create_string_buffer(8)
    nl, nb = ctypes.c_uint64(), ctypes.c_uint64()
    rc = eng._lib.wcg_range(eng._ctx, lo, len(lo), hi, len(hi), small, 8, ctypes.byref(nl), ctypes.byref(nb))
    assert rc == WCG_EINVAL and (nl.value, nb.value) == (want.count(b"\n"), len(want))
    check_range(eng, merged, lo, hi)
    check_lookup(eng, a, words)
    merged_b = job(eng, b, FUSED)                                    # a different job: nothing stale
    assert merged_b != merged
    check_lookup(eng, b, words)
    check_range(eng, merged_b, lo, hi)
    # after wcg_merge_runs the sorted records are lines without counts
    t = torch.frombuffer(bytearray(merged), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    eng.merge_runs(t.data_ptr(), [len(merged)])
    for call in calls:
        assert status_of(call) == WCG_ESTATE
    merged = job(eng, a, MULTI)                                      # and the next reduce works again
    check_lookup(eng, a, words)
    check_range(eng, merged, lo, hi)
    ptr, _ = eng.result_device()
    eng.free(ptr)                                                    # wcg_free of the result
    for call in calls:
        assert status_of(call) == WCG_ESTATE


# ---------------------------------------------------------------- 9. two engines on one device
def test_two_engines(engine):
    e1, e2 = engine(), engine()
    a = {wire.mixed_key(i): 1 + (i * 13) % 977 for i in range(4000)}
    b = {wire.mixed_key(i): 3 + (i * 29) % 499 for i in range(1500, 4100)}
    ma = job(e1, a, MULTI)
    mb = job(e2, b, FUSED)
    words = sorted(set(a) | set(b)) + FAR
    lo, hi = wire.mixed_key(1600), wire.mixed_key(40)
    lo, hi = min(lo, hi), max(lo, hi)
    for _ in range(2):
        check_lookup(e1, a, words)
        check_lookup(e2, b, words)
        check_range(e1, ma, lo, hi)
        check_range(e2, mb, lo, hi)
        check_range(e2, mb, None, lo)
        check_range(e1, ma, hi, None)


# ---------------------------------------------------------------- 10. ranks
def test_ranks(built):
    """W = 3 owners of disjoint keys (exchange_local, then reduce on each): a word's count is the sum
    of the ranks' lookups, a prefix's lines are the ranks' lines merged by key"""
    import wcg
    from wcg.corpus import Generator, ASCII, UTF8
    from wcg.distributed import line_aligned_ranges
    W = 3
    data = Generator(ASCII, 30_000, 1.0, 91).bytes(5 << 19) + Generator(UTF8, 10_000, 1.0, 92).bytes(1 << 19) + b"\n"
    merged = ob.merged(data)
    present = [line.rpartition(b": ")[0] for line in merged.split(b"\n") if line]
    rnd = random.Random(10)
    words = rnd.sample(present, 2000) + [k + b"x" for k in rnd.sample(present, 500)] + FAR
    rnd.shuffle(words)
    engines = [wcg.Engine(device=0, max_keys=1 << 18) for _ in range(W)]
    try:
        for e, (lo, hi) in zip(engines, line_aligned_ranges(len(data), W, lambda i: data[i])):
            e.reset()
            e.map_host(data[lo:hi])
        wcg.exchange_local(engines, 64)
        nkeys = sum(e.reduce()[0] for e in engines)
        assert nkeys == len(present)
        per_rank = [e.lookup(words) for e in engines]
        want = wcg.lookup_in_merged(merged, words)
        assert [sum(col) for col in zip(*per_rank)] == want
        assert all(sum(1 for x in col if x) <= 1 for col in zip(*per_rank))      # one owner per key
        for p in (b"s", b"\xd0", present[len(present) // 2][:3]):
            lines = sorted(line + b"\n" for e in engines for line in e.prefix(p).split(b"\n") if line)
            ob.assert_same(b"".join(lines), wcg.range_of_merged(merged, p, wcg.prefix_succ(p)))
            assert lines or p in (b"s", b"\xd0")
    finally:
        for e in engines:
            e.close()


# ---------------------------------------------------------------- 11. text and the command line
def test_text_and_cli(built, tmp_path):
    from wcg import wc
    import wcg
    from wcg.corpus import Generator, ASCII, UTF8
    data = Generator(ASCII, 50_000, 1.0, 101).bytes(3 << 19) + Generator(UTF8, 20_000, 1.0, 102).bytes(1 << 19) + b"\n"
    path = tmp_path / "input.txt"
    path.write_bytes(data)
    merged = ob.merged(data)
    present = [line.rpartition(b": ")[0] for line in merged.split(b"\n") if line]
    ascii_words = [k for k in present if k.isascii()]
    words = [ascii_words[0], b"nosuchwordatall", ascii_words[len(ascii_words) // 2], present[-1], ascii_words[-1] + b"q",
             ascii_words[0]]
    want_counts = wcg.lookup_in_merged(merged, words)
    assert want_counts[1] == 0 and want_counts[4] == 0 and min(want_counts[0], want_counts[2], want_counts[3]) > 0
    assert wc.count(str(path), words) == want_counts
    p = ascii_words[len(ascii_words) // 3][:2]
    want_lines = wcg.range_of_merged(merged, p, wcg.prefix_succ(p))
    assert want_lines.count(b"\n") >= 1
    ob.assert_same(wc.prefix(str(path), p), want_lines)
    ob.assert_same(wc.prefix(str(path), b"\xd0"), wcg.range_of_merged(merged, b"\xd0", b"\xd1"))
    assert sorted(os.listdir(tmp_path)) == ["input.txt"]         # no mrtmp.* files
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    child = subprocess.run([sys.executable, "-m", "wcg.wc", "count", str(path)] + [os.fsdecode(w) for w in words],
                           env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    assert child.stdout == b"".join(w + b": %d\n" % c for w, c in zip(words, want_counts))   # those bytes and nothing else
    child = subprocess.run([sys.executable, "-m", "wcg.wc", "prefix", str(path), os.fsdecode(p)], env=env,
                           cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    assert child.stdout == want_lines
    assert sorted(os.listdir(tmp_path)) == ["input.txt"]
