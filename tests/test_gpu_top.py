"""wcg_top on the MI355X: the n most frequent words, selected on the device (csrc/wcg_top.h).

Every expected value comes from the host: wcg.top_of_merged (tests/test_top.py checks it against
GNU `sort -n -k2 | tail -n`) over the merged file of the plain-Python reference (wire.expect) for
crafted units, or of the C oracle (ob.merged) for text.  Crafted units (tests/wire.py through
Engine.import_host) make counts free u64 values; a job of a few thousand units costs milliseconds.

Reduce paths as in tests/test_gpu_crafted.py: a job behind an empty job takes the multi-launch
reduce, a job behind a 2000-key warm-up the one-launch reduce; reduce_path() is asserted.
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "mr-testout.txt")


def _const(header, name):
    m = re.search(r"\b%s = (\d+)\b" % name, open(os.path.join(CSRC, header)).read())
    assert m, (header, name)
    return int(m.group(1))


TOP_TILE = _const("wcg_top.h", "TOP_TILE")      # records per workgroup step
TOP_BUF = _const("wcg_top.h", "TOP_BUF")        # candidate items in LDS
TOP_MAX = 1024                                  # WCG_TOP_MAX

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


def check(eng, merged, ns):
    import wcg
    nkeys = merged.count(b"\n")
    for n in ns:
        want = wcg.top_of_merged(merged, n)
        got = eng.top(n)
        ob.assert_same(got, want)
        assert eng.top_size(n) == (min(n, nkeys), len(want)), n      # host_out == NULL agrees with the copy


def status_of(call):
    import wcg
    with pytest.raises(wcg.WcgError) as ei:
        call()
    return ei.value.status


# ---------------------------------------------------------------- 1. edges
@pytest.mark.parametrize("path", PATHS)
def test_edges(engine, path):
    """no key, one key, and n = 0, 1, nkeys, nkeys + 1, 1024 and 1025 around a 300-key job"""
    eng = engine()
    prepare(eng, path)
    eng.reset()
    assert eng.reduce() == (0, 0)                       # an empty job
    assert eng.top(10) == b"" and eng.top_size(10) == (0, 0) and eng.top(0) == b""
    one = {b"word": 2 ** 64 - 1}
    check(eng, job(eng, one, path), [0, 1, 2, 10, 1024])
    assert eng.top(1) == b"word: 18446744073709551615\n"
    counts = {wire.mixed_key(i): 1 + (i * 7) % 50 for i in range(300)}
    merged = job(eng, counts, path)
    check(eng, merged, [0, 1, 300, 301, 1024, 10])
    assert status_of(lambda: eng.top(1025)) == WCG_EINVAL
    assert status_of(lambda: eng.top_size(1 << 31)) == WCG_EINVAL
    check(eng, merged, [10])                            # the error left the job's results alone


# ---------------------------------------------------------------- 2. the reference's vector
@pytest.mark.parametrize("path", PATHS)
def test_reference_vector(engine, path):
    """mr-testout.txt is `sort -n -k2 mrtmp.kjv12.txt | tail -10` (test-wc.sh:2-3).  Its ten words with
    its counts among 5000 filler keys of all length classes with counts below 8940, `The`, `AND`
    and `unt` among them: top(10) is the file, byte for byte (case sensitivity and the format)."""
    want = open(GOLDEN, "rb").read()
    counts = {}
    for line in want.splitlines():
        k, _, c = line.rpartition(b": ")
        counts[k] = int(c)
    assert len(counts) == 10 and min(counts.values()) == 8940
    counts.update({b"The": 8939, b"AND": 8000, b"unt": 8939})
    i = 0
    while len(counts) < 10 + 3 + 5000:
        counts.setdefault(wire.mixed_key(i), 1 + (i * 31) % 8939)
        i += 1
    eng = engine()
    merged = job(eng, counts, path)
    assert eng.top(10) == want
    check(eng, merged, [10, 13])


# ---------------------------------------------------------------- 3. unsigned 64-bit order
@pytest.mark.parametrize("path", PATHS)
def test_u64_order(engine, path):
    """every digit width, 2^32 +- 1, 2^63 (negative as a signed word) and 2^64 - 1"""
    counts = wire.edge_count_keys()
    eng = engine()
    merged = job(eng, counts, path)
    assert len(counts) <= TOP_MAX
    check(eng, merged, [1, 10, len(counts)])
    assert eng.top(1).endswith(b": 18446744073709551615\n")


# ---------------------------------------------------------------- 4. ties
def tie_keys():
    """3000 keys: 200 long keys sharing a 20-byte UTF-8 prefix, of 21..60 bytes (21..32: the table
    slot's cell, 33..60: the arena heap; one tie group of the sort), and 2800 of all length classes"""
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


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("values", [(7,), (5, 7)], ids=["all-7", "5-or-7"])
def test_ties(engine, path, values):
    """equal counts: the last n keys bytewise, which only the index in the sorted records decides"""
    keys = tie_keys()
    counts = {k: values[i % len(values)] for i, k in enumerate(keys)}
    eng = engine()
    merged = job(eng, counts, path)
    check(eng, merged, [10, 64, 1000])
    if values == (7,):
        for n in (10, 64, 1000):
            assert eng.top(n) == b"".join(k + b": 7\n" for k in keys[-n:])


# ---------------------------------------------------------------- 5. adversarial orders
K_ADV = 20 * TOP_TILE + 37
ORDERS = {"ascending": lambda i: 1 + i, "descending": lambda i: K_ADV - i, "equal": lambda i: 7}


@pytest.mark.parametrize("grid", [2, None], ids=["grid-2", "grid-default"])
@pytest.mark.parametrize("order", sorted(ORDERS))
def test_adversarial_orders(engine, monkeypatch, order, grid):
    """K = 20 * TOP_TILE + 37 keys in key order = 21 tiles (the last of 37 records).

    WCG_TOP_GRID=2: workgroup 0 takes tiles 0, 2, .., 20 (10 whole tiles and the short one),
    workgroup 1 tiles 1, 3, .., 19 (10 whole tiles).  A workgroup compacts when its buffer is full
    (TOP_BUF items; a tile's items that found no room wait, and those still above the raised
    threshold go in behind the n kept), and once more at the end.
    Ascending counts and all-equal counts: every item beats the threshold (a larger count; an
    equal count with a larger index), so every whole tile appends TOP_TILE items.
      n = 1024: fill goes 1024 -> 2048 -> compact to 1024 -> 2048 -> ..: a compaction after every
                whole tile from the second, 9 in the loop per workgroup;
      n = 1, 10: 1024 -> 2048 -> compact to n -> n + 1024 -> full with n items waiting -> compact,
                the waiting items that still qualify behind the n kept -> ..: a compaction after
                every second whole tile, 5 in the loop per workgroup, 4 of them with items waiting.
    Descending counts: the first two tiles fill the buffer (no threshold before the first
    compaction), that compaction sets the threshold and nothing beats it afterwards: 1 in the
    loop.  Each workgroup compacts once more at the end.
    Knob unset: 21 workgroups of one tile each, and the final stage selects from 21 * n slots."""
    if grid is None:
        monkeypatch.delenv("WCG_TOP_GRID", raising=False)
    else:
        monkeypatch.setenv("WCG_TOP_GRID", str(grid))
    assert TOP_MAX + TOP_TILE == TOP_BUF                # what the counts above assume
    keys = wire.ordered_keys(K_ADV, 6)
    counts = {k: ORDERS[order](i) for i, k in enumerate(keys)}
    eng = engine()
    merged = job(eng, counts, MULTI)
    check(eng, merged, [1, 10, 1024])


@pytest.mark.parametrize("K", [TOP_TILE - 1, TOP_TILE, TOP_TILE + 1])
def test_tile_edge(engine, K):
    keys = wire.ordered_keys(K, 6)
    counts = {k: 1 + i for i, k in enumerate(keys)}
    eng = engine()
    merged = job(eng, counts, FUSED)
    check(eng, merged, [1, 10, 1024])
    assert eng.top(1) == keys[-1] + b": %d\n" % K


# ---------------------------------------------------------------- 6. zero-count records
def test_zero_count_records(built):
    """A two-pass engine logs a record per key and map call; the sort merges a key's records into
    one and leaves the others with count 0, which the selection must skip."""
    import wcg
    rnd = random.Random(6)
    keys = [wire.key_of(i, 3 + i % 13) for i in range(4500)] + [wire.key_of(i, 16 + i % 45) for i in range(500)]
    assert len(set(keys)) == 5000
    toks = [k for i, k in enumerate(keys) for _ in range(1 + i % 7)]
    rnd.shuffle(toks)
    text = b"\n".join(toks) + b"\n"
    with wcg.Engine(device=0, max_input_bytes=8 << 20, max_keys=(4 << 20) + 1) as eng:
        eng.reset()
        for _ in range(3):
            eng.map_host(text)
        nk, _ = eng.reduce()
        assert nk == 5000
        assert eng.stats()["emitted"] > nk              # merged duplicates were among the sorted records
        check(eng, ob.merged(text * 3), [10, 1024])


# ---------------------------------------------------------------- 7. state
def test_state(engine):
    import torch
    eng = engine()
    assert status_of(lambda: eng.top(10)) == WCG_ESTATE          # before any reduce
    a = {wire.mixed_key(i): 1 + (i * 13) % 977 for i in range(3000)}
    b = {wire.mixed_key(i + 7): 5 + (i * 17) % 1999 for i in range(2500)}
    job(eng, a, MULTI, reduce=False)
    assert status_of(lambda: eng.top(10)) == WCG_ESTATE          # mapped, not reduced
    merged = job(eng, a, FUSED, reduce=False)
    eng.reduce_async()                                           # no wait: top waits for the job
    check(eng, merged, [10])
    assert eng.reduce_path() == FUSED
    check(eng, merged, [10, 100, 10])                            # the cache follows n
    parts = eng.partitions(3)                                    # scatters into the other record buffer
    assert sum(len(p) for p in parts) > 0
    check(eng, merged, [10, 100])
    blob, per_rank = eng.export_host(64, 4)                      # compacts again: the sorted records stay
    assert sum(per_rank) > 0
    check(eng, merged, [100, 10])
    merged_b = job(eng, b, FUSED)                                # a different job: nothing stale
    check(eng, merged_b, [10, 100])
    assert merged_b != merged
    # after wcg_merge_runs the sorted records are lines without counts
    t = torch.frombuffer(bytearray(merged), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()
    eng.merge_runs(t.data_ptr(), [len(merged)])
    assert status_of(lambda: eng.top(10)) == WCG_ESTATE
    check(eng, job(eng, a, MULTI), [10])                         # and the next reduce has a top again


# ---------------------------------------------------------------- 8. two engines on one device
def test_two_engines(engine):
    e1, e2 = engine(), engine()
    a = {wire.mixed_key(i): 1 + (i * 13) % 977 for i in range(4000)}
    b = {wire.mixed_key(i): 3 + (i * 29) % 499 for i in range(1500, 4100)}
    ma = job(e1, a, MULTI)
    mb = job(e2, b, FUSED)
    for n in (10, 1024, 64):
        check(e1, ma, [n])
        check(e2, mb, [n])
    check(e2, mb, [10])
    check(e1, ma, [10])


# ---------------------------------------------------------------- 9. ranks
def test_ranks(built):
    """W = 3 owners of disjoint keys (exchange_local, then reduce on each): the ranks' tops combined
    on the host are the whole input's top"""
    import wcg
    from wcg.corpus import Generator, ASCII, UTF8
    from wcg.distributed import line_aligned_ranges
    W = 3
    data = Generator(ASCII, 30_000, 1.0, 91).bytes(5 << 19) + Generator(UTF8, 10_000, 1.0, 92).bytes(1 << 19) + b"\n"
    merged = ob.merged(data)
    engines = [wcg.Engine(device=0, max_keys=1 << 18) for _ in range(W)]
    try:
        for e, (lo, hi) in zip(engines, line_aligned_ranges(len(data), W, lambda i: data[i])):
            e.reset()
            e.map_host(data[lo:hi])
        wcg.exchange_local(engines, 64)
        nkeys = sum(e.reduce()[0] for e in engines)
        assert nkeys == merged.count(b"\n")
        for n in (10, 1024):
            ob.assert_same(wcg.top_merge([e.top(n) for e in engines], n), wcg.top_of_merged(merged, n))
    finally:
        for e in engines:
            e.close()


# ---------------------------------------------------------------- 10. text and the command line
def test_text_and_cli(built, tmp_path):
    from wcg import wc
    import wcg
    from wcg.corpus import Generator, ASCII, UTF8
    data = Generator(ASCII, 50_000, 1.0, 101).bytes(3 << 19) + Generator(UTF8, 20_000, 1.0, 102).bytes(1 << 19) + b"\n"
    path = tmp_path / "input.txt"
    path.write_bytes(data)
    want = wcg.top_of_merged(ob.merged(data), 10)
    assert want.count(b"\n") == 10
    ob.assert_same(wc.top(str(path), 10), want)
    assert sorted(os.listdir(tmp_path)) == ["input.txt"]         # no mrtmp.* files
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([PKG, ROOT]))
    child = subprocess.run([sys.executable, "-m", "wcg.wc", "top", str(path), "10"], env=env, cwd=str(tmp_path),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert child.returncode == 0, child.stderr[-2000:]
    assert child.stdout == want                                  # those bytes and nothing else
    assert sorted(os.listdir(tmp_path)) == ["input.txt"]
