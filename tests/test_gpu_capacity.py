"""The "buffer full" branches between k_map and the tables, forced on a few MiB of text.

Every stage between k_map and the tables writes into a buffer of fixed size and has a branch for
"full" that production sizing makes rare (regions of at least 2048 units, partitions of at least
1024 entries, a record log of max_keys + 65536 records).  Four test knobs in csrc/wcg_api.hip
shrink a capacity the kernels already receive as an argument, so these branches run here:

  WCG_REGION_CAP     miss-log region of one (map workgroup, bucket): k_map's log_push, both
                     store_pending lambdas and the end-of-kernel LDS flush zero the region's tail
                     and insert into the global table; region_len is clamped; my_global reaches
                     DevState::global_ops through wg_stats (compaction and wcg_reset decide from
                     that counter alone whether a two-pass job's global table is visited)
  WCG_RP_CAP2        k_rp's sub-bucket region: to_region, from a full LDS buffer and from the
                     entry-by-entry write of a buffer that runs past its region (sdirect)
  WCG_LONG_PART_CAP  long-key partition: k_long_hash's fenced ltab_add per entry
  WCG_EMIT_CAP       pass-2 record log: k_agg<AGG_EMIT> sends records past the end to the global
                     table, k_long_agg to the long-key table

Every job is compared byte for byte with the C oracle: the merged file, nkeys and nbytes, the token
and long-token counts, the three -res- files of R = 3; overflow and spin_fail are 0.

A test that passes with the fallback never taken is worth nothing, so each test asserts evidence
that it was.  Where it can, the evidence is computed from the input alone (pigeonhole): a map
launch over n bytes has at most G = ceil(ceil(n / 992) / 16) workgroups, every distinct inline key
of a call is logged at least once (by a miss or by the flush) and an entry takes at least one
unit, so D > G * P * R distinct keys do not fit G * P regions of R units (P = 96 buckets in
one-pass jobs, 64 in two-pass jobs); likewise D distinct long keys against 2048 partitions of
`cap` entries.  tests/test_capacity_inputs.py checks these inequalities, and the builders' key
counts, without a GPU.  Two-pass jobs keep the global table empty unless a fallback ran, so there
a control run of the same input without the knob asserts global_ops == 0 and the run with the
knob asserts global_ops > 0; the record log's evidence is stats()["emitted"] > cap.

What a few MiB cannot do: fill a region of 256 units.  A map workgroup of these launches reads one
16-step window (15.5 KiB, about 1600 tokens over 64 or 96 buckets), some tens of units per region,
so the R = 256 cases run the knob's path near its default and are checked exactly, but assert no
evidence (the two-pass one prints its global_ops).

Engines: max_keys = 1 << 20 gives one-pass jobs (k_map<0, true>, split buckets, P = 96, k_agg
flushing into the global table); max_keys = (4 << 20) + 1 gives two-pass jobs through the
library's own rule (k_map<0, false>, P = 64, k_rp, pass 2, the record log).
"""
import functools
import os
import random

import pytest

from tests import oracle_bridge as ob

pytestmark = pytest.mark.gpu

KNOBS = ("WCG_REGION_CAP", "WCG_RP_CAP2", "WCG_LONG_PART_CAP", "WCG_EMIT_CAP")
R_MIN = 4                       # the smallest WCG_REGION_CAP the library accepts
P_ONE, P_TWO = 96, 64           # miss buckets of one-pass (64 short + 32 medium) and two-pass jobs
LQ = 2048                       # long-key partitions
LONG_SMALL_MAX = 4096           # more long tokens in the previous job: k_long_hash / k_long_agg
MAP_STEP, MAP_WAVES = 992, 16   # input bytes per wave step, waves per map workgroup

ABC = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
MULTI, FUSED = 0, 1


def map_groups(n):
    """the most workgroups a map launch over n bytes has"""
    steps = -(-n // MAP_STEP)
    return -(-steps // MAP_WAVES)


# ------------------------------------------------------------------------------- builders
def inline_keys(D, seed):
    """D distinct letter keys, lengths cycling 3..15 (3..7: 1-unit entries, 8..15: 2 units): the
    index within the length class in three letters, then random letters"""
    rnd = random.Random(seed)
    keys = []
    for i in range(D):
        n, j = 3 + i % 13, i // 13
        assert j < 52 ** 3
        keys.append(bytes((ABC[j // 2704], ABC[j // 52 % 52], ABC[j % 52])) + bytes(rnd.choices(ABC, k=n - 3)))
    return keys


def join_tokens(toks):
    """separators alternate between newline and space"""
    out = bytearray()
    for i, t in enumerate(toks):
        out += t
        out.append(32 if i & 1 else 10)
    return bytes(out)


def inline_text_of(keys, seed, hot, reps):
    """every key once and the first `hot` keys `reps` times more (all lengths, so the LDS flush logs
    short and medium entries that carry a count: 2 and 3 units), shuffled"""
    toks = list(keys) + keys[:hot] * reps
    random.Random(seed + 1000).shuffle(toks)
    return join_tokens(toks)


def inline_text(D, seed, hot=300, reps=600):
    return inline_text_of(inline_keys(D, seed), seed, hot, reps)


def long_keys(D, seed):
    """D distinct keys of 16..80 bytes.  A third share their first 32 bytes in groups of eight (so
    bytes past 32 are compared from the input), some are exactly 16, 32 and 33 bytes, a tenth (and
    a quarter of the shared prefixes) hold 2- and 3-byte UTF-8 letters."""
    rnd = random.Random(seed)

    def idx4(i):
        return bytes((ABC[i // 140608 % 52], ABC[i // 2704 % 52], ABC[i // 52 % 52], ABC[i % 52]))

    def fill(nbytes, utf):
        out = bytearray()
        while len(out) < nbytes:
            left, x = nbytes - len(out), rnd.random()
            if utf and left >= 3 and x < 0.25:
                out += "語".encode()
            elif utf and left >= 2 and x < 0.6:
                out += "é".encode()
            else:
                out.append(rnd.choice(ABC))
        return bytes(out)

    prefix = [b"zz" + idx4(g) + fill(26, g % 4 == 0) for g in range(D // 24 + 1)]
    keys = []
    for i in range(D):
        utf = i % 10 == 7
        if i % 3 == 0:
            n = 33 + (i * 5) % 48                                   # 33..80
            keys.append(prefix[i // 24] + bytes((ABC[i // 3 % 8],)) + fill(n - 33, utf))
        else:
            n = {1: 16, 2: 32, 4: 33}.get(i % 50, 16 + (i * 7) % 65)   # 16..80
            keys.append(idx4(i) + fill(n - 4, utf))
    return keys


def long_text_of(keys, seed):
    """key i 1 + i % 5 times, shuffled"""
    toks = [k for i, k in enumerate(keys) for _ in range(1 + i % 5)]
    random.Random(seed + 2000).shuffle(toks)
    return join_tokens(toks)


def long_text(D, seed):
    return long_text_of(long_keys(D, seed), seed)


# ------------------------------------------------------------------------------- corpora
# name -> the job's map calls.  `distinct` gives, per call, the distinct inline and long keys the
# builders put there (tests/test_capacity_inputs.py checks them against the oracle's count).
def _small():
    # 10 hot keys x 350: the bytes the pigeonhole bound for R = 16, P = 96 leaves (65 workgroups)
    return (inline_text(100_000, 1, hot=10, reps=350),)


def _big():
    return (inline_text(100_000, 2),)


def _other():
    return (inline_text(30_000, 3, hot=100, reps=40) + long_text(500, 3),)


def _pair():
    k = inline_keys(100_000, 4)                                     # the calls share a third of their keys
    return (inline_text_of(k[:60_000], 4, 10, 350), inline_text_of(k[40_000:], 5, 10, 350))


def _sub():
    # 30 hot keys x 2500: every map workgroup logs each of them once as a miss and once, with a
    # count, from its flush, and all of those entries meet in one sub-bucket per k_rp slice
    return (inline_text(300_000, 6, hot=30, reps=2500),)


def _long():
    return (long_text(20_000, 7),)


def _long_pair():
    k = long_keys(20_000, 8)
    return (long_text_of(k[:12_000], 8), long_text_of(k[8_000:], 9))


def _long_prime():
    return (long_text(2_500, 10),)


def _log():
    return (inline_text(100_000, 11, hot=10, reps=350) + long_text(5_000, 11),)


def _mixed_pair():
    k, l = inline_keys(60_000, 12), long_keys(6_000, 12)
    return (inline_text_of(k[:40_000], 12, 10, 200) + long_text_of(l[:4_000], 12),
            inline_text_of(k[20_000:], 13, 10, 200) + long_text_of(l[2_000:], 13))


BUILD = {"small": _small, "big": _big, "other": _other, "pair": _pair, "sub": _sub, "long": _long,
         "long_pair": _long_pair, "long_prime": _long_prime, "log": _log, "mixed_pair": _mixed_pair}
# per call: (distinct inline keys, distinct long keys)
DISTINCT = {"small": [(100_000, 0)], "big": [(100_000, 0)], "other": [(30_000, 500)],
            "pair": [(60_000, 0), (60_000, 0)], "sub": [(300_000, 0)], "long": [(0, 20_000)],
            "long_pair": [(0, 12_000), (0, 12_000)], "long_prime": [(0, 2_500)], "log": [(100_000, 5_000)],
            "mixed_pair": [(40_000, 4_000), (40_000, 4_000)]}
# the whole job's distinct keys (calls of a pair share some)
JOB_KEYS = {"small": 100_000, "big": 100_000, "other": 30_500, "pair": 100_000, "sub": 300_000, "long": 20_000,
            "long_pair": 20_000, "long_prime": 2_500, "log": 105_000, "mixed_pair": 66_000}
# (corpus, P, R) of every pigeonhole assert below, and (corpus, cap) of the long-partition ones
REGION_BOUNDS = [(c, p, r) for c, p in (("small", P_ONE), ("small", P_TWO), ("pair", P_TWO)) for r in (R_MIN, 16)]
REGION_BOUNDS += [("big", P_ONE, R_MIN), ("mixed_pair", P_ONE, R_MIN), ("mixed_pair", P_TWO, R_MIN)]
PART_BOUNDS = [("long", 2), ("long_pair", 2), ("mixed_pair", 1)]


@functools.lru_cache(maxsize=None)
def corpus(name):
    calls = BUILD[name]()
    assert all(c[-1:] in (b" ", b"\n") for c in calls)              # so the job is their concatenation
    return calls


def regions_overfull(name, P, R):
    """the pigeonhole bound, for every call of the job: more distinct inline keys than units"""
    return all(d > map_groups(len(c)) * P * R for c, (d, _) in zip(corpus(name), DISTINCT[name]))


def partitions_overfull(name, cap):
    return all(d > LQ * cap for _, d in DISTINCT[name])


class Want:
    """the oracle's answers for one job, computed once and shared"""

    def __init__(self, data):
        r = ob.Result(data)
        self.merged = r.merged()
        self.res = [r.res(3, k) for k in range(3)]
        self.nkeys, self.ntokens = r.nkeys, r.ntokens
        self.long_tokens = self.long_keys = 0
        for line in self.merged.splitlines():
            k, c = line.rsplit(b": ", 1)
            if len(k) >= 16:
                self.long_tokens += int(c)
                self.long_keys += 1


@functools.lru_cache(maxsize=None)
def want(name):
    return Want(b"".join(corpus(name)))


# ------------------------------------------------------------------------------- fixtures
@pytest.fixture
def knobs():
    """knobs(WCG_REGION_CAP=4, ...): exactly these capacity knobs set, the others unset; all are
    read by the library on every call; restored afterwards"""
    old = {k: os.environ.get(k) for k in KNOBS}

    def set_(**kv):
        assert set(kv) <= set(KNOBS)
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in kv.items():
            os.environ[k] = str(v)
    yield set_
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def one_pass(built):
    import wcg
    e = wcg.Engine(device=0, max_input_bytes=8 << 20, max_keys=1 << 20)
    yield e
    e.close()


@pytest.fixture(scope="module")
def two_pass(built):
    import wcg
    e = wcg.Engine(device=0, max_input_bytes=8 << 20, max_keys=(4 << 20) + 1)
    yield e
    e.close()


def job(eng, name):
    """one job (a reset, the corpus' map calls, the reduce) against the oracle; its stats"""
    w = want(name)
    eng.reset()
    for c in corpus(name):
        eng.map_host(c)
    nk, nb = eng.reduce()
    st = eng.stats()
    ob.assert_same(eng.result(), w.merged)
    assert (nk, nb) == (w.nkeys, len(w.merged))
    assert st["tokens"] == w.ntokens
    assert st["long_tokens"] == w.long_tokens
    parts = eng.partitions(3)
    for r in range(3):
        ob.assert_same(parts[r], w.res[r])
    assert st["overflow"] == 0 and st["spin_fail"] == 0
    return st


def twice(eng, name):
    """the job two times over: the second run finds the buffers laid out as it will use them and
    full of the first run's units, and which entry a full region cuts off depends on the order of
    the atomics, so units that a fallback should have zeroed, and did not, are read as entries"""
    job(eng, name)
    return job(eng, name)


def cold(eng):
    """an empty job: no key-count hint, the next job takes the multi-launch reduce (as a fresh
    engine's first job does)"""
    eng.reset()
    assert eng.reduce() == (0, 0)


def warm(eng):
    """a 2000-key job: the hint that sends the next job to the one-launch reduce"""
    eng.reset()
    eng.map_host(join_tokens(inline_keys(2000, 99)))
    assert eng.reduce()[0] == 2000


def prime_long(eng):
    """a job with more than LONG_SMALL_MAX long tokens: the next one-pass job's long tokens go through
    k_long_hash / k_long_agg, not long_small"""
    st = job(eng, "long_prime")
    assert st["long_tokens"] > LONG_SMALL_MAX


# ------------------------------------------------------------------------------- a. regions, one pass
@pytest.mark.parametrize("path", [pytest.param(MULTI, id="multi-launch"), pytest.param(FUSED, id="one-launch")])
@pytest.mark.parametrize("R,name", [(R_MIN, "small"), (R_MIN, "big"), (16, "small"), (256, "big")])
def test_region_full_one_pass(one_pass, knobs, R, name, path):
    """k_map<0, true> with regions of R units: at R = 4 and 16 more distinct keys than the launch's
    regions have units, so entries are refused.  Split buckets hold one kind of key, so a miss (1
    unit in a short region, 2 in a medium one, the cap even) either fits or finds the region full;
    the entries that are cut off part-way are the flush's, which carry counts (2 and 3 units):
    `big`, whose 300 hot keys every workgroup's table holds, at R = 4 where they meet regions that the
    misses left nearly full.  Then a job of other keys with the knob unset, exact: nothing was left
    behind."""
    if R != 256:
        assert regions_overfull(name, P_ONE, R)
    if path == FUSED:
        warm(one_pass)
    knobs(WCG_REGION_CAP=R)
    for _ in range(2):                                              # (see twice)
        if path == MULTI:
            cold(one_pass)
        st = job(one_pass, name)
        assert one_pass.reduce_path() == path
    print(f"WCG_REGION_CAP={R} {name}: global_ops {st['global_ops']} lds_hits {st['lds_hits']}")
    knobs()
    job(one_pass, "other")


# ------------------------------------------------------------------------------- b. regions, two passes
@pytest.mark.parametrize("R", [R_MIN, 16, 256])
def test_region_full_two_pass(two_pass, knobs, R):
    """k_map<0, false> with regions of R units, two map calls that share a third of their keys: a
    shared key reaches the global table in one call and the record log in the other and is merged
    after the sort.  Control: the same job without the knob leaves global_ops at 0.  Afterwards a
    reset and a job of other keys with the knob unset: exact, and global_ops is 0 again, so the
    reset found and cleared the slots the fallbacks had claimed (by list: fewer than GLIST_CAP)."""
    knobs()
    assert job(two_pass, "pair")["global_ops"] == 0
    knobs(WCG_REGION_CAP=R)
    st = twice(two_pass, "pair")
    print(f"WCG_REGION_CAP={R}: global_ops {st['global_ops']} emitted {st['emitted']}")
    if R != 256:
        assert regions_overfull("pair", P_TWO, R)
        assert st["global_ops"] > 0
        assert st["global_ops"] < 1 << 20                           # GLIST_CAP: compaction and reset by list
    knobs()
    assert job(two_pass, "other")["global_ops"] == 0


def test_region_full_two_pass_one_call(two_pass, knobs):
    """the one-call corpus of the one-pass tests through the two-pass kernels, at both small R"""
    for R in (R_MIN, 16):
        assert regions_overfull("small", P_TWO, R)
        knobs()
        assert job(two_pass, "small")["global_ops"] == 0
        knobs(WCG_REGION_CAP=R)
        assert twice(two_pass, "small")["global_ops"] > 0
    knobs()
    assert job(two_pass, "other")["global_ops"] == 0


# ------------------------------------------------------------------------------- c. k_rp's sub-buckets
@pytest.mark.parametrize("cap2", [2, 64])
def test_sub_bucket_full(two_pass, knobs, cap2):
    """k_rp with sub-bucket regions of cap2 units: at 2 every entry of two or three units goes to
    the global table; at 64 the regions of the hot keys' sub-buckets fill with the map workgroups'
    miss and flush entries (LDS buffers written past a region's end: sdirect)."""
    knobs()
    assert job(two_pass, "sub")["global_ops"] == 0
    knobs(WCG_RP_CAP2=cap2)
    st = twice(two_pass, "sub")
    print(f"WCG_RP_CAP2={cap2}: global_ops {st['global_ops']}")
    assert st["global_ops"] > 0
    knobs()
    assert job(two_pass, "other")["global_ops"] == 0


# ------------------------------------------------------------------------------- d. long-key partitions
@pytest.mark.parametrize("which", ["one_pass", "two_pass"])
def test_long_partition_full(request, knobs, which):
    """k_long_hash with partitions of 2 entries: 20 000 distinct long keys against 4096 entries, the
    rest counted by fenced ltab_add.  One pass: after a job with more than 4096 long tokens, so the
    call takes k_long_hash / k_long_agg.  Two passes: two map calls with shared keys, so a key is
    counted by k_long_agg into the record log and by the fallback into the long-key table."""
    eng = request.getfixturevalue(which)
    name = "long" if which == "one_pass" else "long_pair"
    assert partitions_overfull(name, 2)
    knobs()
    if which == "one_pass":
        prime_long(eng)
    knobs(WCG_LONG_PART_CAP=2)
    st = twice(eng, name)
    assert st["long_tokens"] == want(name).long_tokens > LONG_SMALL_MAX
    assert want(name).long_keys == JOB_KEYS[name]
    knobs()
    job(eng, "other")


# ------------------------------------------------------------------------------- e. the record log
def test_record_log_full(two_pass, knobs):
    """a record log of 20 000 records for 105 000 keys: k_agg<AGG_EMIT> sends the records past the
    end to the global table and k_long_agg its keys to the long-key table (the path that
    test_c4_4gib_sixteen_calls_record_log_overflow reaches with 4 GiB)."""
    cap = 20_000
    knobs()
    assert job(two_pass, "log")["global_ops"] == 0
    knobs(WCG_EMIT_CAP=cap)
    st = twice(two_pass, "log")
    assert st["emitted"] > cap
    assert st["global_ops"] > 0
    knobs()
    assert job(two_pass, "other")["global_ops"] == 0


# ------------------------------------------------------------------------------- f. everything at once
@pytest.mark.parametrize("which", ["one_pass", "two_pass"])
def test_all_small_at_once(request, knobs, which):
    """every knob at its smallest value, two map calls of mixed inline and long text"""
    eng = request.getfixturevalue(which)
    P = P_ONE if which == "one_pass" else P_TWO
    assert regions_overfull("mixed_pair", P, R_MIN) and partitions_overfull("mixed_pair", 1)
    knobs()
    if which == "one_pass":
        prime_long(eng)
    else:
        assert job(eng, "mixed_pair")["global_ops"] == 0
    knobs(WCG_REGION_CAP=R_MIN, WCG_RP_CAP2=2, WCG_LONG_PART_CAP=1, WCG_EMIT_CAP=0)
    st = twice(eng, "mixed_pair")
    assert st["global_ops"] > 0
    if which == "two_pass":
        assert st["emitted"] > 0
    knobs()
    job(eng, "other")
