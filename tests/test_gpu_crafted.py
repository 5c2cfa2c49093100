"""Crafted record units (tests/wire.py) through Engine.import_host: what text cannot reach.

Text gives small counts (the suite's largest was 2000000), so the code after the tables had never
run past seven digits: ndigits' compare ladder up to 10^19, put_digits' 64-bit branch, the byte
sums that place every later line, the LDS staging thresholds of the two formatters, u64 count sums
across imports, k_import's validation, and the all-ones prefix the sorts use as padding.  A unit's
count is a free u64, so a few thousand units reach all of it in milliseconds.

Every job is compared byte for byte with the plain-Python reference over the dict the units were
made from (wire.expect: oracle/wc_ref.py with arbitrary-precision integers), and nkeys / nbytes
with its line and byte counts.  Counts are >= 1 (0 is "merged duplicate, no line" internally) and
keys are letter bytes, except the all-ones test.

Reduce paths: a fresh engine's first job takes the multi-launch path (wcg_reduce.h + wcg_sort.h),
a job after a 2000-key warm-up the one-launch path (wcg_fused.h); reduce_path() is asserted.  Where
one test runs several multi-launch jobs on one engine, an empty job in between clears the key-count
hint again (as tests/test_gpu_fused.py::test_empty_and_letterless shows).
"""
import os
import random
import re
import struct

import pytest

from tests import oracle_bridge as ob
from tests import wire

pytestmark = pytest.mark.gpu

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mit-6.824-2015_amd", "csrc")


def _const(header, name):
    m = re.search(r"\b%s = (\d+)\b" % name, open(os.path.join(CSRC, header)).read())
    assert m, (header, name)
    return int(m.group(1))


FM_TILE = _const("wcg_reduce.h", "FM_NT") * _const("wcg_reduce.h", "FM_IPT")   # lines per tile of k_fmt_write
FM_STAGE = _const("wcg_reduce.h", "FM_STAGE")                                 # its LDS image
FR_STAGE = _const("wcg_fused.h", "FR_STAGE")                                  # the one-launch formatter's
FR_TARGET = _const("wcg_fused.h", "FR_TARGET")                                # mean records per bucket
FR_RCAP = _const("wcg_fused.h", "FR_CAP")                                     # records per bucket region

MULTI, FUSED = 0, 1
PATHS = [pytest.param(MULTI, id="multi-launch"), pytest.param(FUSED, id="one-launch")]

WARM = dict(zip(wire.ordered_keys(2000, 12, first=52 ** 3), range(1, 2001)))


@pytest.fixture
def engine(built):
    """engine(path): a fresh engine whose next job takes that reduce path"""
    import wcg
    made = []

    def make(path, max_keys=1 << 17):
        e = wcg.Engine(device=0, max_input_bytes=4 << 20, max_keys=max_keys)
        made.append(e)
        if path == FUSED:
            warm(e)
        return e
    yield make
    for e in made:
        e.close()


def warm(eng):
    """a 2000-key job: the key-count hint that sends the next job to the one-launch reduce"""
    eng.reset()
    eng.map_host(b"\n".join(k for k, c in WARM.items() for _ in range(1 + c % 3)) + b"\n")
    nk, nb = eng.reduce()
    assert nk == len(WARM)


def cold(eng):
    """an empty job: no hint, the next job takes the multi-launch path"""
    eng.reset()
    assert eng.reduce() == (0, 0)


def check(eng, counts, path):
    """reduce the job in the tables; the merged file, nkeys and nbytes against the reference"""
    nk, nb = eng.reduce()
    want = wire.expect(counts)
    ob.assert_same(eng.result(), want)
    assert nk == want.count(b"\n") == len(counts)
    assert nb == len(want)
    assert eng.reduce_path() == path
    return want


def run(eng, counts, path, seed=1, split=None):
    eng.reset()
    eng.import_host(wire.units(counts, seed=seed, split=split))
    return check(eng, counts, path)


# ---------------------------------------------------------------- a. digit widths
@pytest.mark.parametrize("path", PATHS)
def test_digit_widths(engine, path):
    """10^k - 1, 10^k, 10^k + 1 for k = 1..19, 2^32 - 1, 2^32, 2^32 + 1, 2^63 and 2^64 - 1, each with a
    key of every length class (1-7, 8-15, 16-32: slot cell, 33+: arena heap): the merged file, every
    -res-<r> for R = 3 one by one, all of them at once for R = 1, 3 and 64 (k_part_hist's byte sums),
    and the export's units decoded back to the same dict."""
    ihash = ob.wc_ref.ihash
    c = wire.edge_count_keys()
    eng = engine(path)
    run(eng, c, path)
    for r in range(3):
        assert eng.partition(3, r) == wire.expect_res(c, 3, r), r
    for R in (1, 3, 64):
        parts = eng.partitions(R)
        assert len(parts) == R
        for r in range(R):
            assert parts[r] == wire.expect_res(c, R, r), (R, r)
    blob, per_rank = eng.export_host(64, 4)
    assert len(blob) == 32 * sum(per_rank)
    pairs = list(wire.decode(blob))
    assert len(pairs) == len(c) and dict(pairs) == c                # counts survive the wire
    off = 0
    for rank, nu in enumerate(per_rank):                            # and every unit is at its owner
        mine = dict(wire.decode(blob[off:off + 32 * nu]))
        assert mine == {k: v for k, v in c.items() if (ihash(k) % 64) % 4 == rank}, rank
        off += 32 * nu


# ---------------------------------------------------------------- b. alignment sweep
@pytest.mark.parametrize("path", PATHS)
def test_alignment_sweep(engine, path):
    """3000 ten-byte keys in known order, counts cycling through all 20 widths, behind a first key
    of 1 + s letters for s = 0..15: every later tile (bucket) of the file starts at every
    (dst & 15), so the partial first and last 16 bytes of the staged copies are written at every
    offset (the merged file's equivalent of test_tile_boundaries' shift loop)."""
    keys = wire.ordered_keys(3000, 10)
    base = {k: wire.count_of_width(1 + i % 20, i) for i, k in enumerate(keys)}
    eng = engine(path)
    sizes = set()
    for s in range(16):
        first = b"A" * (1 + s)
        c = {first: 7, **base}
        assert min(c) == first
        if path == MULTI and s:
            cold(eng)
        want = run(eng, c, path, seed=s)
        sizes.add(len(want) % 16)
    assert len(sizes) == 16


# ---------------------------------------------------------------- c. FM_STAGE threshold
def threshold_job(pad, delta):
    """2048 + 8 nine-byte keys in known order: tile 0 (records 0..1023) is `pad` bytes mod 16,
    tile 1 (1024..2047) is FM_STAGE + delta - pad bytes"""
    keys = wire.ordered_keys(2 * FM_TILE + 8, 9)
    width = [1 + i % 20 for i in range(FM_TILE)] + [20] * FM_TILE + [1 + i % 20 for i in range(8)]
    t0 = sum(9 + 3 + w for w in width[:FM_TILE])
    width[19] -= (t0 - pad) % 16                                   # (record 19 has 20 digits)
    cut = FM_TILE * (9 + 3 + 20) - (FM_STAGE + delta - pad)        # bytes tile 1 must lose
    if cut < 0:                                                     # one letter more instead
        assert cut == -1
        keys[FM_TILE + 5] += b"z"
    i = FM_TILE
    while cut > 0:
        d = min(cut, 19, 3 + (i - FM_TILE) % 7)                     # a few counts, several widths
        width[i] -= d
        cut -= d
        i += 1
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    return {k: wire.count_of_width(w, j) for j, (k, w) in enumerate(zip(keys, width))}


@pytest.mark.parametrize("pad", [0, 15])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_fm_stage_threshold(engine, pad, delta):
    """k_fmt_write stages a tile in LDS only when pad + all <= FM_STAGE (pad = dst & 15): tile 1 of
    this job sits at FM_STAGE - 1, FM_STAGE and FM_STAGE + 1, at pad 0 and pad 15.  A 9-byte key
    with a 20-digit count is a 32-byte line, 1024 of them exactly FM_STAGE bytes; a few narrower
    counts (or one letter more) move the tile by the bytes needed.  The totals are computed here
    from the reference's lines and asserted, and the output buffer's alignment with them."""
    c = threshold_job(pad, delta)
    lines = wire.lines(c)
    assert len(lines) == 2 * FM_TILE + 8
    tile0 = sum(len(l) for l in lines[:FM_TILE])
    tile1 = sum(len(l) for l in lines[FM_TILE:2 * FM_TILE])
    assert tile0 % 16 == pad
    assert pad + tile1 == FM_STAGE + delta
    eng = engine(MULTI)
    run(eng, c, MULTI)
    ptr, nb = eng.result_device()
    assert ptr % 16 == 0                                            # so tile 1's dst & 15 is tile0 % 16
    # the same records as JSON lines (FMT_JSON_ALL through the same k_fmt_write)
    assert eng.partitions(1) == [wire.expect_res(c, 1, 0)]


# ---------------------------------------------------------------- d. FR_STAGE neighbourhood
def long_keys(n, seed, lo=34, hi=42):
    """n distinct keys of lo + 3 .. hi + 3 bytes: random letters, then the index in 3 letters"""
    rnd = random.Random(seed)
    abc = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
    return [("".join(rnd.choice(abc) for _ in range(rnd.randint(lo, hi)))).encode() + wire.letters(i, 3) for i in range(n)]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_fr_stage_neighbourhood(engine, seed):
    """The one-launch formatter stages a bucket's lines in LDS only when pad + W <= FR_STAGE.  The
    bucket borders come from the launch's own sample and cannot be fixed from outside, so coverage
    of the exact threshold is statistical: 20000 keys of ~40 bytes with 20-digit counts are
    ~64-byte lines, times the 256-record bucket target ~FR_STAGE bytes per bucket, and the ~80
    buckets of each of the four seeds spread around that mean on both sides of the threshold (the
    sample gives a bucket ~25 splitter candidates: sizes vary by ~20%), at any pad."""
    keys = long_keys(20000, seed)
    c = {k: wire.count_of_width(20, i) for i, k in enumerate(keys)}
    mean_line = len(wire.expect(c)) / len(c)
    assert abs(mean_line * FR_TARGET - FR_STAGE) < 0.03 * FR_STAGE
    eng = engine(FUSED)
    run(eng, c, FUSED, seed=seed)


@pytest.fixture
def fused_target():
    old = os.environ.get("WCG_FUSED_TARGET")

    def set_(v):
        os.environ["WCG_FUSED_TARGET"] = str(v)
    yield set_
    if old is None:
        os.environ.pop("WCG_FUSED_TARGET", None)
    else:
        os.environ["WCG_FUSED_TARGET"] = old


def test_fr_one_bucket_in_windows(engine, fused_target):
    """one bucket of every record (WCG_FUSED_TARGET past n): the region, the spill list, the
    workgroup's merge sort in global memory, and the lines written in windows of 2048 records, each
    far past FR_STAGE bytes (direct stores), the last one partial"""
    keys = long_keys(3 * FR_RCAP - 100, 9) + wire.ordered_keys(300, 9)
    c = {k: wire.count_of_width(1 + (7 * i) % 20, i) for i, k in enumerate(keys)}
    eng = engine(FUSED)
    fused_target(1 << 30)
    run(eng, c, FUSED)


def window_job(pad, delta):
    """2 x 2048 + 8 three-byte keys in known order for a one-bucket job: window 0 (records
    0..2047) is `pad` bytes mod 16, window 1 is FR_STAGE + delta - pad bytes (a 3-byte key with a
    2-digit count is an 8-byte line, 2048 of them exactly FR_STAGE)"""
    n = 2 * FR_RCAP + 8
    keys = [wire.letters(i, 3) for i in range(n)]
    width = [1 + i % 20 for i in range(FR_RCAP)] + [2] * FR_RCAP + [1 + i % 20 for i in range(8)]
    t0 = sum(3 + 3 + w for w in width[:FR_RCAP])
    width[19] -= (t0 - pad) % 16                                   # (record 19 has 20 digits)
    need = FR_STAGE + delta - pad - FR_RCAP * 8                    # bytes window 1 must gain
    assert -16 <= need <= 1
    for j in range(abs(need)):
        width[FR_RCAP + 3 + 97 * j] += 1 if need > 0 else -1
    assert keys == sorted(keys)
    return {k: wire.count_of_width(w, j) for j, (k, w) in enumerate(zip(keys, width))}


@pytest.mark.parametrize("pad", [0, 15])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_fr_stage_threshold_windows(engine, fused_target, pad, delta):
    """With one bucket the borders ARE fixed from outside: a bucket past its region is written in
    windows of 2048 sorted records (fr_format_big), each staged only when pad + W <= FR_STAGE.
    Window 1 of this job sits at FR_STAGE - 1, FR_STAGE and FR_STAGE + 1, at pad 0 and pad 15;
    the totals are computed from the reference's lines and asserted."""
    c = window_job(pad, delta)
    lines = wire.lines(c)
    win0 = sum(len(l) for l in lines[:FR_RCAP])
    win1 = sum(len(l) for l in lines[FR_RCAP:2 * FR_RCAP])
    assert win0 % 16 == pad
    assert pad + win1 == FR_STAGE + delta
    eng = engine(FUSED)
    fused_target(1 << 30)
    run(eng, c, FUSED)
    ptr, nb = eng.result_device()
    assert ptr % 16 == 0                                            # the bucket starts the file: window 1's pad is win0 % 16


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_fr_stage_threshold_one_small_bucket(engine, fused_target, delta):
    """one bucket within its region (fr_format_small) at the start of the file (pad 0): 512 lines of
    32 bytes are exactly FR_STAGE; one digit fewer or one letter more moves it by one"""
    keys = wire.ordered_keys(FR_STAGE // 32, 9)
    width = [20] * len(keys)
    if delta < 0:
        width[77] -= 1
    if delta > 0:
        keys[77] += b"z"
    assert keys == sorted(keys) and len(keys) <= FR_RCAP
    c = {k: wire.count_of_width(w, j) for j, (k, w) in enumerate(zip(keys, width))}
    assert len(wire.expect(c)) == FR_STAGE + delta
    eng = engine(FUSED)
    fused_target(1 << 30)
    run(eng, c, FUSED)
    ptr, nb = eng.result_device()
    assert ptr % 16 == 0 and nb == FR_STAGE + delta


# ---------------------------------------------------------------- e. sums
def sum_cases():
    """(parts) lists whose sums cross 2^32, a digit width, or both, in 2, 3 and 64 units.  (64 x 2^58
    is 2^64, one past a u64: the 64-unit cases end at 2^64 - 1 and at 2^63 instead.)"""
    return [
        [2 ** 32 - 1, 1],
        [9999999999, 1],
        [1, 2 ** 32 - 1],
        [5 * 10 ** 18, 5 * 10 ** 18],                               # 19 -> 20 digits
        [2 ** 63, 2 ** 63 - 1],                                     # 2^64 - 1
        [2 ** 32 - 1, 2 ** 32 - 1, 2],                              # 2^33
        [999, 1, 9000],                                             # 3 -> 5 digits
        [3 * 10 ** 9, 3 * 10 ** 9, 4 * 10 ** 9],                    # 10^10, each part below 2^32
        [2 ** 58] * 63 + [2 ** 58 - 1],                             # 2^64 - 1
        [2 ** 57] * 64,                                             # 2^63
        [2 ** 26] * 64,                                             # 2^32
        [156250] * 64,                                              # 10^7
    ]


SUM_LENGTHS = [3, 8, 15, 16, 32, 33, 100]


@pytest.mark.parametrize("calls", [1, 2])
@pytest.mark.parametrize("path", PATHS)
def test_sums_across_units(engine, path, calls):
    """one key in 2, 3 and 64 units of one import_host call (ginsert / add_agent on one slot from
    many threads), and the same units over two calls: the count is the u64 sum, for inline keys
    and long keys (slot cell and arena heap)"""
    rnd = random.Random(calls)
    blobs = [[], []]
    total = {}
    for ci, parts in enumerate(sum_cases()):
        for li, length in enumerate(SUM_LENGTHS):
            k = wire.key_of(ci * len(SUM_LENGTHS) + li, length)
            assert k not in total and sum(parts) <= wire.U64_MAX
            total[k] = sum(parts)
            for j, p in enumerate(parts):
                blobs[j % calls].append(wire.encode(k, p))
    for i in range(200):                                            # single-unit keys around them
        k = wire.mixed_key(1000 + i)
        total[k] = wire.EDGE_COUNTS[i % len(wire.EDGE_COUNTS)]
        blobs[i % calls].append(wire.encode(k, total[k]))
    eng = engine(path)
    eng.reset()
    for b in blobs[:calls]:
        rnd.shuffle(b)
        eng.import_host(b"".join(b))
    assert wire.add(*(wire.decode_counts(b"".join(b)) for b in blobs[:calls])) == total
    check(eng, total, path)
    parts = eng.partitions(3)
    for r in range(3):
        assert parts[r] == wire.expect_res(total, 3, r), r


@pytest.mark.parametrize("path", PATHS)
def test_map_then_import(engine, path):
    """map_host(text) and import_host(units) in one job ("or onto a live table", include/wcg.h):
    keys counted by both, by the text alone and by the units alone; sums cross a digit width,
    2^32 and reach 2^64 - 1"""
    both, only_text, only_units = [], [], []
    for i in range(120):
        (both if i % 3 == 0 else only_text if i % 3 == 1 else only_units).append(wire.mixed_key(i))
    text_counts = {k: 1 + i % 4 for i, k in enumerate(both + only_text)}
    toks = [k for k, n in text_counts.items() for _ in range(n)]
    random.Random(4).shuffle(toks)
    text = b" ".join(toks) + b"\n"
    assert ob.wc_ref.word_count(text) == text_counts
    tops = [10, 2 ** 32, 10 ** 19, 2 ** 64 - 1, 10 ** 10, 2 ** 63]     # what text + units add up to
    unit_counts = {k: tops[i % len(tops)] - text_counts[k] for i, k in enumerate(both)}
    unit_counts.update({k: wire.EDGE_COUNTS[(5 * i) % len(wire.EDGE_COUNTS)] for i, k in enumerate(only_units)})
    total = wire.add(text_counts, unit_counts)
    assert {total[k] for k in both} == set(tops)
    eng = engine(path)
    eng.reset()
    eng.map_host(text)
    eng.import_host(wire.units(unit_counts, seed=2))
    check(eng, total, path)


# ---------------------------------------------------------------- f. all-ones prefix
@pytest.mark.parametrize("path", PATHS)
def test_all_ones_prefix(engine, path):
    """three long keys whose 16-byte prefix is all ones - the sorts' padding value, which no key
    of the map has (only a crafted import) - among 5000 ordinary keys: both
    reduce paths order them bytewise, after every other key and among themselves by the bytes from
    16 on (one of them is exactly 16 bytes long).  result() only: these are not letters."""
    ones = b"\xff" * 16
    c = {wire.mixed_key(i): wire.EDGE_COUNTS[i % len(wire.EDGE_COUNTS)]
         for i in range(5000)}
    c[ones] = 2 ** 64 - 1
    c[ones + b"\xff" + b"abc"] = 10 ** 19
    c[ones + b"\x01" + b"z" * 30] = 2 ** 32
    assert sorted(c)[-3:] == [ones, ones + b"\x01" + b"z" * 30, ones + b"\xffabc"]
    eng = engine(path)
    want = run(eng, c, path)
    assert want.endswith(ones + b"\xffabc: 10000000000000000000\n")


# ---------------------------------------------------------------- g. shuffle with wide counts
def test_shuffle_wide_counts(built):
    """four engines import crafted shards with overlapping keys and wide counts; the local
    exchange (export, import: the counts add up at the owners), the owners' reduce and the merge
    of their runs at root 2 (k_line_recs and FMT_COPY over lines with up to 20 digits)"""
    import wcg
    from wcg._lib import ihash
    W, R = 4, 64
    rnd = random.Random(8)
    total, shards = {}, [{} for _ in range(W)]
    for i in range(1500):
        k = wire.mixed_key(i)
        t = wire.EDGE_COUNTS[i % len(wire.EDGE_COUNTS)] if i % 2 else wire.count_of_width(1 + i % 20, i)
        holders = rnd.sample(range(W), min(t, 1 + i % W))
        for p, part in zip(holders, wire.split_count(t, len(holders), rnd)):
            shards[p][k] = part
        total[k] = t
    assert wire.add(*shards) == total
    want = wire.expect(total)
    engines = [wcg.Engine(device=0, max_keys=1 << 16) for _ in range(W)]
    try:
        for p, e in enumerate(engines):
            e.reset()
            e.import_host(wire.units(shards[p], seed=p))
        sent, received = wcg.exchange_local(engines, R)
        assert sum(sent) == sum(received) > 0
        for p, e in enumerate(engines):
            owned = {k: v for k, v in total.items() if (ihash(k) % R) % W == p}
            nk, nb = e.reduce()
            mine = wire.expect(owned)
            ob.assert_same(e.result(), mine)                         # the owner's sorted run
            assert nk == len(owned) and nb == len(mine)
        nk, nb = wcg.gather_merge_local(engines, 2)
        assert nk == len(total) == want.count(b"\n") and nb == len(want)
        ob.assert_same(engines[2].result(), want)
    finally:
        for e in engines:
            e.close()


# ---------------------------------------------------------------- h. malformed units
GOOD_A = dict(zip(wire.ordered_keys(300, 11), (wire.count_of_width(1 + i % 20, i) for i in range(300))))
GOOD_B = {wire.mixed_key(i): 1 + i for i in range(300)}
GOOD = wire.add(GOOD_A, GOOD_B)


def raw_unit(first16, cnt, ref):
    hi, lo = struct.unpack(">QQ", first16.ljust(16, b"\0")[:16])
    return struct.pack("<QQQQ", hi, lo, cnt, ref)


def cont_unit(chunk):
    return chunk.ljust(24, b"\0")[:24] + struct.pack("<Q", wire.CONT_MARK)


def malformed(case):
    """(units, at_end): units k_export_write cannot have written"""
    if case == "inline-ref-0":
        return raw_unit(b"abc", 5, 0), False
    if case == "inline-ref-16":
        return raw_unit(b"abcdefghijklmnop", 5, 16), False
    if case == "long-len-15":
        return raw_unit(b"abcdefghijklmno", 5, wire.LONG_FLAG | 15 << 40) + cont_unit(b"abcdefghijklmno"), False
    assert case == "long-past-end"                                  # 100 bytes need 5 continuation units
    key = b"abcdefghijklmnopqrstuvwxyz" * 4
    return raw_unit(key, 5, wire.LONG_FLAG | 100 << 40) + cont_unit(key[:24]) + cont_unit(key[24:48]), True


@pytest.mark.parametrize("mode", ["reduce", "async", "general"])
@pytest.mark.parametrize("case", ["inline-ref-0", "inline-ref-16", "long-len-15", "long-past-end"])
def test_malformed_units(engine, record_property, case, mode):
    """k_import's validation, one malformed unit among 600 good keys, on an engine that first ran a
    good job: reduce() (one-launch path), reduce_async() / reduce_wait(), and the multi-launch
    path (after an empty job) raise WCG_EINVAL for an inline unit of length 0 or 16 and a long
    header of length 15; a long header whose continuation units would run past the end of the
    buffer raises a non-OK status (WCG_EFULL today, through `overflow`; recorded).  reset() and a
    good job are exact again afterwards."""
    from wcg._lib import WcgError, WCG_EINVAL, WCG_OK
    bad, at_end = malformed(case)
    a, b = wire.units(GOOD_A, seed=1), wire.units(GOOD_B, seed=2)
    blob = a + b + bad if at_end else a + bad + b
    eng = engine(FUSED)
    run(eng, GOOD, FUSED)                                           # the good job
    if mode == "general":
        cold(eng)
    eng.reset()
    eng.import_host(blob)
    with pytest.raises(WcgError) as ex:
        if mode == "async":
            eng.reduce_async()
            eng.reduce_wait()
        else:
            eng.reduce()
    status = ex.value.status
    record_property("status", status)
    print(f"{case} / {mode}: status {status} ({ex.value})")
    assert status != WCG_OK
    if not at_end:
        assert status == WCG_EINVAL
    eng.reset()
    eng.import_host(a + b)
    nk, nb = eng.reduce()
    want = wire.expect(GOOD)
    ob.assert_same(eng.result(), want)
    assert nk == len(GOOD) and nb == len(want)


@pytest.mark.parametrize("path", PATHS)
def test_lone_continuation_unit_is_skipped(engine, path):
    """a continuation unit without a header is skipped silently (k_import: every unit says what it
    is); documented behaviour, not an error: the output is the reference without it"""
    a, b = wire.units(GOOD_A, seed=3), wire.units(GOOD_B, seed=4)
    eng = engine(path)
    eng.reset()
    eng.import_host(cont_unit(b"orphan") + a + cont_unit(b"abcdefghijklmnopqrstuvwx") + b + cont_unit(b"z"))
    check(eng, GOOD, path)
