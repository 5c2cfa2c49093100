"""GPU: wcg_map_json's own kernels (k_json_count / k_json_write, csrc/wcg_reduce.h), byte-exact.

wcg_map_json shares no code with the hot path: its tokenizer (for_tokens over letter_byte and
go_decode), its FNV loop and its ordering scheme (per-thread sums, a scan over the threads of a
workgroup, a scan over (partition, workgroup)) are its own.  Every case here compares the R files
of one call with a restatement that uses none of libwcg: tokens from the C oracle (letter ranges
pinned to Unicode 13), partition = wc_ref.ihash(token) % R, line = {"Key":"tok","Value":"1"}\\n.

  a. every golden vector, at the fixture's own R values, and the fixture's pinned merged file
     rebuilt from the GPU's lines alone;
  b. multi-byte letters and invalid sequences across every thread (2048 B) and workgroup
     (262144 B) boundary, at every phase of the pattern;
  c. tokens longer than a thread's and a workgroup's span;
  d. more than 128 partitions (the partition-group loop, its tail and its re-zeroing) and more
     than 4096 (partition, workgroup) offsets (a second round of the scan); R = 1 is the whole
     token stream in input order;
  e. random mixed valid / invalid UTF-8 at random R;
  f. every Unicode scalar value through letter_byte's look-back;
  g. the call contract: size query, cap, the nreduce limits, buffer reuse across calls;
  h. independence from the aggregation tables, the cached results and a pending async job.
"""
import base64
import ctypes
import glob
import json
import math
import os
import random
import re

import pytest

from tests import oracle_bridge as ob
from tests.oracle_bridge import wc_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "mit-6.824-2015_amd", "csrc")

# The kernels' geometry (csrc/wcg_reduce.h, csrc/wcg_sort.h), stated here once; every size below
# derives from these, and test_constants_match_the_kernels fails when the sources move on.
JS_NT = 128                  # threads of a workgroup
JS_SUB = 2048                # input bytes a thread owns
JS_PG = 128                  # partitions per walk over the input
JS_WG = JS_NT * JS_SUB       # input bytes a workgroup owns: 262144
SCAN_ROUND = 4096            # entries k_scan_u64 takes per round (1024 threads x 4)
MAX_NREDUCE = 1024           # PT_MAXR: the partition calls' limit, wcg_map_json's too


# ---------------------------------------------------------------- the restatement
_HASH = {}


def _ihash(tok):
    h = _HASH.get(tok)
    if h is None:
        h = _HASH[tok] = wc_ref.ihash(tok)
    return h


def _line(tok):
    return b'{"Key":"' + tok + b'","Value":"1"}\n'


def files_of(toks, R):
    """DoMap's R intermediate files for a token stream (mapreduce.go:214-230)."""
    outs = [[] for _ in range(R)]
    for t in toks:
        outs[_ihash(t) % R].append(_line(t))
    return [b"".join(o) for o in outs]


def expected(data, R):
    return files_of(ob.tokens(data), R)


def assert_files(got, want, what=""):
    """Byte-exact equality of two lists of files; a failure names the first differing file and
    offset (pytest's own diff of multi-megabyte byte strings takes minutes)."""
    assert len(got) == len(want), f"{what}: {len(got)} files, want {len(want)}"
    for r, (g, w) in enumerate(zip(got, want)):
        if g != w:
            k = len(os.path.commonprefix([g, w]))
            lo = max(0, k - 24)
            raise AssertionError(f"{what}: file {r} of {len(want)} differs at offset {k} ({len(g)} vs {len(w)} "
                                 f"bytes): got {g[lo:k + 48]!r} want {w[lo:k + 48]!r}")


def check(eng, data, R, what=""):
    got = eng.map_json(data, R)
    assert_files(got, expected(data, R), what or f"n={len(data)} R={R}")
    return got


def keys_of(part, what=""):
    """The keys of one GPU-written file, from its bytes alone."""
    if not part:
        return []
    assert part.endswith(b"\n"), what
    keys = []
    for ln in part[:-1].split(b"\n"):
        assert ln.startswith(b'{"Key":"') and ln.endswith(b'","Value":"1"}'), (what, ln[:80])
        keys.append(ln[8:-14])
    return keys


def raw_call(e, data, R, cap=None, fill=True, nsizes=None):
    """wcg_map_json through the C ABI: (status, sizes, bytes).  cap = None: the size query's total."""
    sizes = (ctypes.c_uint64 * (nsizes or max(R, 1)))()
    if not fill:
        rc = e._lib.wcg_map_json(e._ctx, data, len(data), R, None, 0, sizes)
        return rc, list(sizes), b""
    if cap is None:
        rc = e._lib.wcg_map_json(e._ctx, data, len(data), R, None, 0, sizes)
        assert rc == 0
        cap = sum(sizes)
    buf = ctypes.create_string_buffer(max(cap, 1))
    rc = e._lib.wcg_map_json(e._ctx, data, len(data), R, buf, cap, sizes)
    return rc, list(sizes), buf.raw[:cap]


@pytest.fixture(scope="module")
def eng(built):
    import wcg
    e = wcg.Engine(0, 0, 1 << 16)
    yield e
    e.close()


def test_constants_match_the_kernels():
    src = open(os.path.join(CSRC, "wcg_reduce.h")).read()
    for name, val in (("JS_NT", JS_NT), ("JS_SUB", JS_SUB), ("JS_PG", JS_PG), ("PT_MAXR", MAX_NREDUCE)):
        m = re.search(r"constexpr \w+ %s = (\d+);" % name, src)
        assert m and int(m.group(1)) == val, name
    scan = open(os.path.join(CSRC, "wcg_sort.h")).read()
    body = scan[scan.index("void k_scan_u64("):]
    assert "base += 1024 * 4" in body[:400] and SCAN_ROUND == 1024 * 4


def test_restatement_equals_wc_ref(built):
    """the helper above (C oracle tokens, memoised hash) against wc_ref.map_files (pure Python
    tokens and hash): two restatements of DoMap, tied together once on a small mixed input"""
    data = ("the quick brown fox, The fox; ǅungla é́é 中文 и кот 𠀀𠀁 x".encode()
            + b"\x80 ab\xe4\xb8 cd\xed\xa0\x80ef\xf0\x90 gh\xc0\xafij\x00kl\xffmn the fox\n") * 7
    for R in (1, 2, 3, 5, 129, 300):
        assert_files(expected(data, R), wc_ref.map_files(data, R), f"restatement R={R}")


# ---------------------------------------------------------------- a. golden vectors
def _golden_names():
    return [os.path.basename(p)[:-5] for p in sorted(glob.glob(os.path.join(GOLDEN, "*.json")))
            if not p.endswith("fnv1a32_kat.json")]


@pytest.mark.parametrize("name", _golden_names())
def test_golden(eng, name):
    d = json.load(open(os.path.join(GOLDEN, name + ".json")))
    data = base64.b64decode(d["input_b64"])
    assert d["res"], name
    for R in sorted(int(k) for k in d["res"]):
        got = check(eng, data, R, f"{name} R={R}")
        counts, nlines = {}, 0
        for r, part in enumerate(got):
            for k in keys_of(part, (name, R, r)):
                assert wc_ref.ihash(k) % R == r, (name, R, r, k)
                counts[k] = counts.get(k, 0) + 1
                nlines += 1
        assert nlines == d["ntokens"], (name, R)
        assert wc_ref.merged_output(counts) == base64.b64decode(d["merged_b64"]), (name, R)
        assert eng.map_json(b"", R) == [b""] * R


# ---------------------------------------------------------------- b. thread and workgroup boundaries
PATTERN_VALID = "é中𠀀ab中 ".encode()
# a truncated 3-byte lead, a combining mark that splits a token, a stray continuation byte before
# a letter, an encoded surrogate and a truncated 4-byte lead
PATTERN_INVALID = b"ab\xe4\xb8 " + "é́é".encode() + b" \x80" + "中".encode() + b"\xed\xa0\x80q\xf0\x90 "


def _boundary_pattern(family):
    p = PATTERN_VALID if family == "valid" else PATTERN_INVALID
    if math.gcd(len(p), JS_SUB) != 1:
        p += b" "
    return p


@pytest.mark.parametrize("family", ["valid", "invalid"])
def test_runes_across_thread_and_workgroup_boundaries(eng, family):
    p = _boundary_pattern(family)
    L = len(p)
    if family == "valid":
        assert L == 15
    assert math.gcd(L, JS_SUB) == 1
    reps = -(-(2 * JS_WG + 4096) // L)
    shifts = range(L)
    # from the inputs alone: over the shifts every byte phase of the pattern falls on both workgroup
    # boundaries; within one input the 2048-byte boundaries see every phase (gcd = 1, > L of them)
    for edge in (JS_WG, 2 * JS_WG):
        assert {(edge - s) % L for s in shifts} == set(range(L))
    assert reps * L >= 2 * JS_WG + 4096 and (reps * L) // JS_SUB > L
    for s in shifts:
        data = b"a" * s + p * reps
        assert data[s:s + L] == p and len(data) > 2 * JS_WG
        check(eng, data, 3, f"{family} shift={s}")


# ---------------------------------------------------------------- c. long tokens
LONG_START = JS_SUB * 3 + 1000


def _long_input(start, token):
    filler = b"lorem ipsum dolor sit amet consectetur "
    head = (filler * (start // len(filler) + 1))[:start - 1] + b" "
    return head + token + b" after the long token come short words again\n"


def _ascii_token(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ") for _ in range(n))


@pytest.mark.parametrize("case", ["2047", "2048", "2049", "65535", "65535_cjk", "workgroup"])
def test_long_tokens(eng, case):
    """Tokens longer than a thread's span (every following thread inside the token skips "the
    previous owner's token") and than a workgroup's: workgroup 1 owns no token start at all, the
    workgroup after it starts inside the token.  Beyond a 64 KiB line, so outside RunSingle's
    parity domain, but inside this entry point's contract (any split bytes); the oracle defines them."""
    start = LONG_START
    if case == "workgroup":
        start, n = JS_WG - 144, JS_WG + 400
        token = _ascii_token(n, 7)
        assert start == 262000 and start + n > 2 * JS_WG and start < JS_WG
    elif case == "65535_cjk":
        token = "中".encode() * (65535 // 3)
        n = len(token)
        assert n % 3 == 0 and n == 65535
    else:
        n = int(case)
        token = _ascii_token(n, n)
    data = _long_input(start, token)
    assert data[start:start + n] == token and data[start - 1:start] == b" " and data[start + n:start + n + 1] == b" "
    toks = ob.tokens(data)
    assert toks.count(token) == 1 and max(len(t) for t in toks) == n
    check(eng, data, 2, f"long token {case}")


# ---------------------------------------------------------------- d. partition groups and the scan
GROUP_RS = [1, 2, 127, 128, 129, 256, 257, 1000, 1024]
CORPUS_BYTES = 5 * JS_WG - 1000 + 1777      # just past the fifth workgroup: W = 6, the last one nearly empty


@pytest.fixture(scope="module")
def corpus(built):
    from wcg.corpus import Generator
    data = Generator(1, 20_000, 1.0, 53).bytes(CORPUS_BYTES)
    return data, ob.tokens(data)


@pytest.mark.parametrize("R", GROUP_RS)
def test_partition_groups_and_scan(eng, corpus, R):
    data, toks = corpus
    W = -(-len(data) // JS_WG)
    assert W == 6 and len(data) > 5 * JS_WG - 1000
    want = files_of(toks, R)
    # from the expected files: every group of JS_PG partitions has work to do, and with R >= 1000
    # also a file that is empty or short (under half the mean size) next to the longer ones, so an
    # offset that belongs to another partition moves bytes
    mean = sum(len(f) for f in want) / R
    for pg in range(0, R, JS_PG):
        group = want[pg:pg + JS_PG]
        assert any(group), (R, pg)
        if R >= 1000:
            assert any(len(f) < mean / 2 for f in group), (R, pg)
    if R >= 1000:
        assert R * W > SCAN_ROUND
    if R == 1:
        assert want == [b"".join(_line(t) for t in toks)]       # every token, in input order
    assert_files(eng.map_json(data, R), want, f"corpus R={R}")


# ---------------------------------------------------------------- e. random bytes
def test_random_bytes(eng):
    rng = random.Random(99)
    pool = [b"a", b"Zq", b" ", b"\n", b"\x80", b"\xc3\xa9", b"\xe4\xb8\xad", b"\xf0\xa0\x80\x80", b"\xed\xa0\x80",
            b"\xc0", b"\xff", b"\xe0\xa0", b"\xcc\x81", b"\xc3", b"\x00", b"abcdefghijklmnopq",
            b"\xf4\x90\x80\x80", b"\xf0\x8f\xbf\xbf", b"\xef\xbf\xbd"]
    for i in range(30):
        n = rng.randrange(1, 50_001)
        out = bytearray()
        while len(out) < n:
            out += rng.choice(pool) if rng.random() < 0.8 else bytes([rng.randrange(256)])
        R = rng.randrange(1, 301)
        check(eng, bytes(out[:n]), R, f"random input {i} n={n} R={R}")


# ---------------------------------------------------------------- f. every Unicode scalar
def _scalars():
    return [cp for cp in range(0x80, 0x110000) if not (0xD800 <= cp <= 0xDFFF)]


@pytest.mark.parametrize("layout", ["separated", "runs"])
def test_every_unicode_scalar(eng, layout):
    """the layouts of test_gpu_scale.py::test_every_unicode_scalar: the whole letter table through
    letter_byte's look-back, continuation byte by continuation byte"""
    cps = _scalars()
    if layout == "separated":
        data = b" ".join(chr(cp).encode() for cp in cps) + b"\n"
    else:
        parts, i, k = [], 0, 0
        while i < len(cps):
            n = 1 + k % 7
            parts.append(b"a" * (k % 16) + "".join(chr(c) for c in cps[i:i + n]).encode() + b"\x80" * (k % 2) + b" ")
            i += n
            k += 1
        data = b"".join(parts) + b"\n"
    check(eng, data, 3, f"scalars {layout}")


# ---------------------------------------------------------------- g. call contract and state
def test_size_query_and_cap(eng, corpus):
    from wcg._lib import WCG_OK, WCG_EINVAL
    data = corpus[0][:300_000]
    R = 7
    want = expected(data, R)
    rc, sizes, _ = raw_call(eng, data, R, fill=False)             # host_out == NULL
    assert rc == WCG_OK and sizes == [len(f) for f in want]
    total = sum(sizes)
    rc, sizes2, _ = raw_call(eng, data, R, cap=total - 1)
    assert rc == WCG_EINVAL
    assert eng._lib.wcg_last_error(eng._ctx)
    rc, sizes3, raw = raw_call(eng, data, R, cap=total)
    assert rc == WCG_OK and sizes3 == sizes
    assert raw == b"".join(want)


def test_nreduce_limits(eng):
    from wcg._lib import WCG_OK, WCG_EINVAL
    data = b"the cat and the hat\nand the bat\n" * 40
    for R in (0, MAX_NREDUCE + 1):
        rc, _, _ = raw_call(eng, data, R, cap=1 << 16, nsizes=MAX_NREDUCE + 1)
        assert rc == WCG_EINVAL, R
    assert b"nreduce above 1024" in eng._lib.wcg_last_error(eng._ctx)
    rc, sizes, raw = raw_call(eng, data, MAX_NREDUCE)
    want = expected(data, MAX_NREDUCE)
    assert rc == WCG_OK and sizes == [len(f) for f in want] and raw == b"".join(want)


def test_buffer_reuse_across_calls(built, corpus):
    """one context, shrinking and growing inputs and R: the input, offset and output buffers and
    the per-call sizes of an earlier call leave nothing behind"""
    import wcg
    data = corpus[0]
    with wcg.Engine(0, 0, 1 << 16) as e:
        for d, R in ((data, 257), (b"one two\nza", 1), (b"", 5), (data, 64)):
            assert_files(e.map_json(d, R), files_of(corpus[1], R) if d is data else expected(d, R),
                         f"reuse n={len(d)} R={R}")


# ---------------------------------------------------------------- h. independence
@pytest.fixture(scope="module")
def abc(built):
    from wcg.corpus import Generator
    return [Generator(1, 3_000, 1.0, 61 + i).bytes(40_000 + 7_001 * i) + b"\n" for i in range(3)]


def test_independent_of_the_aggregation_tables(eng, abc):
    import wcg
    A, B, C = abc
    eng.reset()
    eng.map_host(A)
    check(eng, B, 5, "between two map calls")
    eng.map_host(C)
    eng.reduce()
    ref = ob.Result(A + C)
    merged = ref.merged()
    ob.assert_same(eng.result(), merged)
    words = [b"the", b"", b"zzzz", b"\x00\xff"] + sorted(set(ob.tokens(A)))[:50] + sorted(set(ob.tokens(B)))[:50]

    def views():
        return eng.partitions(3), eng.top(10), eng.lookup(words), eng.result()
    before = views()
    assert before[0] == [ref.res(3, r) for r in range(3)]
    assert before[1] == wcg.top_of_merged(merged, 10)
    assert before[2] == wcg.lookup_in_merged(merged, words)
    check(eng, B, 200, "after the reduce")
    assert views() == before


def test_pending_async_job_survives(eng, abc):
    """wcg_map_json between wcg_reduce_async and wcg_reduce_wait: include/wcg.h lists the calls
    that drop a pending job (wcg_reset, wcg_map, wcg_map_device, wcg_map_file, wcg_import) and
    says that wcg_map_json is not one of them; reduce_wait returns the job's sizes and result.  The
    job is a context's second or later one, so it takes the one-launch reduce and really is pending."""
    A, B, C = abc
    eng.reset()
    eng.map_host(C)
    eng.reduce()                                   # an earlier job: the next one is eligible
    eng.reset()
    eng.map_host(A)
    eng.reduce_async()
    check(eng, B, 5, "behind a pending job")
    nk, nb = eng.reduce_wait()
    want = ob.merged(A)
    assert eng.reduce_path() == 1
    assert nk == want.count(b"\n") and nb == len(want)
    ob.assert_same(eng.result(), want)
