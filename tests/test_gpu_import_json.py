"""wcg_import_json on the MI355X: DoMap's per-occurrence JSON intermediates (MAP) and DoReduce's
-res files (RES) decoded on the device into the aggregation tables (csrc/wcg_import_json.h).

Expected values come from the host: wc_ref.res_file / merged_output over wc_ref.word_count, the C
oracle's merged file (ob.merged), jv.parse of the files themselves, and the hand-written
(line, rule) pairs of tests/json_vectors.py for the files that must be refused.
"""
import ctypes
import os

import pytest

from tests import json_vectors as jv
from tests import oracle_bridge as ob
from tests import wire

pytestmark = pytest.mark.gpu

wc_ref = jv.wc_ref
MAP, RES = jv.MAP, jv.RES
WCG_EINVAL, WCG_ESTATE = 1, 5
EDGE_LENGTHS = [1, 7, 8, 9, 15, 16, 17, 24, 25, 32, 33, 48, 49, 70_000]
EDGE_COUNTS = [1, 9, 10, 2 ** 32, 10 ** 19, 2 ** 64 - 1]


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


@pytest.fixture(scope="module")
def text(built):
    """a few hundred KB of mixed UTF-8 text, its two map splits and its counts (made once)"""
    from wcg.corpus import Generator, UTF8
    data = Generator(UTF8, 20_000, 1.0, 11).bytes(300 << 10)
    cut = len(data) // 2
    while not (data[cut] < 0x80 and not chr(data[cut]).isalpha()):
        cut += 1                                    # after an ASCII non-letter: no token straddles
    halves = [data[:cut + 1], data[cut + 1:]]
    counts = wc_ref.word_count(data)
    assert wire.add(*[wc_ref.word_count(h) for h in halves]) == counts
    assert any(len(k) > 15 for k in counts) and any(max(k) >= 0xF0 for k in counts)
    return data, halves, counts


def refused(call):
    import wcg
    with pytest.raises(wcg.WcgError) as ei:
        call()
    return ei.value.status, str(ei.value)


def double(counts, times=2):
    return {k: times * v for k, v in counts.items()}


def pad_to(nbytes, tag=0):
    """accepted lines of exactly nbytes bytes (0, or at least 24)"""
    assert nbytes == 0 or nbytes >= 24
    out, left = [], nbytes
    while left >= 24 + 33:
        out.append(jv.ln(b"pad" + wire.letters((tag + len(out)) % 2704, 2) + b"xxxxx"))
        left -= 33
    if left:
        out.append(jv.ln(b"p" * (left - 23)))
    data = b"".join(out)
    assert len(data) == nbytes
    return data


def with_value(data, mode, i, wide=True):
    """MAP files keep their "1"; RES files get counts of every width (wide), or of one digit: the
    lines keep their lengths"""
    if mode == MAP:
        return data
    lines = data.split(b"\n")[:-1]
    return b"".join(l[:-3] + str(wire.count_of_width(1 + (i + j) % 20 if wide else 1, j)).encode() + b'"}\n'
                    for j, l in enumerate(lines))


# ---------------------------------------------------------------- 1. MAP parity
@pytest.mark.parametrize("R", [1, 3])
def test_map_parity(engine, text, R):
    data, halves, counts = text
    eng = engine()
    parts = [eng.map_json(h, R) for h in halves]               # [map job][partition]
    for m, h in enumerate(halves):
        assert [bytes(p) for p in wc_ref.map_files(h, R)] == parts[m]
    for r in range(R):
        eng.reset()
        for m in range(2):
            assert eng.import_json(parts[m][r], MAP) == parts[m][r].count(b"\n")
        eng.reduce()
        ob.assert_same(eng.partition(1, 0), wc_ref.res_file(counts, R, r))
    eng.reset()
    for m in range(2):
        for r in range(R):
            eng.import_json(parts[m][r], MAP)
    assert eng.reduce()[0] == len(counts)
    ob.assert_same(eng.result(), ob.merged(data))


# ---------------------------------------------------------------- 2. RES parity
def test_res_parity(engine, text):
    data, halves, counts = text
    a, b = engine(), engine()
    a.map_host(data)
    a.reduce()
    merged = a.result()
    parts = a.partitions(3)
    assert parts == [wc_ref.res_file(counts, 3, r) for r in range(3)]
    for p in parts:
        assert b.import_json(p, RES) == p.count(b"\n")
    assert b.reduce() == (len(counts), len(merged))
    ob.assert_same(b.result(), merged)
    # one file twice: its counts double
    b.reset()
    b.import_json(parts[1], RES)
    b.import_json(parts[1], RES)
    b.reduce()
    ob.assert_same(b.result(), wire.expect(double(jv.parse(parts[1], RES))))
    # onto a table map_host filled: the counts add
    b.reset()
    b.map_host(halves[0])
    for p in parts:
        b.import_json(p, RES)
    b.map_host(halves[1])
    b.reduce()
    ob.assert_same(b.result(), wire.expect(double(counts)))


# ---------------------------------------------------------------- 3. edges
def edge_counts():
    counts = {"é".encode(): 3, "中".encode(): 4, "𝒳".encode(): 5, "é中𝒳".encode(): 6}
    for i, L in enumerate(EDGE_LENGTHS):
        for j in (0, 1) if L > 1 else (40, 41):
            counts[wire.key_of(i * 2 + j, L)] = EDGE_COUNTS[(i + j) % len(EDGE_COUNTS)]
    assert set(EDGE_LENGTHS) <= {len(k) for k in counts} and set(EDGE_COUNTS) <= set(counts.values())
    return counts


def test_edge_keys_and_counts(engine):
    counts = edge_counts()
    eng = engine()
    keys = sorted(counts, key=lambda k: (wc_ref.ihash(k), k))       # no particular order
    res = b"".join(jv.ln(k, str(counts[k]).encode()) for k in keys)
    assert jv.check_json(res, RES) is None
    assert eng.import_json(res, RES) == len(keys)
    eng.reduce()
    ob.assert_same(eng.result(), wire.expect(counts))
    ob.assert_same(eng.partition(1, 0), wire.expect_res(counts, 1, 0))
    # MAP: every key 1 + (its length % 3) times, interleaved
    times = {k: 1 + len(k) % 3 for k in keys}
    mp = b"".join(jv.ln(k) for rep in range(3) for k in keys if times[k] > rep)
    assert jv.check_json(mp, MAP) is None
    eng.reset()
    assert eng.import_json(mp, MAP) == sum(times.values())
    eng.reduce()
    ob.assert_same(eng.result(), wire.expect(times))


@pytest.mark.parametrize("mode", [MAP, RES])
def test_sweep_over_the_tile_boundary(engine, mode):
    T = jv.tile()
    eng = engine()
    want = {}
    i = 0
    for off in range(T - 40, T + 41):
        target = with_value(jv.ln(wire.key_of(i, 2 + i % 37)), mode, i)     # RES: 1 .. 20 digits
        # the line's first byte at offset off, lines after it; then its '\n' at offset off as the
        # file's last byte (off >= T: the file's last tile holds off - T + 1 bytes)
        pad = lambda n, tag: with_value(pad_to(n, tag), mode, tag, wide=False)
        for f in (pad(off, i) + target + pad(70, i + 1), pad(off + 1 - len(target), i + 2) + target):
            assert f[-1:] == b"\n" and jv.check_json(f, mode) is None
            assert f.index(target) in (off, off + 1 - len(target))
            assert eng.import_json(f, mode) == f.count(b"\n"), off
            want = wire.add(want, jv.parse(f, mode))
            i += 1
    # the same in the third tile of a file, the last one
    for off in (2 * T - 1, 2 * T, 2 * T + 1, 2 * T + 23):
        f = with_value(pad_to(off + 1 - 40, i) + jv.ln(b"q" * 17), mode, i, wide=False)
        assert len(f) == off + 1
        assert eng.import_json(f, mode) == f.count(b"\n")
        want = wire.add(want, jv.parse(f, mode))
        i += 1
    want = {k: v % 2 ** 64 for k, v in want.items()}               # counts add as unsigned 64-bit
    eng.reduce()
    ob.assert_same(eng.result(), wire.expect(want))


@pytest.mark.parametrize("mode", [MAP, RES])
def test_one_line_and_lines_that_end_in_the_second_tile(engine, mode):
    T = jv.tile()
    eng = engine()
    v = b"1" if mode == MAP else b"18446744073709551615"
    assert eng.import_json(jv.ln(b"solo", v), mode) == 1
    eng.reduce()
    ob.assert_same(eng.result(), b"solo: " + v + b"\n")
    # the first line's key fills the first tile: no line ends there
    eng.reset()
    big = wire.filler(T)
    f = with_value(jv.ln(big) + jv.ln(b"after") + jv.ln(wire.filler(T // 2, 5)) + jv.ln(b"z"), mode, 3)
    assert T <= f.index(b"\n") and len(f) <= 2 * T and jv.check_json(f, mode) is None
    assert eng.import_json(f, mode) == 4
    eng.reduce()
    ob.assert_same(eng.result(), wire.expect(jv.parse(f, mode)))


# ---------------------------------------------------------------- 4. refusals
def message(line, rule):
    return "newline" if rule == "newline" else f"wcg_import_json: line {line}: {rule}"


def test_every_vector_is_refused_and_changes_nothing(engine, text):
    data, halves, counts = text
    eng = engine()
    eng.map_host(halves[0])
    nk, nb = eng.reduce()
    base = eng.result()
    top = eng.top(10)
    for name, f, mode, line, rule in jv.VECTORS:
        status, msg = refused(lambda: eng.import_json(f, mode))
        assert status == WCG_EINVAL, name
        assert message(line, rule) in msg, (name, msg)
        if rule != "newline":
            assert msg.endswith(message(line, rule)), (name, msg)
        assert eng.top(10) == top, name                            # the last result and its caches
        assert eng.result() == base, name
        assert eng.reduce() == (nk, nb), name                      # the tables
        assert eng.result() == base, name


def test_refusal_keeps_a_pending_job_and_the_device_form_refuses_alike(engine, text):
    import torch
    data, halves, counts = text
    eng = engine()
    eng.map_host(halves[0])
    nk, nb = eng.reduce()
    base = eng.result()
    for name, f, mode, line, rule in jv.VECTORS[:3] + jv.VECTORS[-4:]:
        eng.reset()
        eng.map_host(halves[0])
        eng.reduce_async()
        status, msg = refused(lambda: eng.import_json(f, mode))
        assert status == WCG_EINVAL and message(line, rule) in msg, (name, msg)
        t = torch.frombuffer(bytearray(f), dtype=torch.uint8).to("cuda")
        torch.cuda.synchronize()
        status, msg = refused(lambda: eng.import_json_device(t.data_ptr(), len(f), mode))
        assert status == WCG_EINVAL and message(line, rule) in msg, (name, msg)
        assert eng.reduce_wait() == (nk, nb), name
        assert eng.result() == base, name


# ---------------------------------------------------------------- 5. state and arguments
def test_state_and_arguments(engine, text):
    import torch
    import wcg
    data, halves, counts = text
    eng = engine()
    lib = wcg.load()
    eng.map_host(halves[0])
    eng.reduce()
    base = eng.result()
    nl = ctypes.c_uint64(99)
    # n == 0 touches nothing, whatever the pointer
    assert eng.import_json(b"", MAP) == 0 and eng.import_json(b"", RES) == 0
    assert lib.wcg_import_json(eng._ctx, b"x", 0, RES, ctypes.byref(nl)) == 0
    assert lib.wcg_import_json_device(eng._ctx, None, 0, MAP, ctypes.byref(nl)) == 0
    assert eng.result() == base and eng.lookup([b"zzzznotaword"]) == [0]
    # a NULL pointer, a bad mode
    assert lib.wcg_import_json(eng._ctx, None, 5, MAP, ctypes.byref(nl)) == WCG_EINVAL
    assert lib.wcg_import_json_device(eng._ctx, None, 5, RES, ctypes.byref(nl)) == WCG_EINVAL
    good = jv.ln(b"abc")
    for mode in (2, -1):
        assert refused(lambda: eng.import_json(good, mode))[0] == WCG_EINVAL
        assert lib.wcg_import_json_device(eng._ctx, None, 5, mode, ctypes.byref(nl)) == WCG_EINVAL
    assert eng.result() == base
    # an accepted import drops the result, as wcg_import does
    assert eng.import_json(good, MAP) == 1
    for q in (lambda: eng.top(10), lambda: eng.lookup([b"abc"]), lambda: eng.range(), lambda: eng.partition(1, 0),
              lambda: eng.result()):
        assert refused(q)[0] == WCG_ESTATE
    eng.reduce()
    ob.assert_same(eng.result(), wire.expect(wire.add(wc_ref.word_count(halves[0]), {b"abc": 1})))
    # ... and a pending job
    eng.reset()
    eng.map_host(halves[0])
    eng.reduce_async()
    eng.import_json(good, RES)
    eng.reduce()
    ob.assert_same(eng.result(), wire.expect(wire.add(wc_ref.word_count(halves[0]), {b"abc": 1})))

    # the device form equals the host form; calls of different sizes on one context reuse buffers
    a = engine()
    parts = a.map_json(data, 2)
    res = [wc_ref.res_file(counts, 2, r) for r in range(2)]
    for mode, files in ((MAP, [parts[0], good, parts[1]]), (RES, [res[0], jv.ln(b"abc", b"7"), res[1], res[0][:res[0].index(b"\n") + 1]])):
        got = []
        for dev in (False, True):
            eng.reset()
            for f in files:
                if dev:
                    t = torch.frombuffer(bytearray(b"\n" + f), dtype=torch.uint8).to("cuda")[1:]   # an odd address
                    torch.cuda.synchronize()
                    assert eng.import_json_device(t.data_ptr(), len(f), mode) == f.count(b"\n")
                else:
                    assert eng.import_json(f, mode) == f.count(b"\n")
            eng.reduce()
            got.append(eng.result())
        want = {}
        for f in files:
            want = wire.add(want, jv.parse(f, mode))
        ob.assert_same(got[0], wire.expect(want))
        ob.assert_same(got[1], got[0])


# ---------------------------------------------------------------- 6. mr.do_reduce and mr.merge_gpu
class Spy:
    """an engine that notes which calls took the data"""

    def __init__(self, eng):
        self._e, self.calls = eng, []

    def __getattr__(self, name):
        f = getattr(self._e, name)
        if name not in ("import_json", "map_host", "import_host"):
            return f

        def g(*a):
            self.calls.append(name)
            return f(*a)
        return g


def test_do_reduce_and_merge_gpu(engine, text, tmp_path):
    from wcg import mr
    data, halves, counts = text
    wd, fname, R = str(tmp_path), "in.txt", 2
    files = {}
    for m, h in enumerate(halves):
        for r, p in enumerate(wc_ref.map_files(h, R)):
            files[m, r] = bytes(p)
            open(os.path.join(wd, mr.reduce_name(fname, m, r)), "wb").write(files[m, r])
    eng = Spy(engine())
    for r in range(R):
        mr.do_reduce(eng, r, wd, fname, 2)
        ob.assert_same(open(os.path.join(wd, mr.merge_name(fname, r)), "rb").read(), wc_ref.res_file(counts, R, r))
    assert eng.calls == ["import_json"] * 4
    # the merge of those files, on the GPU and on the host
    gpu = mr.merge_gpu(eng, wd, fname, R)
    assert open(os.path.join(wd, "mrtmp." + fname), "rb").read() == gpu
    ob.assert_same(gpu, mr.merge(wd, fname, R))
    ob.assert_same(gpu, wc_ref.merged_output(counts))
    # a truncated last line: the GPU refuses the file, the host decode takes it up to that line
    cut = files[1, 0][:-9]
    open(os.path.join(wd, mr.reduce_name(fname, 1, 0)), "wb").write(cut)
    eng.calls.clear()
    mr.do_reduce(eng, 0, wd, fname, 2)
    assert eng.calls == ["import_json", "import_json", "map_host"]
    host = wc_ref.word_count(mr._json_keys(files[0, 0]) + mr._json_keys(cut))
    assert sum(host.values()) == files[0, 0].count(b"\n") + cut.count(b"\n")
    ob.assert_same(open(os.path.join(wd, mr.merge_name(fname, 0)), "rb").read(), wc_ref.res_file(host, 1, 0))
