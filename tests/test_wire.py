"""tests/wire.py and the reference it hands the crafted GPU tests (tests/test_gpu_crafted.py), on
the CPU: the units decode back to the dict they were made from (counts up to 2^64 - 1, every key
length class, shuffled, split), and oracle/wc_ref.py's merged file and -res-<r> files agree with
"%s: %d\\n" / JSON lines formatted here independently."""
import random
import struct

import pytest

from tests import wire
from tests.oracle_bridge import wc_ref


def crafted_sets():
    edge = wire.edge_count_keys()
    ordered = dict(zip(wire.ordered_keys(300, 10), (wire.WIDTH_COUNTS[i % 20] for i in range(300))))
    ones = {b"\xff" * 16: 7, b"\xff" * 16 + b"a": 2 ** 64 - 1, b"\xff" * 17 + b"zz" * 20: 10 ** 19}
    tiny = {b"a": 1, b"b" * 15: 2 ** 64 - 1, b"c" * 16: 2 ** 32, "中".encode() * 11: 2 ** 63}
    return {"edge": edge, "ordered": ordered, "all-ones": ones, "tiny": tiny}


SETS = crafted_sets()


def test_edge_counts_cover_every_width_and_branch():
    widths = {len(str(c)) for c in wire.EDGE_COUNTS}
    assert widths == set(range(1, 21))
    for k in range(1, 20):
        assert {10 ** k - 1, 10 ** k, 10 ** k + 1} <= set(wire.EDGE_COUNTS)
    assert {2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1} <= set(wire.EDGE_COUNTS)
    assert len(wire.EDGE_COUNTS) == 62 and max(wire.EDGE_COUNTS) == wire.U64_MAX and min(wire.EDGE_COUNTS) >= 1
    assert [len(str(c)) for c in wire.WIDTH_COUNTS] == list(range(1, 21))


def test_edge_keys_cover_every_length_class():
    c = wire.edge_count_keys()
    assert len(c) == 4 * len(wire.EDGE_COUNTS)
    lens = {len(k) for k in c}
    assert {7, 8, 15, 16, 17, 32, 33} <= lens and min(lens) == 1 and max(lens) >= 100
    for lo, hi in ((1, 7), (8, 15), (16, 32), (33, 1 << 20)):
        assert sorted(v for k, v in c.items() if lo <= len(k) <= hi) == wire.EDGE_COUNTS
    for k in c:                                     # letters only: a token of the map would be the same key
        assert wc_ref.tokens(k) == [k], k


def test_ordered_keys_sort_as_built():
    ks = wire.ordered_keys(3000, 10) + wire.ordered_keys(50, 10, first=3000)
    assert ks == sorted(ks) and len(set(ks)) == len(ks) and {len(k) for k in ks} == {10}
    assert all(wc_ref.tokens(k) == [k] for k in ks[:100])


@pytest.mark.parametrize("name", sorted(SETS))
def test_units_decode_back(name):
    c = SETS[name]
    blob = wire.units(c)
    assert len(blob) % wire.UNIT == 0
    assert dict(wire.decode(blob)) == c
    assert [k for k, _ in wire.decode(blob)] == list(c)             # seed None: the dict's order
    for seed in (0, 1, 2):
        sh = wire.units(c, seed=seed)
        assert len(sh) == len(blob) and dict(wire.decode(sh)) == c
    assert len(c) < 20 or len({wire.units(c, seed=s) for s in (0, 1, 2)} | {blob}) == 4


def test_unit_layout():
    """the bytes themselves (include/wcg.h), not only the round trip"""
    u = wire.encode(b"ab", 2 ** 64 - 1)
    assert u == bytes([0, 0, 0, 0, 0, 0, 0x62, 0x61]) + b"\0" * 8 + b"\xff" * 8 + struct.pack("<Q", 2)
    key = bytes(range(0x41, 0x41 + 26)) + b"abc"                   # 29 bytes: header + 2 continuations
    u = wire.encode(key, 5)
    assert len(u) == 96
    hi, lo, cnt, ref = struct.unpack_from("<QQQQ", u, 0)
    assert struct.pack(">QQ", hi, lo) == key[:16] and cnt == 5 and ref == wire.LONG_FLAG | 29 << 40
    assert u[32:56] == key[:24] and u[64:69] == key[24:] and u[69:88] == b"\0" * 19
    assert struct.unpack_from("<Q", u, 56)[0] == wire.CONT_MARK == struct.unpack_from("<Q", u, 88)[0]
    assert len(wire.encode(b"k" * 15, 1)) == 32 and len(wire.encode(b"k" * 16, 1)) == 64
    assert len(wire.encode(b"k" * 24, 1)) == 64 and len(wire.encode(b"k" * 25, 1)) == 96


def test_split_units_sum_back():
    c = SETS["edge"]
    big = [k for k in c if c[k] >= 64]
    split = {k: (2, 3, 64)[i % 3] for i, k in enumerate(big)}
    blob = wire.units(c, seed=5, split=split)
    pairs = list(wire.decode(blob))
    assert len(pairs) == len(c) + sum(n - 1 for n in split.values())
    assert all(1 <= v <= wire.U64_MAX for _, v in pairs)
    assert wire.decode_counts(blob) == c
    rnd = random.Random(3)
    for cnt, parts in ((2, 2), (64, 64), (2 ** 64 - 1, 64), (2 ** 32, 3), (10 ** 10, 2)):
        p = wire.split_count(cnt, parts, rnd)
        assert len(p) == parts and sum(p) == cnt and min(p) >= 1


def test_add_is_the_dict_sum():
    a, b = {b"x": 2 ** 32 - 1, b"y": 5}, {b"x": 1, b"z": 9}
    assert wire.add(a, b) == {b"x": 2 ** 32, b"y": 5, b"z": 9}
    assert a == {b"x": 2 ** 32 - 1, b"y": 5}


@pytest.mark.parametrize("name", sorted(SETS))
def test_reference_formats_independently(name):
    c = SETS[name]
    want = b"".join(b"%s: %d\n" % (k, c[k]) for k in sorted(c))
    assert wire.expect(c) == want == wc_ref.merged_output(c) == b"".join(wire.lines(c))
    assert want.count(b"\n") == len(c)
    for R in (1, 3, 64):
        files = [wire.expect_res(c, R, r) for r in range(R)]
        for r, f in enumerate(files):
            ks = sorted(k for k in c if wc_ref.ihash(k) % R == r)
            assert f == b"".join(b'{"Key":"%s","Value":"%d"}\n' % (k, c[k]) for k in ks) == wc_ref.res_file(c, R, r)
        assert sum(f.count(b"\n") for f in files) == len(c)


def test_reference_matches_the_c_oracle_on_text(built):
    """the dict reference and the C oracle agree where both apply: a text's counts"""
    from tests import oracle_bridge as ob
    ks = list(SETS["edge"])[::5] + wire.ordered_keys(40, 12)
    rnd = random.Random(11)
    text = b" ".join(rnd.choice(ks) for _ in range(3000)) + b"\n"
    c = wc_ref.word_count(text)
    assert wire.expect(c) == ob.merged(text)
    ref = ob.Result(text)
    for r in range(3):
        assert wire.expect_res(c, 3, r) == ref.res(3, r)
