"""The inputs of tests/test_gpu_capacity.py, checked without a GPU: a builder that stops producing
the distinct keys it promises, or grows past the bytes a pigeonhole bound allows, would let the GPU
tests pass with no buffer filled.  The C oracle counts the keys; the bounds are arithmetic."""
import pytest

from tests import oracle_bridge as ob
from tests import test_gpu_capacity as cap


@pytest.mark.parametrize("name", sorted(cap.BUILD))
def test_builders_make_the_promised_keys(built, name):
    calls = cap.corpus(name)
    for c, (d_inline, d_long) in zip(calls, cap.DISTINCT[name]):
        assert 0 < len(c) <= 8 << 20                                # the engines' max_input_bytes
        r = ob.Result(c)
        assert r.nkeys == d_inline + d_long
        keys = [l.rsplit(b": ", 1)[0] for l in r.merged().splitlines()]
        assert sum(1 for k in keys if len(k) >= 16) == d_long
        assert all(3 <= len(k) <= 15 or 16 <= len(k) <= 80 for k in keys)
    assert len(calls) == len(cap.DISTINCT[name])
    w = cap.want(name)
    assert w.nkeys == cap.JOB_KEYS[name]
    assert w.ntokens == sum(ob.Result(c).ntokens for c in calls)    # calls end with a separator


def test_inline_text_has_units_of_every_kind():
    keys = cap.inline_keys(26, 1)
    assert sorted({len(k) for k in keys}) == list(range(3, 16)) and len(set(keys)) == 26
    text = cap.inline_text_of(keys, 1, 13, 5)
    toks = text.split()
    assert len(toks) == 26 + 13 * 5 and set(toks) == set(keys)
    seps = bytes(c for c in text if c in b" \n")
    assert seps == bytes(32 if i & 1 else 10 for i in range(len(toks)))     # alternating


def test_long_keys_have_the_edge_lengths():
    keys = cap.long_keys(20_000, 7)
    assert len(set(keys)) == 20_000
    lens = {len(k) for k in keys}
    assert min(lens) == 16 and max(lens) == 80 and {16, 32, 33} <= lens
    shared = {}
    for k in keys:
        if len(k) > 32:
            shared.setdefault(k[:32], []).append(k)
    assert sum(len(v) for v in shared.values() if len(v) >= 2) >= 20_000 // 3   # a third share 32 bytes
    assert any(max(k) >= 0x80 for k in keys)                                    # some UTF-8


@pytest.mark.parametrize("name,P,R", cap.REGION_BOUNDS)
def test_region_bounds_hold(name, P, R):
    assert cap.regions_overfull(name, P, R)
    for c, (d, _) in zip(cap.corpus(name), cap.DISTINCT[name]):
        print(name, len(c), cap.map_groups(len(c)), cap.map_groups(len(c)) * P * R, d)


@pytest.mark.parametrize("name,entries", cap.PART_BOUNDS)
def test_partition_bounds_hold(name, entries):
    assert cap.partitions_overfull(name, entries)


def test_map_groups():
    assert [cap.map_groups(n) for n in (1, 992, 993, 992 * 16, 992 * 16 + 1)] == [1, 1, 1, 1, 2]
