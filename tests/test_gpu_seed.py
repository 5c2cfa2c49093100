"""GPU: k_map's LDS key tables seeded from the previous job's most frequent keys (wcg_seed.h,
DESIGN.md section 22).

A context that has reduced a one-pass job keeps a placed image of that job's top inline keys; its
later one-pass map calls launch k_map<MAP_SEEDED, true>, which copies the image into LDS instead of
zeroing the key words.  A seed is a hint: every job here is compared byte for byte with the C
oracle, whatever seed its context held, and the hit rates (lds_hits / tokens) and wcg_seed_stats
show which path a job took.

  * repeats: jobs 2 and 3 over job 1's text are seeded and hit more often; reduce_path() is what it
    is without seeds (WCG_SEED=0 on a second engine: nothing is built, no job is seeded);
  * a stale seed: vocabulary A, then a disjoint B of the same size and distribution - B's job is
    exact, holds no A key, hits less often than A's unseeded job and drops the seed; the next B job
    runs unseeded (above the stale job's rate) and builds the seed the fourth job uses;
  * seed keys at the tables' edges: 1- and 7-byte keys, 8- and 15-byte keys, a key whose two slot
    choices are both taken by more frequent seed keys (slots restated here from wcg_lds_table.h),
    fewer keys than SEED_FRAC x slots, exactly one key;
  * two map calls before one reduce, seeded; a two-pass context (never seeded); two contexts on
    two streams, each with its own seed; a stale seed with miss-log regions of 16 units
    (WCG_REGION_CAP, as tests/test_gpu_capacity.py: the full-region branch, global_ops > 0).

Inputs are a few MiB at the most: a map workgroup sees some tens of KiB, so the unseeded tables are
cold for most of a job and the seeded rates lie far above them.
"""
import os
import random

import pytest

from tests import oracle_bridge as ob

pytestmark = pytest.mark.gpu

NS, NM = 8410, 1024             # k_map's short and medium slots (wcg_map.h)
ABC = b"abcdefghijklmnopqrstuvwxyz"
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------- the kernel's slots
def rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def lds_hash32(a, b, c, d):
    x = a ^ rotl(b, 9) ^ rotl(c, 17) ^ rotl(d, 25)
    x ^= x >> 15
    x = x * 0x2C1B3C6D & M32
    return x ^ (x >> 12)


def short_slots(key):
    """MapTable::slots of a short key (<= 7 bytes): k0 = its bytes | len << 56"""
    assert 1 <= len(key) <= 7
    k0 = int.from_bytes(key, "little") | len(key) << 56
    h = lds_hash32(k0 & M32, k0 >> 32, 0, 0)
    return ((h >> 8) * (NS << 8)) >> 32, ((h & 0xFFFFFF) * (NS << 8)) >> 32


# ------------------------------------------------------------------------------- texts
def word(i, n, first):
    """the i-th word of n letters that starts with `first` (distinct for i < 26 ** (n - 1))"""
    out = bytearray(first)
    for _ in range(n - 1):
        out.append(ABC[i % 26])
        i //= 26
    return bytes(out)


def vocab(first, size, lengths):
    return [word(i // len(lengths), lengths[i % len(lengths)], first) for i in range(size)]


def zipf_text(words, ntok, seed):
    """ntok tokens, word r with weight 1 / (r + 1); the same draws for any `words` of one size"""
    rnd = random.Random(seed)
    idx = rnd.choices(range(len(words)), weights=[1.0 / (r + 1) for r in range(len(words))], k=ntok)
    return b"".join(words[i] + (b" " if j & 7 else b"\n") for j, i in enumerate(idx))


def run(e, *texts):
    """one job: reset, a map call per text, reduce -> the facts the tests compare"""
    e.reset()
    for t in texts:
        e.map_host(t)
    e.reduce()
    got, path, st, sd = e.result(), e.reduce_path(), e.stats(), e.seed_stats()
    return {"out": got, "path": path, "rate": st["lds_hits"] / max(1, st["tokens"]), "stats": st, "seed": sd}


def engine(keys=1 << 20, cap=8 << 20):
    import wcg
    return wcg.Engine(device=0, max_input_bytes=cap, max_keys=keys)


@pytest.fixture
def seed_env():
    """WCG_SEED and WCG_REGION_CAP as a test sets them (read by the library on every call), restored"""
    old = {k: os.environ.get(k) for k in ("WCG_SEED", "WCG_REGION_CAP")}
    yield os.environ
    for k, v in old.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


@pytest.fixture(scope="module")
def c2_text(built):
    from wcg.corpus import Generator
    data = Generator(0, 100_000, 1.0, 42).bytes(4 << 20)
    return data, ob.merged(data, 16)


@pytest.fixture(scope="module")
def ab_texts(built):
    """vocabularies A and B: 20 000 words each, lengths 3..12, no word in common, the same draws"""
    lengths = (3, 4, 5, 6, 7, 5, 6, 9, 12, 4)
    a, b = vocab(b"a", 20_000, lengths), vocab(b"b", 20_000, lengths)
    ta, tb = zipf_text(a, 600_000, 7), zipf_text(b, 600_000, 7)
    return (ta, ob.merged(ta, 16)), (tb, ob.merged(tb, 16))


# ------------------------------------------------------------------------------- tests
def test_repeat_jobs_are_seeded(c2_text, seed_env):
    data, want = c2_text
    seed_env.pop("WCG_SEED", None)
    with engine() as e:
        jobs = [run(e, data) for _ in range(3)]
    seed_env["WCG_SEED"] = "0"
    with engine() as e:
        plain = [run(e, data) for _ in range(3)]
    for j in jobs + plain:
        ob.assert_same(j["out"], want)
    print("seeded rates", [round(j["rate"], 4) for j in jobs], "unseeded", [round(j["rate"], 4) for j in plain])
    assert [j["seed"]["last_job_seeded"] for j in jobs] == [False, True, True]
    assert [j["seed"]["builds"] for j in jobs] == [1, 1, 1]
    assert all(j["seed"]["valid"] for j in jobs)
    assert jobs[1]["rate"] > jobs[0]["rate"] and jobs[2]["rate"] > jobs[0]["rate"]
    # WCG_SEED=0: nothing built, nothing seeded, and the same reduce paths
    assert all(not j["seed"]["valid"] and j["seed"]["builds"] == 0 and not j["seed"]["last_job_seeded"] for j in plain)
    assert [j["path"] for j in jobs] == [j["path"] for j in plain]


def test_stale_seed_is_dropped_and_rebuilt(ab_texts, seed_env):
    (ta, wa), (tb, wb) = ab_texts
    seed_env.pop("WCG_SEED", None)
    with engine() as e:
        j1, j2, j3, j4 = run(e, ta), run(e, tb), run(e, tb), run(e, tb)
    ob.assert_same(j1["out"], wa)
    for j in (j2, j3, j4):
        ob.assert_same(j["out"], wb)
    assert not any(line.startswith(b"a") for line in j2["out"].splitlines())    # no A key in B's job
    print("rates A, B stale, B unseeded, B seeded:", [round(j["rate"], 4) for j in (j1, j2, j3, j4)])
    assert j2["seed"]["last_job_seeded"] and j2["rate"] < j1["rate"]
    assert not j2["seed"]["valid"]                                  # dropped
    assert not j3["seed"]["last_job_seeded"] and j3["seed"]["valid"] and j3["seed"]["builds"] == 2
    assert j3["rate"] > j2["rate"]                                  # back above the stale job's
    assert j4["seed"]["last_job_seeded"] and j4["seed"]["valid"] and j4["seed"]["builds"] == 2
    assert j4["rate"] > j3["rate"]


def colliding_keys():
    """three 5-byte keys: both slot choices of the third are the first choices of the other two"""
    first = {}
    ws = [word(i, 5, b"c") for i in range(40_000)]
    for w in ws:
        first.setdefault(short_slots(w)[0], w)
    for w in ws:
        s1, s2 = short_slots(w)
        k1, k2 = first.get(s1), first.get(s2)
        if k1 and k2 and s1 != s2 and w not in (k1, k2):
            return k1, k2, w
    raise AssertionError("no colliding keys among 40 000 words")


def edge_text(case):
    rnd = random.Random(11)
    if case == "short_1_7":
        words = [bytes((c,)) for c in ABC] + vocab(b"s", 3000, (7,))
    elif case == "medium_8_15":
        words = vocab(b"m", 1500, (8,)) + vocab(b"n", 1500, (15,))
    elif case == "collide":
        k1, k2, k3 = colliding_keys()
        words = [k1] * 40 + [k2] * 40 + [k3] * 10 + vocab(b"d", 200, (4, 6))      # ~8300, ~8300, ~2100, ~200 each: k1, k2 first
    elif case == "few_keys":
        words = vocab(b"f", 500, (2, 5, 7, 8, 11, 15))
    else:
        assert case == "one_key"
        words = [b"solitary"]
    toks = [rnd.choice(words) for _ in range(60_000)]
    return b"".join(t + (b" " if j % 5 else b"\n") for j, t in enumerate(toks))


@pytest.mark.parametrize("case", ["short_1_7", "medium_8_15", "collide", "few_keys", "one_key"])
def test_seed_keys_at_the_tables_edges(built, seed_env, case):
    seed_env.pop("WCG_SEED", None)
    text = edge_text(case)
    want = ob.merged(text, 16)
    with engine() as e:
        j1, j2 = run(e, text), run(e, text)
    ob.assert_same(j1["out"], want)
    ob.assert_same(j2["out"], want)
    print(case, "rates", round(j1["rate"], 4), round(j2["rate"], 4))
    assert not j1["seed"]["last_job_seeded"] and j2["seed"]["last_job_seeded"]
    assert j2["rate"] >= j1["rate"]


def test_two_map_calls_seeded(c2_text, seed_env):
    data, want = c2_text
    seed_env.pop("WCG_SEED", None)
    cut = data.rfind(b"\n", 0, len(data) // 3) + 1                  # between two tokens
    with engine() as e:
        j1 = run(e, data)
        j2 = run(e, data[:cut], data[cut:])
    ob.assert_same(j1["out"], want)
    ob.assert_same(j2["out"], want)
    assert j2["seed"]["last_job_seeded"] and j2["rate"] > j1["rate"]


def test_two_pass_context_is_never_seeded(c2_text, seed_env):
    data, want = c2_text
    seed_env.pop("WCG_SEED", None)
    with engine(keys=(4 << 20) + 1) as e:
        jobs = [run(e, data) for _ in range(2)]
    for j in jobs:
        ob.assert_same(j["out"], want)
        assert not j["seed"]["valid"] and j["seed"]["builds"] == 0 and not j["seed"]["last_job_seeded"]


def test_two_contexts_seed_themselves(ab_texts, seed_env):
    import torch
    (ta, wa), (tb, wb) = ab_texts
    seed_env.pop("WCG_SEED", None)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    devs = [torch.frombuffer(bytearray(t), dtype=torch.uint8).to("cuda:0") for t in (ta, tb)]
    torch.cuda.synchronize()
    engs = [engine(), engine()]
    try:
        for e, s in zip(engs, streams):
            e.set_stream(s.cuda_stream)
        rates = [[], []]
        for _ in range(3):                                          # context 0 counts A, context 1 B
            for j, e in enumerate(engs):
                e.reset()
                e.map_device(devs[j].data_ptr(), len((ta, tb)[j]))
                e.reduce_async()
            for j, e in enumerate(engs):
                e.reduce_wait()
                ob.assert_same(e.result(), (wa, wb)[j])
                st = e.stats()
                rates[j].append(st["lds_hits"] / st["tokens"])
        print("rates", rates)
        for j, e in enumerate(engs):
            sd = e.seed_stats()
            assert sd["valid"] and sd["builds"] == 1 and sd["last_job_seeded"]
            assert rates[j][1] > rates[j][0] and rates[j][2] > rates[j][0]
    finally:
        for e in engs:
            e.close()


def test_region_overflow_under_a_stale_seed(ab_texts, seed_env):
    (ta, wa), (tb, wb) = ab_texts
    seed_env.pop("WCG_SEED", None)
    seed_env["WCG_REGION_CAP"] = "16"
    with engine() as e:
        j1, j2 = run(e, ta), run(e, tb)
    ob.assert_same(j1["out"], wa)
    ob.assert_same(j2["out"], wb)
    print("global_ops", j1["stats"]["global_ops"], j2["stats"]["global_ops"], "rates", j1["rate"], j2["rate"])
    assert j2["seed"]["last_job_seeded"] and not j2["seed"]["valid"]
    assert j2["stats"]["global_ops"] > 0                            # the full-region branch ran
