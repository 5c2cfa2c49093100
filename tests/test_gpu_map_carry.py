"""k_map's carried tokens: inputs on which every wave runs several steps.

A list's partial last iteration stays in registers - raw: the start-list entry and the aligned key
dwords - and fills the first lanes of the next step's first iteration, where it is decoded.  A wave
takes a second step only past CUs * 16 * 992 bytes (4.06 MB on 256 CUs: k_map's grid is
min(CUs, ceil(steps / 16)) workgroups of 16 waves), so the suite's few-MiB inputs never carry a
token from one step to the next.  Every input here is sized from the device's CU count so that
each wave runs at least 4 steps, and each case asserts that.

Cases (each compared byte for byte with the C oracle, and stats()["tokens"] with its count):
  short        only short tokens, 198.4 per step on average (not a multiple of 64), period 455
  short_exact  exactly 256 short tokens in every step of the first half, 128 in the second: the
               leftover is always 0
  medium_few   only tokens of 8-15 bytes, ~10.2 per step: the carry grows for 6 steps before the
               first medium iteration runs, so this input has 8 steps per wave
  medium_long  tokens of 8-15 bytes interleaved with tokens of 16, 17 and 40 bytes: carried medium
               entries that are no medium key, long tokens logged in their own step
  stretches    stretches without any medium token (tm = 0) between stretches of ~80 per step
  utf8         stretches + medium_long with 2-, 3- and 4-byte letters sprinkled in, and runes
               placed across the end of a step's last chunk
  medium_long through the two-pass instance k_map<0, false> (max_keys past the one-pass limit, as
               tests/test_gpu_capacity.py forces it)
"""
import functools
import random

import pytest

from tests import oracle_bridge as ob

pytestmark = pytest.mark.gpu

MAP_STEP, MAP_WAVES = 992, 16   # input bytes per wave step, waves per map workgroup
ABC = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
FILL = b" 0123456789.,;:-+*/()[]"            # no letters
RUNES = ["é".encode(), "中".encode(), "\U0001d400".encode(), "ж".encode()]   # 2, 3, 4, 2 bytes


@functools.lru_cache(maxsize=None)
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def size(steps_per_wave=4):
    return steps_per_wave * cus() * MAP_WAVES * MAP_STEP + 333


def min_steps_per_wave(n):
    steps = -(-n // MAP_STEP)
    grid = min(cus(), -(-steps // MAP_WAVES))
    return steps // (grid * MAP_WAVES)


def word(rng, n):
    return bytes(rng.choice(ABC) for _ in range(n))


def fill(pattern, n):
    return (pattern * (n // len(pattern) + 1))[:n]


def short_pattern(rng):
    """13 groups of 7 words of 1..7 bytes: 455 bytes, 91 tokens"""
    p = b"".join(word(rng, k) + b" " for _ in range(13) for k in (1, 2, 3, 4, 5, 6, 7))
    assert len(p) == 455 and MAP_STEP % len(p) != 0
    assert (MAP_STEP * 91 / 455) % 64 != 0
    return p


def exact_period(rng, lens):
    """992 bytes: 32 groups of 31 bytes (the words of `lens`, a space after each)"""
    assert sum(lens) + len(lens) == 31 and max(lens) <= 7
    p = b"".join(word(rng, k) + b" " for _ in range(32) for k in lens)
    assert len(p) == MAP_STEP
    return p


def medium_few_pattern(rng):
    """5 x 8 units of 97 bytes, one word of 8..15 bytes each: 10.2 tokens per step"""
    units = []
    for i in range(5):
        for k in range(8, 16):
            w = word(rng, k)
            units.append(w + fill(FILL[i:] + FILL[:i], 97 - k))
    p = b"".join(units)
    assert len(p) == 5 * 776 and MAP_STEP % 776 != 0
    return p


def medium_long_pattern(rng):
    p = b"".join(word(rng, k) + b" " for _ in range(3) for k in (9, 16, 12, 8, 17, 15, 10, 40, 11, 13, 14))
    assert len(p) == 3 * 176 and MAP_STEP % 176 != 0
    return p


def stretches_pattern(rng):
    dense = b"".join(word(rng, k) + b" " for _ in range(40) for k in (8, 15, 11, 9, 14, 12, 10, 13))
    return fill(short_pattern(rng), 3 * MAP_STEP + 123) + b" " + fill(dense, 2 * MAP_STEP + 77) + b" "


def sprinkle(data):
    """runes over ASCII letters (a token keeps its length in bytes): one every 101 bytes where the
    bytes there are letters, and one starting 1, 2 or 3 bytes before the end of every 7th step"""
    d = bytearray(data)
    nsteps = len(d) // MAP_STEP
    straddle = [MAP_STEP * j - 1 - (j % 3) for j in range(1, nsteps, 7)]
    placed = 0
    for i, p in enumerate(straddle + list(range(50, len(d) - 4, 101))):
        # a straddling rune needs more bytes than are left in its step
        r = RUNES[2] if i < len(straddle) else RUNES[i % len(RUNES)]
        if bytes(d[p:p + len(r)]).isalpha():
            d[p:p + len(r)] = r
            placed += i < len(straddle)
    assert placed >= 16, placed
    return bytes(d)


@functools.lru_cache(maxsize=None)
def corpus(name):
    rng = random.Random(sum(name.encode()))
    if name == "short":
        return fill(short_pattern(rng), size())
    if name == "short_exact":
        n = size()
        half = n // (2 * MAP_STEP) * MAP_STEP
        a, b = exact_period(rng, (3, 3, 3, 3, 3, 3, 3, 2)), exact_period(rng, (7, 7, 7, 6))
        assert len(a.split()) == 4 * 64 and len(b.split()) == 2 * 64
        return fill(a, half) + fill(b, n - half)
    if name == "medium_few":
        return fill(medium_few_pattern(rng), size(8))
    if name == "medium_long":
        return fill(medium_long_pattern(rng), size())
    if name == "stretches":
        return fill(stretches_pattern(rng), size())
    if name == "utf8":
        return sprinkle(fill(stretches_pattern(rng) + fill(medium_long_pattern(rng), MAP_STEP + 201) + b" ", size()))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def want(name):
    """the oracle's merged file and token count: computed once, shared by both instances' tests"""
    r = ob.Result(corpus(name))
    return r.merged(), r.ntokens


def engine(max_keys):
    import wcg
    return wcg.Engine(device=0, max_input_bytes=size(8), max_keys=max_keys)


@pytest.fixture(scope="module")
def one_pass(built):
    e = engine(1 << 20)                 # k_map<0, true>
    yield e
    e.close()


@pytest.fixture(scope="module")
def two_pass(built):
    e = engine((4 << 20) + 1)           # k_map<0, false>
    yield e
    e.close()


def check(eng, name):
    data = corpus(name)
    assert min_steps_per_wave(len(data)) >= 4      # every wave carries tokens over >= 3 step ends
    merged, ntokens = want(name)
    eng.reset()
    eng.map_host(data)
    eng.reduce()
    st = eng.stats()
    ob.assert_same(eng.result(), merged)
    assert st["tokens"] == ntokens
    assert st["overflow"] == 0 and st["spin_fail"] == 0
    return st


@pytest.mark.parametrize("name", ["short", "short_exact", "medium_few", "medium_long", "stretches", "utf8"])
def test_carry_one_pass(one_pass, name):
    st = check(one_pass, name)
    if name == "medium_few":
        assert min_steps_per_wave(len(corpus(name))) >= 8     # 7 * 10.2 > 64: a medium iteration runs
    if name == "medium_long":
        assert st["long_tokens"] > 0


def test_carry_two_pass_medium_long(two_pass):
    st = check(two_pass, "medium_long")
    assert st["long_tokens"] > 0
