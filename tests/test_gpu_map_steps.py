"""k_map's step arithmetic at its edges: 32-bit step index, count and stride, the tail boundary as a
step index, the window origin formed from the 32-bit step.

k_map's grid is G = min(CUs, ceil(steps / 16)) workgroups of 16 waves; wave w of workgroup g takes
the 992-byte steps g * 16 + w + k * G * 16.  The main loop is unrolled over four register sets and
leaves at the first step whose 1 KiB window passes the input's end; that step and the later ones
are reloaded byte-exactly.  Sizes (bytes), G taken from the device's CU count:

  1, 991, 992, 993       one step and the first byte of a second one (all of them tail steps)
  G*16*992 - 1, +0, +1   every wave has exactly one step; +1 is the first byte of any wave's
                         second step
  4*G*16*992 + 977       all four register sets, the break inside the unrolled block
  5*G*16*992 + 15        the block's first set again, a 15-byte last step in the byte-exact tail loop

Content, both cut off at the size (so a token or a rune may end with the input):
  ascii   short (1-7 bytes), medium (8-15) and 40-byte tokens, period 283 (a prime: tokens of
          every kind cross step ends at every offset)
  utf8    the same with 2-, 3- and 4-byte letters over it: one every 101 bytes, and one that starts
          1, 2 or 3 bytes before the end of every step of a 7-step block

Each case is compared byte for byte with the C oracle, and stats()["tokens"] with its count; one
case runs through the two-pass instance k_map<0, false> (max_keys past the one-pass limit, as
tests/test_gpu_capacity.py forces it).  The largest input is about 20 MB on 256 CUs."""
import functools
import random

import pytest

from tests import oracle_bridge as ob

pytestmark = pytest.mark.gpu

MAP_STEP, MAP_WAVES = 992, 16   # input bytes per wave step, waves per map workgroup
ABC = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
RUNES = ["é".encode(), "中".encode(), "\U0001d400".encode(), "ж".encode()]   # 2, 3, 4, 2 bytes
LENS = (3, 9, 1, 40, 7, 12, 5, 15, 2, 8, 6, 40, 4, 11, 7, 13, 1, 14, 3, 10, 5, 40)

SIZES = {
    "1": lambda g: 1,
    "991": lambda g: 991,
    "992": lambda g: 992,
    "993": lambda g: 993,
    "G-1": lambda g: g * MAP_WAVES * MAP_STEP - 1,
    "G": lambda g: g * MAP_WAVES * MAP_STEP,
    "G+1": lambda g: g * MAP_WAVES * MAP_STEP + 1,
    "4G+977": lambda g: 4 * g * MAP_WAVES * MAP_STEP + 977,
    "5G+15": lambda g: 5 * g * MAP_WAVES * MAP_STEP + 15,
}
MAX_BYTES = SIZES["5G+15"]


@functools.lru_cache(maxsize=None)
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def steps_per_wave(n):
    """(fewest, most) steps of a wave of a map launch over n bytes"""
    steps = -(-n // MAP_STEP)
    grid = min(cus(), -(-steps // MAP_WAVES))
    return steps // (grid * MAP_WAVES), -(-steps // (grid * MAP_WAVES))


@functools.lru_cache(maxsize=None)
def ascii_pattern():
    rng = random.Random(20240607)
    p = b"".join(bytes(rng.choice(ABC) for _ in range(k)) + b" " for k in LENS)
    assert len(p) == sum(LENS) + len(LENS) == 278
    p = p[:-1] + b", .;- "                      # 283: a prime, so coprime to 992 = 32 * 31
    assert len(p) == 283
    return p


@functools.lru_cache(maxsize=None)
def utf8_block():
    """7 steps of the ASCII text with runes written over it (a block's bytes keep their offsets)"""
    n = 7 * MAP_STEP
    p = ascii_pattern()
    d = bytearray((p * (n // len(p) + 1))[:n])
    for i, q in enumerate(range(50, n - 4, 101)):
        r = RUNES[i % len(RUNES)]
        d[q:q + len(r)] = r
    for j in range(1, 8):                       # the rune starts 1, 2 or 3 bytes before step j's end
        back = 1 + j % 3
        r = RUNES[back - 1]                     # one byte more than is left in the step
        assert len(r) == back + 1
        q = j * MAP_STEP - back
        d[q:q + len(r)] = r
    out = bytes(d[:n])                          # the last rune runs into the next block's start ...
    tail = bytes(d[n:])                         # ... whose first bytes it replaces
    return out, tail


@functools.lru_cache(maxsize=None)
def corpus(kind, label):
    n = SIZES[label](cus())
    if kind == "ascii":
        p = ascii_pattern()
        return (p * (n // len(p) + 1))[:n]
    blk, tail = utf8_block()
    blk2 = tail + blk[len(tail):]               # every block but the first starts with the last rune's end
    return (blk + blk2 * (n // len(blk) + 1))[:n]


@functools.lru_cache(maxsize=None)
def want(kind, label):
    """the oracle's merged file and token count: computed once per input"""
    r = ob.Result(corpus(kind, label))
    return r.merged(), r.ntokens


def engine(max_keys):
    import wcg
    return wcg.Engine(device=0, max_input_bytes=MAX_BYTES(cus()), max_keys=max_keys)


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


def check(eng, kind, label):
    data = corpus(kind, label)
    lo, hi = steps_per_wave(len(data))
    if label in ("G-1", "G"):
        assert (lo, hi) == (1, 1)
    if label == "G+1":
        assert (lo, hi) == (1, 2)
    if label == "4G+977":
        assert (lo, hi) == (4, 5)       # a fifth step on the first wave only: the rest break in set A
    if label == "5G+15":
        assert (lo, hi) == (5, 6)
    merged, ntokens = want(kind, label)
    eng.reset()
    eng.map_host(data)
    eng.reduce()
    st = eng.stats()
    ob.assert_same(eng.result(), merged)
    assert st["tokens"] == ntokens
    assert st["overflow"] == 0 and st["spin_fail"] == 0
    return st


def test_utf8_block_has_runes_across_step_ends():
    blk, tail = utf8_block()
    assert 1 <= len(tail) <= 3
    full = blk + tail
    for j in range(1, 8):
        q = j * MAP_STEP
        starts = [s for s in range(q - 3, q) if full[s] >= 0xC0]
        assert starts, j                                   # a lead byte in the step's last 3 bytes ...
        s = starts[-1]
        width = 2 if full[s] < 0xE0 else 3 if full[s] < 0xF0 else 4
        assert s + width > q, j                            # ... whose rune ends in the next step
        assert full[s:s + width].decode().isalpha()


@pytest.mark.parametrize("label", list(SIZES))
@pytest.mark.parametrize("kind", ["ascii", "utf8"])
def test_steps_one_pass(one_pass, kind, label):
    st = check(one_pass, kind, label)
    if len(corpus(kind, label)) >= 4 * MAP_STEP:
        assert st["long_tokens"] > 0


def test_steps_two_pass(two_pass):
    st = check(two_pass, "utf8", "4G+977")
    assert st["long_tokens"] > 0
