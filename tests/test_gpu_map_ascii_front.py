"""k_map's all-ASCII front end at its edges: the letter mask gathered by v_dot4_u32_u8, the neighbour
masks shifted by DPP with bound_ctrl, the rune carry left to the UTF-8 side and the short slots' run
length read off the inverted window.

A wave's step is 992 input bytes, 62 chunks of 16; its 1 KiB window starts one chunk earlier, so
lane 0 holds the previous step's last chunk, lanes 1-62 the step's own chunks and lane 63 the next
step's first chunk.  Input offset p lies in chunk offset p % 16 (992 is a multiple of 16), in window
position p % 992 + 16 of its own step, and - for p % 992 >= 976 or < 16 - in lane 0 of the next
step's window or lane 63 of the previous one's.

Every case is compared byte for byte with the C oracle, and stats()["tokens"] with its count:

  bytes    every value 0x00-0x7F between two letter runs, at every chunk offset 0-15 and at the
           step offsets 975-977, 990, 991, 0, 1, 15, 16 (window positions 991-993, the step's last
           two bytes = lane 0's bits 14-15 for the next step, the next step's first bytes = lane
           63's for this one, and both sides of the first chunk's end); also through
           k_map<0, false>
  slots    chunks of eight one-letter tokens next to chunks without a letter; tokens of 1-17
           bytes, and runs of 32, 33, 40 and 47 letters, starting at every chunk offset (a 7-byte
           token at offset 15 ends the short list's reach, an 8-byte one there is the medium
           list's); a token that ends with its step, one that ends with its window, one that ends
           with the input
  carry    otherwise all-ASCII steps in a 7-step block repeated until every wave has run all four
           register sets: "lanes" has one rune whole inside a step's first chunk (lane 1 there,
           lane 63 of the step before) and one whole inside a step's last chunk (lane 62, and
           lane 0 of the step after), with a step of pure-ASCII window between them; "straddle"
           has 2-, 3- and 4-byte letters across chunk ends and across step ends, ASCII letters on
           both sides"""
import functools
import random

import pytest

from tests import oracle_bridge as ob

pytestmark = pytest.mark.gpu

MAP_STEP, MAP_WAVES = 992, 16
LOWER = b"abcdefghijklmnopqrstuvwxyz"
LETTERS = LOWER + LOWER.upper()
MAX_BYTES = 24 << 20


@functools.lru_cache(maxsize=None)
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def word(rng, n):
    return bytes(rng.choice(LETTERS) for _ in range(n))


# ---- bytes: every ASCII value at every lane position

NAMED = b"@[\\`{\x7f\x00"            # the letters' neighbours in the code table, DEL and NUL
STEP_OFFSETS = (975, 976, 977, 990, 991, 0, 1, 15, 16)
CHUNK_OFFSETS = tuple(100 + 17 * k for k in range(16))      # step offsets 100, 117, ...: chunk offsets 4, 5, ... 3


@functools.lru_cache(maxsize=None)
def bytes_corpus():
    """value v at step offset t of the first step where the spot, its two letter runs and a
    separator on both sides are free.  A step offset holds one value per step, so the 128 values
    take 128 steps, and the adjacent offsets (990, 991, 0, 1 of one step end) a step end each:
    about 510 steps"""
    assert sorted(t % 16 for t in CHUNK_OFFSETS) == list(range(16))
    rng = random.Random(19)
    nsteps = 520
    d = bytearray(b" " * (nsteps * MAP_STEP))
    taken = bytearray(len(d))
    first = {t: 1 for t in CHUNK_OFFSETS + STEP_OFFSETS}
    last = 0
    for v in range(128):
        for t in CHUNK_OFFSETS + STEP_OFFSETS:
            edge = t in STEP_OFFSETS
            left = word(rng, 1 + (v + t) % (2 if edge else 4))
            right = word(rng, 1 + (3 * v + t) % (2 if edge else 4))
            k = first[t]
            while True:
                q = k * MAP_STEP + t
                lo, hi = q - len(left) - 1, q + len(right) + 2
                if not any(taken[lo:hi]):
                    break
                k += 1
            first[t] = k + 1
            d[q - len(left):q] = left
            d[q] = v
            d[q + 1:q + 1 + len(right)] = right
            taken[lo:hi] = b"\x01" * (hi - lo)
            last = max(last, k)
    assert last + 2 <= nsteps
    return bytes(d[:(last + 2) * MAP_STEP])


def test_bytes_corpus_covers_every_value_and_position():
    d = bytes_corpus()
    assert len(d) <= 512 << 10
    seen_chunk, seen_step = set(), set()
    for p in range(1, len(d) - 1):
        if d[p - 1] in LETTERS and d[p + 1] in LETTERS:
            seen_chunk.add((d[p], p % 16))
            seen_step.add((d[p], p % MAP_STEP))
    for v in range(128):
        for off in range(16):
            assert (v, off) in seen_chunk, (v, off)
        for t in STEP_OFFSETS:
            assert (v, t) in seen_step, (v, t)
    for v in NAMED:
        assert v < 128 and v not in LETTERS


# ---- slots: start lists

@functools.lru_cache(maxsize=None)
def slots_corpus():
    rng = random.Random(23)
    out = bytearray()

    def pad_to_chunk():
        out.extend(b" " * (-len(out) % 16))

    for k in range(12):                         # 8 one-letter tokens in a chunk, none in the next
        a = bytes(LETTERS[(5 * k + j) % 52] for j in range(8))
        out.extend(b"".join(bytes([c]) + b" " for c in a))
        out.extend(b" ." * 8 if k % 2 else b"        12345678")
    for n in list(range(1, 18)) + [32, 33, 40, 47]:
        for off in range(16):
            pad_to_chunk()
            out.extend(b" " * 16 if off == 0 else b"")           # a start at offset 0 follows a non-letter chunk
            out.extend(b"-" * off + word(rng, n) + b" ")
    pad_to_chunk()
    # a token that ends with its step (step offset 991), one that ends with its window (the next
    # step's offset 15) and one that ends with the input
    k = len(out) // MAP_STEP + 1
    out.extend(b" " * (k * MAP_STEP - len(out)))
    for end, n in ((MAP_STEP, 5), (2 * MAP_STEP, 9), (3 * MAP_STEP + 16, 6), (4 * MAP_STEP + 16, 12)):
        p = k * MAP_STEP + end - n
        out.extend(b" " * (p - len(out)))
        out.extend(word(rng, n))
    out.extend(b" " * 37 + word(rng, 7))        # ... the input ends with a token
    return bytes(out)


def test_slots_corpus_shape():
    d = slots_corpus()
    toks = ob.tokens(d)
    assert d[-1] in LETTERS
    assert max(len(t) for t in toks) == 47
    starts = set()
    for i in range(len(d)):                     # (length, chunk offset) of every token
        if d[i] in LETTERS and (i == 0 or d[i - 1] not in LETTERS):
            j = i
            while j < len(d) and d[j] in LETTERS:
                j += 1
            starts.add((j - i, i % 16))
    for n in list(range(1, 18)) + [32, 33, 40, 47]:
        for off in range(16):
            assert (n, off) in starts, (n, off)


# ---- carry: runes in otherwise all-ASCII steps

E2, E3, E4 = "é".encode(), "中".encode(), "\U0001d400".encode()


@functools.lru_cache(maxsize=None)
def ascii_block():
    rng = random.Random(29)
    lens = (3, 9, 1, 7, 12, 5, 15, 2, 8, 6, 4, 11, 7, 13, 1, 14, 3, 10, 5)
    p = b"".join(word(rng, k) + b" " for k in lens) + b", .;-\n"
    assert len(p) % 2 == 1 and len(p) % 31 != 0          # coprime to 992
    n = 7 * MAP_STEP
    return (p * (n // len(p) + 1))[:n]


def put_rune(d, p, r):
    """rune r at offset p with an ASCII letter on both sides"""
    d[p - 1] = ord("q")
    d[p:p + len(r)] = r
    d[p + len(r)] = ord("k")


@functools.lru_cache(maxsize=None)
def carry_block(kind):
    d = bytearray(ascii_block())
    if kind == "lanes":
        put_rune(d, 2 * MAP_STEP + 4, E2)               # step 2's first chunk: lane 1 / step 1's lane 63
        put_rune(d, 4 * MAP_STEP + 980, E3)             # step 4's last chunk: lane 62 / step 5's lane 0
        for s in (2, 3, 4):                             # step 3's window is pure ASCII
            lo, hi = (s * MAP_STEP - 16, (s + 1) * MAP_STEP + 16)
            nonascii = [i for i in range(lo, hi) if d[i] >= 0x80]
            assert bool(nonascii) == (s != 3)
    else:
        for j, (c, r) in enumerate(((5, E2), (11, E3), (17, E3), (23, E4), (29, E4), (35, E4))):
            back = (1, 1, 2, 1, 2, 3)[j]                # bytes of the rune before the chunk's end
            put_rune(d, 1 * MAP_STEP + 16 * c - back, r)
        put_rune(d, 3 * MAP_STEP - 1, E2)               # across step ends: 2 -> 3, 4 -> 5, 5 -> 6
        put_rune(d, 5 * MAP_STEP - 2, E3)
        put_rune(d, 6 * MAP_STEP - 3, E4)
        put_rune(d, 4 * MAP_STEP - 1, E4)               # ... and 3 -> 4 with one byte before the end
    bytes(d).decode()                                   # valid UTF-8
    return bytes(d)


@functools.lru_cache(maxsize=None)
def carry_corpus(kind):
    n = 4 * cus() * MAP_WAVES * MAP_STEP + 3 * MAP_STEP + 5      # every wave: four steps; a few: five
    blk = carry_block(kind)
    return (blk * (n // len(blk) + 1))[:n]


# ---- the runs

@functools.lru_cache(maxsize=None)
def want(name):
    r = ob.Result(CORPORA[name]())
    return r.merged(), r.ntokens


CORPORA = {
    "bytes": bytes_corpus,
    "slots": slots_corpus,
    "carry-lanes": lambda: carry_corpus("lanes"),
    "carry-straddle": lambda: carry_corpus("straddle"),
}


def engine(max_keys, max_bytes):
    import wcg
    return wcg.Engine(device=0, max_input_bytes=max_bytes, max_keys=max_keys)


@pytest.fixture(scope="module")
def one_pass(built):
    e = engine(1 << 20, MAX_BYTES)          # k_map<0, true>
    yield e
    e.close()


@pytest.fixture(scope="module")
def two_pass(built):
    e = engine((4 << 20) + 1, 1 << 20)      # k_map<0, false>
    yield e
    e.close()


def check(eng, name):
    data = CORPORA[name]()
    assert len(data) <= MAX_BYTES
    merged, ntokens = want(name)
    eng.reset()
    eng.map_host(data)
    eng.reduce()
    st = eng.stats()
    ob.assert_same(eng.result(), merged)
    assert st["tokens"] == ntokens
    assert st["overflow"] == 0 and st["spin_fail"] == 0
    return st


@pytest.mark.parametrize("name", ["bytes", "slots", "carry-lanes", "carry-straddle"])
def test_front_one_pass(one_pass, name):
    st = check(one_pass, name)
    if name == "slots":
        assert st["long_tokens"] >= 6 * 16          # 16, 17, 32, 33, 40, 47 letters at 16 offsets


@pytest.mark.parametrize("name", ["bytes", "slots"])
def test_front_two_pass(two_pass, name):
    check(two_pass, name)
