"""libwcg's 32-byte record-unit wire format (include/wcg.h: WCG_RECORD_BYTES; csrc/wcg_reduce.h:
k_export_write / k_import), written and read in plain Python.

A unit's count is a free u64, so a handful of crafted units puts counts of any decimal width into
an engine's tables (Engine.import_host), which text cannot do: a count of 10^19 would need 10^19
tokens.  The reference of every crafted job is the plain dict[bytes, int] the units were made
from, formatted by oracle/wc_ref.py with Python's arbitrary-precision integers.

  inline key (1..15 bytes)   one unit  {hi, lo, cnt, ref = length}; hi, lo = the key, zero-padded
                             to 16 bytes, as two big-endian words
  long key (16+ bytes)       a header  {hi, lo, cnt, ref = LONG_FLAG | length << 40}; hi, lo = the
                             key's first 16 bytes, then ceil(length / 24) continuation units of 24
                             key bytes each (zero-padded) with ref = CONT_MARK
All four words of a unit are little-endian u64.
"""
from __future__ import annotations

import random
import struct
from typing import Dict, Iterable, Iterator, List, Mapping, Optional, Tuple

from tests.oracle_bridge import wc_ref

LONG_FLAG = 1 << 63
CONT_MARK = 1 << 62
UNIT = 32
U64_MAX = (1 << 64) - 1


def encode(key: bytes, cnt: int) -> bytes:
    """libwcg record units (csrc/wcg_reduce.h: k_export_write)."""
    if len(key) <= 15:
        pad = key + b"\0" * (16 - len(key))
        hi, lo = struct.unpack(">QQ", pad)
        return struct.pack("<QQQQ", hi, lo, cnt, len(key))
    hi, lo = struct.unpack(">QQ", key[:16])
    out = struct.pack("<QQQQ", hi, lo, cnt, LONG_FLAG | (len(key) << 40))
    for i in range(0, len(key), 24):
        chunk = key[i:i + 24].ljust(24, b"\0")
        out += chunk + struct.pack("<Q", CONT_MARK)
    return out


def decode(buf: bytes) -> Iterator[Tuple[bytes, int]]:
    i, n = 0, len(buf) // 32
    while i < n:
        hi, lo, cnt, ref = struct.unpack_from("<QQQQ", buf, 32 * i)
        assert ref != CONT_MARK, "continuation unit without header"
        if ref & LONG_FLAG:
            ln = (ref >> 40) & ((1 << 23) - 1)
            nu = (ln + 23) // 24
            raw = b"".join(buf[32 * (i + 1 + k): 32 * (i + 1 + k) + 24] for k in range(nu))
            yield raw[:ln], cnt
            i += 1 + nu
        else:
            key = struct.pack(">QQ", hi, lo)[:ref]
            yield key, cnt
            i += 1


def decode_counts(buf: bytes) -> Dict[bytes, int]:
    """decode() summed per key (a key may come in several units; no wrap at 2^64: Python ints)."""
    out: Dict[bytes, int] = {}
    for k, c in decode(buf):
        out[k] = out.get(k, 0) + c
    return out


def split_count(cnt: int, parts: int, rnd: random.Random) -> List[int]:
    """`parts` counts >= 1 that sum to cnt (cnt >= parts), of mixed magnitudes."""
    assert cnt >= parts >= 1
    out, rest = [], cnt
    for left in range(parts - 1, 0, -1):          # `left` more parts follow this one
        hi = rest - left
        c = 1 if hi == 1 else (rnd.randint(1, hi) if rnd.random() < 0.5 else rnd.randint(1, max(1, hi >> rnd.randrange(64))))
        out.append(c)
        rest -= c
    out.append(rest)
    return out


def units(counts: Mapping[bytes, int], seed: Optional[int] = None,
          split: Optional[Mapping[bytes, int]] = None) -> bytes:
    """The record units of a key -> count dict (counts 1 .. 2^64 - 1).

    seed   None: the dict's own order; else the units in a shuffled order (a long key's header and
           continuation units stay together, as k_import needs)
    split  {key: n}: that key's count is spread over n units (n >= 1 parts >= 1, summing to it),
           which land anywhere in the shuffled order; import adds them up again
    """
    rnd = random.Random(seed)
    blobs = []
    for k, c in counts.items():
        assert 1 <= c <= U64_MAX and len(k) >= 1, (k, c)
        n = split.get(k, 1) if split else 1
        for part in ([c] if n == 1 else split_count(c, n, rnd)):
            blobs.append(encode(k, part))
    if seed is not None:
        rnd.shuffle(blobs)
    return b"".join(blobs)


def add(*dicts: Mapping[bytes, int]) -> Dict[bytes, int]:
    """The reference of several imports / maps into one job: the per-key sum."""
    out: Dict[bytes, int] = {}
    for d in dicts:
        for k, c in d.items():
            out[k] = out.get(k, 0) + c
    return out


def expect(counts: Mapping[bytes, int]) -> bytes:
    """The merged file of a key -> count dict: bytewise key order, "key: count\\n"."""
    return wc_ref.merged_output(dict(counts))


def expect_res(counts: Mapping[bytes, int], nreduce: int, r: int) -> bytes:
    """The -res-<r> file (JSON lines) of a key -> count dict."""
    return wc_ref.res_file(dict(counts), nreduce, r)


# ---------------------------------------------------------------- crafted keys and counts
# every decimal width 1..20 at its edges, and the 32-bit / 64-bit edges of put_digits
EDGE_COUNTS: List[int] = sorted(
    {10 ** k + d for k in range(1, 20) for d in (-1, 0, 1)} | {2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 64 - 1})
# one count of each width 1..20
WIDTH_COUNTS: List[int] = [10 ** (w - 1) for w in range(1, 21)]



def count_of_width(w: int, salt: int = 0) -> int:
    """a count of exactly w decimal digits (1..20) with mixed digits, at most 2^64 - 1"""
    assert 1 <= w <= 20
    rnd = random.Random(w * 1000003 + salt)
    s = "1" + "".join(str(rnd.randint(0, 7 if i == 0 else 9)) for i in range(w - 1))
    c = int(s)
    assert len(str(c)) == w and 1 <= c <= U64_MAX
    return c


# key length classes: inline in one prefix word, inline in two, long in its table slot's cell
# (16..32 bytes), long on the arena heap (33+)
LENGTH_CLASSES: List[List[int]] = [[1, 2, 3, 4, 5, 6, 7], [8, 9, 11, 12, 14, 15], [16, 17, 24, 31, 32], [33, 34, 48, 49, 100]]

_DIGITS = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"      # ascending bytes
_FILL = ["ж".encode(), b"x", "中".encode(), b"Q", "ǅ".encode(), b"m", "𝒳".encode()]   # 2, 1, 3, 1, 2, 1, 4 bytes


def letters(i: int, width: int) -> bytes:
    """i in base 52 as `width` ASCII letters; bytewise order = numeric order."""
    assert 0 <= i < 52 ** width
    out = bytearray()
    for _ in range(width):
        out.append(_DIGITS[i % 52])
        i //= 52
    return bytes(reversed(out))


def filler(n: int, phase: int = 0) -> bytes:
    """exactly n bytes of letters, ASCII and 2-, 3- and 4-byte UTF-8 letters mixed"""
    out, k = b"", phase
    while len(out) < n:
        p = _FILL[k % len(_FILL)]
        k += 1
        out += p if len(out) + len(p) <= n else b"y"
    return out


def key_of(i: int, length: int) -> bytes:
    """a letter key of exactly `length` bytes, distinct for distinct (i, length): the index in
    min(length, 3) letters, then filler"""
    w = min(length, 3)
    return letters(i, w) + filler(length - w, i)


def mixed_key(i: int) -> bytes:
    """key i of a mixed set: the length classes in turn, the lengths of each class in turn (a
    length too short to hold the index gives way to 3..7 bytes); distinct for distinct i"""
    length = LENGTH_CLASSES[i % 4][(i // 4) % 5]
    if i >= 52 ** min(length, 3):
        length = 3 + i % 5
    return key_of(i, length)


def ordered_keys(n: int, length: int, first: int = 0) -> List[bytes]:
    """n keys of one length whose bytewise order is their construction order (a fixed-width
    letter-encoded index, then filler)"""
    assert length >= 4
    return [letters(first + i, 4) + filler(length - 4) for i in range(n)]


def edge_count_keys() -> Dict[bytes, int]:
    """every EDGE_COUNTS count paired with a key of every length class (lengths cycle inside a
    class, so 7, 8, 15, 16, 17, 32 and 33 all occur with many widths)"""
    out: Dict[bytes, int] = {}
    for ci, lens in enumerate(LENGTH_CLASSES):
        for j, c in enumerate(EDGE_COUNTS):
            k = key_of(j // len(lens), lens[(j + ci) % len(lens)])
            assert k not in out
            out[k] = c
    return out


def lines(counts: Mapping[bytes, int]) -> List[bytes]:
    """the merged file's lines, in order"""
    return [k + b": " + str(counts[k]).encode() + b"\n" for k in sorted(counts)]
