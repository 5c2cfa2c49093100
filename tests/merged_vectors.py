"""Merged files ("key: count\\n" lines) for the tests of wcg.check_merged, wcg_index_merged and
wcg_load_merged*: files of about five lines with one defect each, and the (line, rule) that defect
is, written down by hand; valid files at the edges of the rules.

tests/test_merged_query.py holds wcg.check_merged to these on the CPU; tests/test_gpu_merged_query.py
holds the device to check_merged and to these.
"""
from typing import List, Optional, Tuple

TIE17 = b"tiegroupprefixabc"                      # 17 bytes: keys that share it differ only after byte 16
assert len(TIE17) == 17


def file_of(lines: List[bytes]) -> bytes:
    return b"".join(l + b"\n" for l in lines)


def _with(line: bytes) -> bytes:
    """five lines, the second (index 1) replaced: keys B < a... < b < c < d"""
    return file_of([b"B: 1", line, b"b: 7", b"c: 9", b"d: 11"])


NUL3 = b"abc\0de"                                 # a zero byte at position 3 (an inline key)
NUL20 = b"abcdefghijklmnopqrst\0uv"               # ... at position 20 (a long key, past the prefix)
assert NUL3[3] == 0 and NUL20[20] == 0

# (id, file, (index of the first bad line, rule))
REJECTED: List[Tuple[str, bytes, Tuple[int, str]]] = [
    ("zero", _with(b"a: 0"), (1, "zero")),
    ("leading-zeros", _with(b"a: 007"), (1, "count")),
    ("21-digits", _with(b"a: 1" + b"0" * 20), (1, "count")),
    ("2^64", _with(b"a: 18446744073709551616"), (1, "count")),
    ("no-digits", _with(b"a: "), (1, "count")),
    ("no-space", _with(b"a:5"), (1, "count")),
    ("letter-after-count", _with(b"a: 5x"), (1, "count")),
    ("space-after-count", _with(b"a: 5 "), (1, "count")),
    ("short-keys-swapped", file_of([b"B: 1", b"b: 7", b"a: 5", b"c: 9", b"d: 11"]), (2, "order")),
    ("equal-adjacent", file_of([b"B: 1", b"a: 5", b"a: 6", b"c: 9", b"d: 11"]), (2, "order")),
    ("tie-keys-swapped", file_of([b"B: 1", b"a: 5", TIE17 + b"qb: 2", TIE17 + b"qa: 3", b"u: 4"]), (3, "order")),
    ("nul-at-3", _with(NUL3 + b": 5"), (1, "nul")),
    ("nul-at-20", _with(NUL20 + b": 5"), (1, "nul")),
    # beyond the issue's list: the same rules from other sides
    ("no-colon", _with(b"abc"), (1, "count")),
    ("empty-key", file_of([b": 5", b"a: 1", b"b: 2"]), (0, "count")),
    ("colon-in-key", _with(b"a:b: 5"), (1, "count")),
    ("nul-after-count", _with(b"a: 5\0"), (1, "count")),
    ("zero-with-leading-zero", _with(b"a: 00"), (1, "count")),
    ("equal-long-keys", file_of([b"B: 1", TIE17 + b"x: 2", TIE17 + b"x: 3", b"u: 4"]), (2, "order")),
    ("prefix-after-extension", file_of([b"B: 1", TIE17 + b"xy: 2", TIE17 + b"x: 3", b"u: 4"]), (2, "order")),
    ("last-line-bad", file_of([b"B: 1", b"a: 5", b"b: 7", b"c: 9", b"d: 0"]), (4, "zero")),
    ("two-defects-first-wins", file_of([b"B: 1", b"b: 7", b"a: 0", b"c: 9", b"c: 9"]), (2, "zero")),
]

# the last line lacks its newline: looked at before anything else
NO_NEWLINE = [(b"a: 1\nb: 2", (1, "newline")), (b"a: 1", (0, "newline")), (b"a: 0\nb: 2\nc", (2, "newline"))]

VALID: List[bytes] = [
    b"",
    b"a: 1\n",                                                       # one line
    b"word: 18446744073709551615\n",                                 # 2^64 - 1
    file_of([b"B: 1", b"a: 10000000000000000000", b"ab: 9", b"b: 18446744073709551615"]),
    file_of([b"a: 1", TIE17 + b": 2", TIE17 + b"a: 3", TIE17 + b"ab: 4", TIE17 + b"b: 5"]),   # a prefix first
    file_of([b"a b: 1", b"a-b: 2", b"a.b 7: 3"]),                    # keys need not be letters
]


def kind_line(msg: str) -> Optional[Tuple[int, str]]:
    """(line, rule) out of wcg_last_error's "wcg_index_merged: line <N>: <rule> (...)" """
    import re
    m = re.search(r"line (\d+): (\w+)", msg)
    return (int(m.group(1)), m.group(2)) if m else None
