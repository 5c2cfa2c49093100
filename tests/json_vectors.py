"""The rules wcg_import_json holds the reference's JSON files to, restated on the host, and
hand-written files that break them.

check_json is written from the rule list in include/wcg.h, not from the kernels: per line (B = the
line without its newline, L = its length), the first broken rule of
  frame  L >= 10, B starts with {"Key":" and ends with "}
  value  V = the run of bytes other than '"' that ends at L-2, followed back for at most 21 bytes and
         never into B[0..8); not empty, opened by a '"' within those bounds; MAP: V == b"1";
         RES: a canonical decimal in 1 .. 2^64-1
  sep    the 11 bytes that end with V's opening quote are ","Value":" and begin at offset >= 8
  key    K = B[8 .. L-2-len(V)-11) has 1 .. 2^23-1 bytes and the reference's tokenizer returns [K]
and, for the file, "newline" (line -1): a last byte other than a newline.

VECTORS: (name, file, mode, line, rule), each pair written by hand.
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import wc_ref  # noqa: E402

MAP, RES = 0, 1
KEY_MAX = (1 << 23) - 1
U64_MAX = (1 << 64) - 1


def tile() -> int:
    """IJ_TILE: the text bytes one workgroup checks (csrc/wcg_import_json.h)"""
    src = open(os.path.join(ROOT, "mit-6.824-2015_amd", "csrc", "wcg_import_json.h")).read()
    m = re.search(r"constexpr \w+ IJ_TILE = (\d+);", src)
    assert m, "IJ_TILE"
    return int(m.group(1))


def ln(key: bytes, value: bytes = b"1") -> bytes:
    return b'{"Key":"' + key + b'","Value":"' + value + b'"}\n'


def _line_rule(B: bytes, mode: int):
    L = len(B)
    if L < 10 or not B.startswith(b'{"Key":"') or not B.endswith(b'"}'):
        return "frame"
    j = L - 2                                  # V = B[j : L-2]
    while L - 2 - j < 21 and j - 1 >= 8 and B[j - 1:j] != b'"':
        j -= 1
    q = j - 1                                  # V's opening quote
    if q < 8 or B[q:q + 1] != b'"':
        return "value"
    V = B[j:L - 2]
    if not V:
        return "value"
    if mode == MAP:
        if V != b"1":
            return "value"
    else:
        if len(V) > 20 or not V.isdigit() or V[:1] == b"0" or int(V) > U64_MAX or not all(48 <= c <= 57 for c in V):
            return "value"
    if q - 10 < 8 or B[q - 10:q + 1] != b'","Value":"':
        return "sep"
    K = B[8:q - 10]
    if not 1 <= len(K) <= KEY_MAX or wc_ref.tokens(K) != [K]:
        return "key"
    return None


def check_json(data: bytes, mode: int):
    """None for a file wcg_import_json accepts, else (line, rule): the lowest offending line (from 0)
    and the first rule it breaks; (-1, "newline") for a last byte other than a newline."""
    assert mode in (MAP, RES)
    if not data:
        return None
    if data[-1:] != b"\n":
        return (-1, "newline")
    for i, B in enumerate(data[:-1].split(b"\n")):
        rule = _line_rule(B, mode)
        if rule:
            return (i, rule)
    return None


def parse(data: bytes, mode: int):
    """key -> summed count of an accepted file"""
    out = {}
    for B in data[:-1].split(b"\n") if data else []:
        v = B[:-2].rsplit(b'"', 1)[1]
        k = B[8:len(B) - 2 - len(v) - 11]
        out[k] = out.get(k, 0) + int(v)
    return out


GOOD = ln(b"abc")
E_ACUTE = "é".encode()


def _two_tiles():
    """two bad lines in different tiles: the lower line wins, whatever the rules' order"""
    T = tile()
    per = len(ln(b"word"))
    n1 = T // per + 5                           # line n1 ends in the second tile
    n2 = 2 * T // per + 9                       # line n1 + 1 + n2 ends in the third or later
    data = ln(b"word") * n1 + ln(b"bad1") + ln(b"word") * n2 + b'{"key":"x","Value":"1"}\n' + ln(b"word") * 3
    return data, n1


_TT, _TT_LINE = _two_tiles()

VECTORS = [
    ("no final newline", GOOD + ln(b"x")[:-1], MAP, -1, "newline"),
    ("no final newline, one byte", b"{", RES, -1, "newline"),
    ("lower-case key field", GOOD + b'{"key":"abc","Value":"1"}\n', MAP, 1, "frame"),
    ("empty line", GOOD + b"\n" + GOOD, MAP, 1, "frame"),
    ("only a newline", b"\n", RES, 0, "frame"),
    ("carriage return", GOOD + ln(b"x")[:-1] + b"\r\n" + GOOD, MAP, 1, "frame"),
    ("garbage after the brace", GOOD + GOOD + ln(b"x")[:-1] + b" \n", MAP, 2, "frame"),
    ("two objects on a line, then garbage", ln(b"x")[:-1] + ln(b"y")[:-1] + b",\n", MAP, 0, "frame"),
    ("nine bytes", b'{"Key":"}\n', MAP, 0, "frame"),
    ("ten bytes: no room for a value", b'{"Key":""}\n', MAP, 0, "value"),
    ("no value field", b'{"Key":"a"}\n', RES, 0, "value"),
    ("the value's quote would lie in the frame", b'{"Key":"abcdefgh"}\n', RES, 0, "value"),
    ("value 2 in MAP mode", GOOD + ln(b"a", b"2"), MAP, 1, "value"),
    ("value 10 in MAP mode", ln(b"a", b"10"), MAP, 0, "value"),
    ("empty value", ln(b"a", b""), RES, 0, "value"),
    ("empty value in MAP mode", ln(b"a", b""), MAP, 0, "value"),
    ("value 0", GOOD + ln(b"a", b"0"), RES, 1, "value"),
    ("value 01", ln(b"a", b"01"), RES, 0, "value"),
    ("value 1a", ln(b"a", b"1a"), RES, 0, "value"),
    ("value -1", ln(b"a", b"-1"), RES, 0, "value"),
    ("21 digits", ln(b"a", b"123456789012345678901"), RES, 0, "value"),
    ("25 digits: no quote within 21 bytes", ln(b"a", b"1234567890123456789012345"), RES, 0, "value"),
    ("2^64", ln(b"a", b"18446744073709551616"), RES, 0, "value"),
    ("2^64 + 3", ln(b"a", b"18446744073709551619"), RES, 0, "value"),
    ("20 digits above 2^64", ln(b"a", b"99999999999999999999"), RES, 0, "value"),
    ("lower-case value field", GOOD + b'{"Key":"a","value":"1"}\n', MAP, 1, "sep"),
    ("separator without the comma", b'{"Key":"a" "Value":"1"}\n', RES, 0, "sep"),
    ("separator inside the frame", b'{"Key":"Value":"1"}\n', MAP, 0, "sep"),
    ("empty key", ln(b""), MAP, 0, "key"),
    ("space in the key", ln(b"a b"), MAP, 0, "key"),
    ("digit in the key", ln(b"a1"), RES, 0, "key"),
    ("quote in the key", ln(b'a"b'), MAP, 0, "key"),
    ("escaped quote in the key", ln(b'a\\"b'), MAP, 0, "key"),
    ("\\u escape in the key", ln(b"caf\\u00e9"), MAP, 0, "key"),
    ("NUL in the key", ln(b"a\0b"), MAP, 0, "key"),
    ("lone 0xC3 at the key's end", ln(b"a\xc3"), MAP, 0, "key"),
    ("lone 0xC3 inside the key", ln(b"a\xc3b"), RES, 0, "key"),
    ("lone continuation byte", ln(b"\x80"), MAP, 0, "key"),
    ("overlong C0 80", ln(b"\xc0\x80"), MAP, 0, "key"),
    ("surrogate ED A0 80", ln(b"a\xed\xa0\x80"), MAP, 0, "key"),
    ("U+00D7, no letter", ln(E_ACUTE + "×".encode() + E_ACUTE), MAP, 0, "key"),
    ("above U+10FFFF", ln(b"\xf4\x90\x80\x80"), RES, 0, "key"),
    ("truncated 4-byte rune", ln(b"\xf0\x9d\x92"), MAP, 0, "key"),
    ("key of 2^23 bytes", ln(b"k" * (KEY_MAX + 1)), RES, 0, "key"),
    ("two bad lines in different tiles", _TT, MAP, _TT_LINE, "key"),
    ("value and sep and key broken on one line", b'{"Key":"a1","value":"2"}\n', MAP, 0, "value"),
    ("sep and key broken on one line", GOOD + b'{"Key":"a1","value":"7"}\n', RES, 1, "sep"),
    ("frame and key broken on one line", b'{"Key":"a1","Value":"1"}x\n', MAP, 0, "frame"),
]
