"""The host restatement of wcg_import_json's rules (tests/json_vectors.py): what the reference
writes passes, and every hand-written vector gives its hand-written (line, rule)."""
import base64
import glob
import json
import os

import pytest

from tests import json_vectors as jv

wc_ref = jv.wc_ref
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.json")))


def golden_inputs():
    out = []
    for path in GOLDEN:
        doc = json.load(open(path))
        if isinstance(doc, dict) and "input_b64" in doc:
            out.append((os.path.basename(path), base64.b64decode(doc["input_b64"])))
    return out


def test_golden_inputs_are_found():
    assert len(golden_inputs()) >= 10


@pytest.mark.parametrize("name,data", golden_inputs())
def test_reference_output_passes(name, data):
    counts = wc_ref.word_count(data)
    for R in (1, 3):
        parts = wc_ref.map_files(data, R)
        seen = {}
        for p in parts:
            seen.update(jv.parse(bytes(p), jv.MAP))                # the parts' keys are disjoint
        assert seen == counts
        for r in range(R):
            assert jv.check_json(bytes(parts[r]), jv.MAP) is None
            res = wc_ref.res_file(counts, R, r)
            assert jv.check_json(res, jv.RES) is None
            assert jv.parse(res, jv.RES) == {k: v for k, v in counts.items() if wc_ref.ihash(k) % R == r}
            # a -res file is no map file unless every count is 1, and the other way round always holds
            assert jv.check_json(bytes(parts[r]), jv.RES) is None
            if any(v != 1 for v in jv.parse(res, jv.RES).values()):
                assert jv.check_json(res, jv.MAP)[1] == "value"


@pytest.mark.parametrize("name,data,mode,line,rule", jv.VECTORS, ids=[v[0] for v in jv.VECTORS])
def test_vector(name, data, mode, line, rule):
    assert jv.check_json(data, mode) == (line, rule)


def test_every_rule_and_required_case_is_in_the_table():
    assert {v[4] for v in jv.VECTORS} == {"newline", "frame", "value", "sep", "key"}
    assert {v[2] for v in jv.VECTORS} == {jv.MAP, jv.RES}
    T = jv.tile()
    name, data, mode, line, rule = next(v for v in jv.VECTORS if "different tiles" in v[0])
    lines = data.split(b"\n")
    first = sum(len(x) + 1 for x in lines[:line + 1]) - 1         # the lower bad line's newline
    second = next(i for i, x in enumerate(lines) if x.startswith(b'{"key"'))
    assert first // T >= 1 and sum(len(x) + 1 for x in lines[:second + 1]) // T > first // T


def test_accepted_edges():
    ok = [jv.ln(b"a"), jv.ln("é".encode()), jv.ln(b"k" * 70_000), jv.ln("中𝒳ǅ".encode()) * 3]
    for f in ok:
        assert jv.check_json(f, jv.MAP) is None and jv.check_json(f, jv.RES) is None
    for v in (1, 9, 10, 2 ** 32, 10 ** 19, 2 ** 64 - 1):
        assert jv.check_json(jv.ln(b"x", str(v).encode()), jv.RES) is None
    assert jv.check_json(b"", jv.MAP) is None and jv.check_json(b"", jv.RES) is None
    assert jv.parse(jv.ln(b"x", b"7") + jv.ln(b"y", b"8") + jv.ln(b"x", b"5"), jv.RES) == {b"x": 12, b"y": 8}
