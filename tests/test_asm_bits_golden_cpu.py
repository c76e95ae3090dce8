"""tests/golden/asm_bits_parent.json (the digests tests/test_gpu_asm_bits.py compares against) is complete: every case of
tests/asm_bits_cases.py exactly once, both paths, every buffer, 64 hex digits each.  No GPU needed."""
import json
import os
import re

import asm_bits_cases as ab                        # tests/asm_bits_cases.py


def _pairs_no_duplicates(pairs):
    keys = [k for k, _ in pairs]
    assert len(set(keys)) == len(keys), sorted(k for k in set(keys) if keys.count(k) > 1)
    return dict(pairs)


def test_golden_lists_every_case_exactly_once():
    assert os.path.getsize(ab.GOLDEN) < 256 * 1024
    with open(ab.GOLDEN) as f:
        doc = json.load(f, object_pairs_hook=_pairs_no_duplicates)      # a case listed twice is an error, not an overwrite
    ids = [c[0] for c in ab.all_cases()]
    assert len(set(ids)) == len(ids)
    assert sorted(doc["digests"]) == sorted(ids)
    for cid in ids:
        entry = doc["digests"][cid]
        assert sorted(entry) == sorted(p for p, _ in ab.PATHS), cid
        for p, _ in ab.PATHS:
            assert sorted(entry[p]) == sorted(ab.BUFFERS), (cid, p)
            for b in ab.BUFFERS:
                assert re.fullmatch(r"[0-9a-f]{64}", entry[p][b]), (cid, p, b)


def test_cases_cover_what_the_golden_file_is_for():
    cases = dict(ab.all_cases())
    plain = [c for c in cases.values() if c["batch"] == 1 and c["pivot"] is None]
    assert {(c["S"], c["C"]) for c in plain} == {(14, 7), (2, 1), (4, 2), (6, 3), (32, 16)}
    for S, C in ab.SHAPES:
        for dt in ("float64", "float32"):
            assert sorted(c["K"] for c in plain if (c["S"], c["C"], c["dt"]) == (S, C, dt)) == [1, 2, 3, 5]
    assert sorted(c["dt"] for c in cases.values() if c["batch"] == 3 and (c["S"], c["C"], c["K"]) == (14, 7, 3)) == ["float32", "float64"]
    assert sorted(c["pivot"] for c in cases.values() if c["pivot"]) == ["1e+300", "1e-300"]
    assert all(c["dt"] == "float64" for c in cases.values() if c["pivot"])
