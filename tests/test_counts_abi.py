"""CPU: what pm_counts / pm_count_scan / pm_align_hits_device check before they need a device, and the tally rule
itself (tests/count_rule.py) against the real primer_match's recorded output: tests/golden/cli_counts_*.json hold, per
option set, the hits the reference prints with -A '%i %r %E %d' and its -c tallies with and without -M."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sat_amd
import count_rule
from sat_amd import pattern_match as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_calls_before_init_and_null_pointers():
    L = P.load_library()
    counts = np.zeros(8, dtype=np.uint64)
    assert L.pm_counts(None, counts.ctypes.data_as(C.c_void_p), None, 1, None) == -1
    assert L.pm_count_scan(None, 0, 10, 0) == -1
    assert L.pm_align_hits_device(None, None, 0, None, None, None, 0) == -1
    pm = sat_amd.PatternMatch(k=1)
    try:
        pm.add_pattern("ACGTACGTACGTACGTACGT", 1)
        h = pm._h
        assert L.pm_counts(h, counts.ctypes.data_as(C.c_void_p), None, 1, None) == -1          # before pm_init
        assert b"not initialised" in L.pm_last_error(h)
        assert L.pm_count_scan(h, 0, 10, 0) == -1
        assert L.pm_align_hits_device(h, None, 0, None, None, None, 0) == -1
        with pytest.raises(sat_amd.PmError):
            pm.counts()
        with pytest.raises(sat_amd.PmError):
            pm.count_scan(0, 10)
    finally:
        pm.close()


def test_count_info_layout():
    assert C.sizeof(P._CountInfo) == 6 * 8 + 16 and C.sizeof(P._Hit) == 16
    assert P.ALIGNMENT_DTYPE.itemsize == 24


@pytest.mark.parametrize("fixture", ["cli_counts_a", "cli_counts_b"])
def test_tally_rule_reproduces_the_reference(fixture):
    """count_rule.tally over the reference's own hit list gives the reference's own -c output, for every option set and
    -M in {none, 1, 3, 7}: the rule the GPU tests build their expected values with is the reference's"""
    with open(os.path.join(ROOT, "tests", "golden", fixture + ".json")) as f:
        g = json.load(f)
    n = len(g["primers_txt"].split())
    dense = 0
    for oname, h in g["hits"].items():
        k = h["k"]
        recs = [(e, i + (n if r == "R" else 0)) for i, r, e, _ in h["records"]]
        eds = [dd for _, _, _, dd in h["records"]]
        for M in (0, 1, 3, 7):
            counts, capped, info = count_rule.tally(recs, lambda j: eds[j], 2 * n, k, M)
            assert info["bogus"] == 0
            lines = []
            for i in range(1, n + 1):
                for r, pid in (("F", i), ("R", i + n)):
                    c = counts[pid - 1]
                    lines.append("%d %s %d [%s] %s\n" % (i, r, sum(c), " ".join(map(str, c)), "+" if capped[pid - 1] else ""))
            assert "".join(lines) == g["cases"]["%s_M%d_C" % (oname, M)]["stdout"], (fixture, oname, M)
            dense += sum(1 for c in counts if sum(c) >= 7)
    assert dense > 0                                                  # some primer met the largest cap


def test_tally_rule_skips_bogus_hits():
    hits = [(10, 1), (20, 1), (30, 1), (40, 1), (15, 2)]
    eds = [0, 5, 1, 1, 2**31 - 1]
    counts, capped, info = count_rule.tally(hits, lambda j: eds[j], 2, 1, 2)
    assert counts == [[1, 1], [0, 0]] and capped == [1, 0]
    assert info == dict(tallied=2, skipped=1, bogus=2, first_bogus=(15, 2))
