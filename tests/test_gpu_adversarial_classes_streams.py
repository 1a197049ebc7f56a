"""The class-mixing adversarial cases (tests/adversarial_classes.py, the fixed seeds of tests/test_gpu_adversarial_classes.py)
on the stream forms that file does not open: pm_init_windowed (the halo is sized from the longest pattern of the whole
list, and the piece cap, the carry reach and the host-made edge records depend on the classes the list holds),
pm_init_packed resident and windowed, and the device tally on a windowed handle.  Every permission bit of
pm_config.long_patterns is set as the case says, bit 7 beside them.  Hits against the oracle, tallies against
tests/count_rule.py on the oracle's hits; the residency figures as tests/test_gpu_windowed.py and tests/test_gpu_packed.py
check them for their own lists."""
import collections

import pytest

import adversarial as A
import adversarial_classes as AC
import sat_amd
from test_gpu_adversarial_classes import SEEDS, case, differ, routes_named
from test_gpu_adversarial_classes_stages import check_counts
from test_gpu_packed import check_resident, check_windowed
from test_gpu_windowed import ran_windowed, residency_bound

WINDOWED = SEEDS[:100]
TABLED = [s for s in SEEDS if AC.class_case(s)["table"] is not None]
# packed and resident: every seed with a table, not the first 100 alone -- among those, 3 handles named the halves plan and 5
# the degenerate class, and the condition below asks for 5 of each
PACKED, PACKED_WINDOWED = TABLED, TABLED[:50]
MIN_WINDOW = 2048                                                     # 8 * roundup64(2 L + 3 k + 84) for a longest primer of 33 .. 70 nt, k <= 2
ROUTES = ("pair", "exact", "edits", "halves", "wild", "edit_pair", "short_edit", "short_sub", "residue")


def test_windowed_cases_are_longer_than_two_windows():
    """(CPU) the generator's side of "at least 40 windowed cases loaded more than two windows": a list with a primer of
    33 .. 70 nt has a minimum window of 2048 positions, the cases run at 2048 + 64 (seed % 5), and of the first 100 seeds all
    hold such a primer, 57 have n > 4096 and 54 have n > twice their own window (all 400 seeds: 215 with n > 4096; 170 of the
    306 with a table; of the first 100 with a table, the last of them seed 1026, 57)."""
    cases = [AC.class_case(s) for s in WINDOWED]
    assert sum(any(33 <= L <= 70 for L in c["lens"]) for c in cases) >= 95
    assert sum(c["n"] > 2 * MIN_WINDOW for c in cases) >= 40
    assert sum(c["n"] > 2 * (MIN_WINDOW + 64 * (c["seed"] % 5)) for c in cases) >= 40
    assert len(TABLED) >= 300 and TABLED[99] == 1026 and sum(AC.class_case(s)["n"] > 2 * MIN_WINDOW for s in TABLED[:100]) >= 40


_RAN = {}
NAMED = {"windowed": collections.Counter(), "packed": collections.Counter()}
HANDLES = collections.Counter()
LOADS = {}


def described(form, desc):
    NAMED[form].update(routes_named(desc)[0])
    HANDLES[form] += 1


def rejected(want, e):
    """the oracle rejects the option set and the library does too, as tests/test_gpu_adversarial_classes.py takes it"""
    return want is None and e.code in (-6, -2)


def windowed_run(seed):
    """the case on a pm_init_windowed handle at its window, in its ranges: (hits, residency, window, ranges, describe()), once per seed"""
    if seed not in _RAN:
        c, _ = case(seed)
        window, chunk = AC.window_of(c)
        got, res, desc = AC.stream_hits(c, window=window, chunk=chunk)
        described("windowed", desc)
        _RAN[seed] = (got, res, window, chunk, desc)
    return _RAN[seed]


def check_windowed_residency(res, c, window):
    assert res["window"] == window and res["bits"] == 0, res
    ran_windowed(res, c["n"])
    assert res["held"] <= res["peak"] <= residency_bound(window), res


@pytest.mark.gpu
@pytest.mark.parametrize("seed", WINDOWED)
def test_class_case_windowed_vs_oracle(seed):
    """the handle's minimum window (observed on an MI355X: 2048 for every case with a primer of 33 nt or more) plus 0 .. 4
    times 64, ranges that do not divide it; the first 30 seeds also with one range over the whole stream, which the library
    cuts to its piece cap"""
    c, want = case(seed)
    try:
        got, res, window, chunk, c["kernel_desc"] = windowed_run(seed)
    except sat_amd.PmError as e:
        if rejected(want, e):
            return
        raise
    assert want is not None, ("the oracle rejects what the library accepts", AC.describe(c))
    LOADS[seed] = res["loads"]
    check_windowed_residency(res, c, window)
    assert got == want, differ(c, got, want, " windowed %d in ranges of %d" % (window, chunk))
    if seed in WINDOWED[:30]:
        got, res, desc = AC.stream_hits(c, window=window)
        described("windowed", desc)
        check_windowed_residency(res, c, window)
        assert got == want, differ(c, got, want, " windowed %d in one range" % window)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", PACKED)
def test_class_case_packed_vs_oracle(seed):
    c, want = case(seed)
    bits = AC.bits_for(c["table"])
    try:
        got, res, desc = AC.stream_hits(c, packed=True)
    except sat_amd.PmError as e:
        if rejected(want, e):
            return
        raise
    assert want is not None, ("the oracle rejects what the library accepts", AC.describe(c))
    described("packed", desc)
    c["kernel_desc"] = desc
    assert res["bits"] == bits, res
    check_resident(res, c["n"], bits)
    assert got == want, differ(c, got, want, " packed, %d bits" % bits)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", PACKED_WINDOWED)
def test_class_case_packed_windowed_vs_oracle(seed):
    c, want = case(seed)
    bits = AC.bits_for(c["table"])
    try:
        _, base, window, chunk, _ = windowed_run(seed)
        got, res, desc = AC.stream_hits(c, window=window, packed=True, chunk=chunk)
    except sat_amd.PmError as e:
        if rejected(want, e):
            return
        raise
    assert want is not None, ("the oracle rejects what the library accepts", AC.describe(c))
    described("packed", desc)
    c["kernel_desc"] = desc
    assert res["bits"] == bits, res
    check_windowed(res, base, c["n"], window, bits)
    assert got == want, differ(c, got, want, " packed, %d bits, windowed %d in ranges of %d" % (bits, window, chunk))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", WINDOWED[:30])
def test_class_case_counts_on_a_windowed_handle(seed):
    """pm_count_scan on a windowed handle: the host re-aligns (include/pm_gpu.h, pm_count_scan), the tallies are the rule's"""
    c, want = case(seed)
    assert want is not None, AC.describe(c)
    window, chunk = AC.window_of(c)
    pm = AC.handle(c, window=window)
    try:
        described("windowed", pm.describe())
        for M in (0, 3):
            check_counts(c, want, M, pm.count_all(max_count=M, chunk=chunk), "windowed %d" % window, resident=False)
    finally:
        pm.close()


# ---- primers that lie over the two ends of the stream -------------------------------------------------------------------------
EDGE = AC.edge_seeds(SEEDS)
_EDGE_WANT = {}


def edge(seed):
    c = AC.edge_case(seed)
    if seed not in _EDGE_WANT:
        _EDGE_WANT[seed] = A.oracle_hits(c)
    return c, _EDGE_WANT[seed]


def test_edge_cases_have_hits_at_both_ends_of_the_stream():
    """(CPU) the oracle alone: of the 37 cases, 7 have the hit of the first 40-mer at end 40 - k (its first k characters
    missing in front of the stream) and 28 a hit of the second at the stream's last position or beyond it (exact_halves
    extends over the end)"""
    assert len(EDGE) >= 30, EDGE
    start = end = 0
    for seed in EDGE:
        c, want = edge(seed)
        assert want is not None and c["lens"][0] == c["lens"][1] == 40
        start += (40 - c["k"], 1) in [(h[0], h[1]) for h in want]
        end += any(h[1] == 2 and h[0] >= c["n"] for h in want)
    assert start >= 5 and end >= 20, (start, end)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", EDGE)
def test_edge_case_windowed_and_in_tiny_ranges_vs_oracle(seed):
    """the host-made records of the two stream ends for primers of 40 nt (pm_api.cpp edge_reach: 64 with a long class, else
    32) on a windowed handle and in pm_scan ranges of a few positions at both ends of a resident one"""
    c, want = edge(seed)
    window, chunk = AC.window_of(c)
    got, res, c["kernel_desc"] = AC.stream_hits(c, window=window, chunk=chunk)
    check_windowed_residency(res, c, window)
    assert got == want, differ(c, got, want, " edge primers, windowed %d in ranges of %d" % (window, chunk))
    n = c["n"]
    got = A.gpu_hits(c, kernel=sat_amd.KERNEL_AUTO, route=AC.route_of(c),
                     cuts=[1, 3, 7, 19, 33, 37, 38, 39, 40, 42, 60, 64, 66, 70, n // 2, n - 70, n - 66, n - 42, n - 40, n - 38, n - 30, n - 5, n - 3, n - 2, n - 1])
    assert got == want, differ(c, got, want, " edge primers, tiny ranges")


@pytest.mark.gpu
def test_the_classes_did_run_on_these_streams():
    """(after the cases above, in file order) every route was named by windowed and by packed handles, and the windowed cases
    were longer than their ring"""
    if len(LOADS) < len(WINDOWED) // 2 or HANDLES["packed"] < len(PACKED) // 2:
        pytest.skip("the cases did not run in this process")
    over_two = sum(1 for v in LOADS.values() if v > 2)
    print("class streams: %d windowed handles named %s; %d packed handles named %s; window loads per windowed case: %d cases with more than two, most %d" % (
        HANDLES["windowed"], dict(sorted(NAMED["windowed"].items())), HANDLES["packed"], dict(sorted(NAMED["packed"].items())), over_two, max(LOADS.values())))
    for form in ("windowed", "packed"):
        for name in ROUTES:
            assert NAMED[form][name] >= 5, (form, name, dict(NAMED[form]))
    assert over_two >= 40, (over_two, sorted(LOADS.items()))
