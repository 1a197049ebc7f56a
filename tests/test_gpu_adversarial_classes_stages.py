"""The class-mixing adversarial cases (tests/adversarial_classes.py, the fixed seeds of tests/test_gpu_adversarial_classes.py)
through the two stages behind the scan that hold the final hits in HBM: the device tally (pm_count_scan / pm_counts,
DESIGN.md 5d) and the pairing stage (pm_pcr_setup / pm_pcr_scan / pm_pcr_pair, 5e).  One range's final hits then hold
records for three re-aligners -- pm_align_hits_kernel, pm_align_hits_wide_kernel<4/6/8> and the host list -- compacted and
re-aligned in place, on hit-dense text, with every permission bit of pm_config.long_patterns set (bit 7 beside the case's
own).  Expected values come from the oracle's hits, the oracle's re-alignment (pmoracle.cli_align) and the rules of
tests/count_rule.py and tests/pcr_rule.py; the library's hits come from its own scan, so every case is a parity run too."""
import collections

import pytest

import adversarial_classes as AC
import sat_amd
from test_gpu_adversarial_classes import SEEDS, case
from test_gpu_counts import check

COUNT_SEEDS = SEEDS[:150]
MS = (0, 1, 3)


def over64(c):
    return [i for i, L in enumerate(c["lens"]) if L >= 65]


# ---- the device tally -----------------------------------------------------------------------------------------------------
def test_count_cases_cover_the_tally_rule():
    """(CPU) conditions on the generator and the seed range, from the oracle and the count rule alone.  Seeds 900 .. 1049:
    148 cases have a hit of a primer of 33..64 nt, 24 one of a primer of 65 nt or more, 30 a bogus hit (a hit that re-aligns
    to more than k: 28 under M = 3), 48 skip hits behind M = 3 (all 400 seeds: 394, 71, 64, 123)."""
    f = collections.Counter()
    for seed in COUNT_SEEDS:
        c, hits = case(seed)
        assert hits is not None, ("the reference rejects the option set", AC.describe(c))
        lens = set(c["lens"][pid - 1] for _, pid, _ in hits)
        f["wide"] += any(33 <= L <= 64 for L in lens)
        f["over"] += any(L >= 65 for L in lens)
        f["bogus"] += AC.count_expected(c, hits, 0)[2]["bogus"] > 0
        f["skipped"] += AC.count_expected(c, hits, 3)[2]["skipped"] > 0
    assert f["wide"] >= 100 and f["over"] >= 10 and f["bogus"] >= 10 and f["skipped"] >= 10, dict(f)


TALLIED = collections.Counter()                                       # records per re-aligner over the count cases, for the summary line
COUNTED = {}


def check_counts(c, hits, M, got, what, resident=True):
    """that file's assertions on counts, capped, tallied, skipped, bogus, first_bogus and aligned_device + aligned_host >=
    tallied + bogus; then where the records were re-aligned"""
    want = AC.count_expected(c, hits, M)
    check(c, M, got, what, device_route=None if resident else False, want=want[:3], describe=AC.describe)
    info, asked = got[2], want[3]
    ctx = (what, "M", M, AC.describe(c), info)
    if not resident:
        return
    # No quiet way round the kernels.  DESIGN.md 5d: "`k = 0` without wildcards reads no text; `k = 0` with `-w/-W` compares
    # character by character"; "Device limit: patterns of <= 32 characters for `k >= 1`, `k <= 3`; records beyond it are
    # compacted into a side list [...] and aligned by `align_hits_impl` inside the same call"; with PM_LONG_ALIGN "and indels,
    # 1 <= k <= 3 and a pattern of 33-64 characters in the list" the wide kernel takes that list, "What it cannot take either --
    # more than 64 characters, an empty pattern -- goes into a second compacted list [...] and only that list crosses to the
    # host"; unchanged: "the `-K` one-diagonal branch" (substitutions only, up to 64 characters, in the narrow kernel).  So the
    # host re-aligns at k >= 1 only: primers of 65 nt or more, and primers of 33..64 nt under -k where the long_align bit is
    # clear (AC.host_aligned).  With all seven bits on and no primer over 64 nt nothing is left to it.
    to_host = sum(asked[i] for i, L in enumerate(c["lens"]) if AC.host_aligned(c, L))
    if not any(AC.host_aligned(c, L) for L in c["lens"]):
        assert info["aligned_host"] == 0, ctx
        assert info["aligned_device"] > 0 or info["tallied"] == 0, ctx
    else:
        # a case with a primer of 65 nt or more (at k >= 1; at k = 0 no record needs the host, see above): the host re-aligns at
        # least the tallied-or-bogus hits of those primers
        assert info["aligned_host"] >= sum(asked[i] for i in over64(c)), ctx
        assert info["aligned_host"] >= to_host, ctx
    if what == "count_all":
        TALLIED["device"] += info["aligned_device"]
        TALLIED["host"] += info["aligned_host"]
        TALLIED["wide"] += sum(asked[i] for i, L in enumerate(c["lens"]) if 33 <= L <= 64 and c["k"] >= 1 and c["indels"] and c["route"]["long_align"])
        TALLIED["rule"] += sum(asked)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", COUNT_SEEDS)
def test_class_case_counts(seed):
    """count_all, three equal ranges and ranges of 193 positions, M in {0, 1, 3}, one handle per case (pm_reset between)"""
    c, hits = case(seed)
    try:
        pm = AC.handle(c)
    except sat_amd.PmError as e:
        if hits is None and e.code in (-6, -2):
            return                                                    # the reference rejects this option set too
        raise
    assert hits is not None, ("the oracle rejects what the library accepts", AC.describe(c))
    try:
        n = c["n"]
        for M in MS:
            check_counts(c, hits, M, pm.count_all(max_count=M), "count_all")
            check_counts(c, hits, M, AC.count_walk(pm, c, (n // 3, 2 * (n // 3), n), M), "three ranges")
            check_counts(c, hits, M, AC.count_walk(pm, c, list(range(193, n, 193)) + [n], M), "ranges of 193")
        COUNTED[seed] = pm.describe()
        pm.reset()                                                    # pm_reset clears
        counts, capped, info = pm.counts()
        assert int(counts.sum()) == 0 and int(capped.sum()) == 0 and info["tallied"] == info["skipped"] == info["bogus"] == 0
    finally:
        pm.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", COUNT_SEEDS[:40])
def test_class_case_counts_with_ranges_cut_by_the_library(seed, monkeypatch):
    """PM_DENSE_BOUND: the library scans a range in pieces (pm_api.cpp scan_range); the tallies accumulate over them"""
    c, hits = case(seed)
    assert hits is not None, AC.describe(c)
    for bound in (400, 6000, 400000):                                 # (a case with several records per position cannot get below 400 in a piece of 256 positions)
        monkeypatch.setenv("PM_DENSE_BOUND", str(bound))
        pm = AC.handle(c)
        try:
            got = {M: pm.count_all(max_count=M) for M in (0, 3)}
            break
        except sat_amd.PmError as e:
            if e.code != -2 or "smaller ranges" not in str(e) or bound == 400000:
                raise
        finally:
            pm.close()
    for M in (0, 3):
        check_counts(c, hits, M, got[M], "pieces")


@pytest.mark.gpu
def test_the_re_aligners_did_run():
    """(after the count cases above, in file order) all three re-aligners took records"""
    if len(COUNTED) < len(COUNT_SEEDS) // 2:
        pytest.skip("the cases did not run in this process")
    print("class counts: %d cases; count_all over M in %s re-aligned %d records on the device (%d of them primers of 33..64 nt under -k with long_align: "
          "pm_align_hits_wide_kernel) and %d on the host; the rule re-aligns %d" % (len(COUNTED), MS, TALLIED["device"], TALLIED["wide"], TALLIED["host"], TALLIED["rule"]))
    assert TALLIED["device"] > 0 and TALLIED["wide"] > 0 and TALLIED["host"] > 0, dict(TALLIED)
    assert TALLIED["device"] + TALLIED["host"] >= TALLIED["rule"], dict(TALLIED)


# ---- the pairing stage ----------------------------------------------------------------------------------------------------
ELIGIBLE = [s for s in SEEDS if AC.pcr_eligible(AC.class_case(s))]
_ROUNDS = {}


def rounds_of(seed):
    """the case's three expected rounds, or None where the case is left out for its density"""
    if seed not in _ROUNDS:
        c, hits = case(seed)
        _ROUNDS[seed] = None if hits is None or len(hits) > AC.PCR_DENSE else AC.pcr_expected(c, hits)
    return _ROUNDS[seed]


def test_pairing_cases_cover_the_rule():
    """(CPU) from the oracle and the pairing rule alone.  143 of the 400 seeds have a list of the form pm_pcr_setup takes (2n
    patterns, n even, the second half the reverse complements of the first: no 806R appended, no odd primer count); 9 of them
    have more than 3,000 oracle hits and are left out.  The 134 cases: 155,682 candidate pairs, 136,759 amplicons, the largest
    round 14,151 candidates; 96 cases have a survivor, 244 rounds carry deferred hits, in 82 cases a surviving hit belongs to a
    primer of 33..64 nt (9: to one of 65 nt or more)."""
    assert len(ELIGIBLE) >= 120, len(ELIGIBLE)
    f = collections.Counter()
    for seed in ELIGIBLE:
        c = AC.class_case(seed)
        rounds = rounds_of(seed)
        if rounds is None:
            f["dense"] += 1
            continue
        surv = [s for r in rounds for s in r[3]]
        f["cases"] += 1
        f["candidates"] += sum(r[4] for r in rounds)
        f["amplicons"] += len(surv)
        f["with_survivor"] += bool(surv)
        f["rounds_carried"] += sum(1 for r in rounds if r[5])
        f["wide_survivor"] += any(33 <= c["lens"][h[1] - 1] <= 64 for s in surv for h in s[:2])
    assert f["dense"] <= 15, dict(f)
    assert f["with_survivor"] >= 70 and f["rounds_carried"] >= 100 and f["wide_survivor"] >= 30, dict(f)


PAIRED = {}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", ELIGIBLE)
def test_class_case_pairing_rounds(seed):
    """amplicon_max 600, -a on odd seeds, -b where seed & 2, entries from the stream's end-of-entry characters; rounds that
    end at n // 3, 2 (n // 3) and n: held, candidates, survivors (order, both hits, both alignments, amplicon length, pair
    index, N count) against tests/pcr_rule.py on the oracle's hits and the oracle's re-alignment -- the library's host
    re-alignment is not independent of the device's for primers of 33..64 nt --, the strings against pm_align_hits_text.
    Which round a hit joins: adversarial_classes.pcr_run."""
    c, hits = case(seed)
    rounds = rounds_of(seed)
    if hits is not None and rounds is None:
        return                                                        # left out for its density (counted by the CPU test above)
    try:
        PAIRED[seed] = AC.pcr_run(c, hits, rounds)
    except sat_amd.PmError as e:
        if hits is None and e.code in (-6, -2):
            return                                                    # the reference rejects this option set too
        raise
    assert hits is not None, ("the oracle rejects what the library accepts", AC.describe(c))


NONE = 2**31 - 1


@pytest.mark.gpu
def test_seed_1129_a_long_primers_hit_without_alignment_in_a_round_with_strings():
    """Regression, found by the rounds above: seed 1129 (-k 1, exact zones, long_align clear) has three hits of primers of 41 and 67 nt
    whose re-alignment gives up at a row (start 0, editdist INT32_MAX: no alignment).  pm_align_hits_device leaves primers of
    33 nt or more to the host there, and with strings asked for the host's pm_align_hits_text form refused such a record
    ("stride too small"), so pm_pcr_pair(text=True) failed with PM_E_INVALID where the device kernels write two empty
    strings.  The records handed to the host now get the empty strings too."""
    c, hits = case(1129)
    al = AC.alignments(c, hits)
    none = [h for h, a in zip(hits, al) if AC.host_aligned(c, c["lens"][h[1] - 1]) and a == (0, h[0], NONE)]
    assert len(none) == 3 and not c["route"]["long_align"], none
    import test_gpu_align_device as AD
    pm = AC.handle(c)
    try:
        got, ops, txt = pm.align_hits_device_numpy(AD.hit_array(none), text=True)
        assert [(int(a["start"]), int(a["end"]), int(a["editdist"])) for a in got] == [(0, h[0], NONE) for h in none]
        assert ops == ["", "", ""] and txt == ["", "", ""]
        assert pm.counts()[2]["aligned_host"] == 3
    finally:
        pm.close()
    AC.pcr_run(c, hits, rounds_of(1129))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", AC.edge_seeds(SEEDS))
def test_edge_case_pairing_rounds(seed):
    """the first round at the stream start and the last at its end with 40-mers that lie over the stream's two ends
    (adversarial_classes.edge_case): the hits the host makes for the edges join the held list like any other"""
    import adversarial as A
    c = AC.edge_case(seed)
    hits = A.oracle_hits(c)
    assert hits is not None, AC.describe(c)
    if len(hits) <= AC.PCR_DENSE:
        AC.pcr_run(c, hits)


@pytest.mark.gpu
def test_the_pairing_rounds_did_run():
    if len(PAIRED) < len(ELIGIBLE) // 2:
        pytest.skip("the cases did not run in this process")
    f = collections.Counter()
    for r in PAIRED.values():
        for key in ("survivors", "candidates", "carried", "aligned_device", "aligned_host"):
            f[key] += r[key]
        f["early"] += r["early"] > 0
        f["late"] += r["late"] > 0
        f["same"] += r["same"]
        f["with_survivor"] += r["survivors"] > 0
    print("class pairing: %d cases, every round compared; in %d a hit came a round early (exact_halves / exact_bases), in %d a round late (filter_bitvec's "
          "chains); %d with the amplicons and candidate total of the rounds made from the oracle's hits alone; %d candidate pairs, %d amplicons, %d cases with "
          "one, %d rounds carried hits; re-aligned %d records on the device, %d on the host" % (
              len(PAIRED), f["early"], f["late"], f["same"], f["candidates"], f["survivors"], f["with_survivor"], f["carried"], f["aligned_device"], f["aligned_host"]))
    # (a hit comes late only where its chain ends at most 2k + 1 in front of a round's end, and only under filter_bitvec)
    assert f["late"] <= len(PAIRED) // 2 and f["same"] >= len(PAIRED) // 2, dict(f)
    assert f["with_survivor"] >= 70 and f["carried"] >= 100 and f["aligned_device"] > 0, dict(f)
