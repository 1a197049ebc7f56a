"""GPU against the ORACLE on the class-mixing adversarial cases (tests/adversarial_classes.py): tests/test_gpu_adversarial.py's
streams, option sets, knobs, record caps and ways through the library, with lists whose primers fill the narrow main class,
wide tiles (33..64 characters), the 16..19 character classes, the degenerate -w class and the bit-parallel residue at once,
and the permission bits of pm_config.long_patterns set -- all seven on three cases in four.  Every per-bit test file
(test_gpu_long_*.py, test_gpu_wild_class.py, test_gpu_edit_pair.py) sets its own bit alone on lists made for it; here the
classes share one record buffer, the suspect counters, the regrow-and-rescan loop and one finalize on hit-dense text.  The
oracle is pinned to the real reference at these shapes by tests/test_oracle_vs_ref_classes.py."""
import collections

import numpy as np
import pytest

import adversarial as A
import adversarial_classes as AC
import sat_amd
import test_gpu_align_device as AD

SEEDS = list(range(900, 1300))                                    # (the range: every condition of the two coverage tests holds with a margin)
AUTO = sat_amd.KERNEL_AUTO

# describe() phrases of the routes (csrc/pm_api.cpp pm_describe; the per-bit test files assert the same ones)
WIDE = {"pair": "(pm_pair_verify_wide, wide tiles=", "exact": "(wide rows, wide tiles=", "edits": "(pm_edits_verify_wide, wide tiles=",
        "halves": "(pm_half_verify_wide, wide tiles="}
WILD, SHORT_EDIT, SHORT_SUB, RESIDUE = "pm_wild_sub_scan", "pm_short_edit_scan for", "pm_short_sub_scan for", "the seed plan does not take"
EDIT_PAIR = "kernel=pm_pair_edit_scan+pm_pair_edit_resolve+"

_WANT = {}


def case(seed):
    """(the case, the oracle's hits or None), computed once per seed and shared by the tests below"""
    c = AC.class_case(seed)
    if seed not in _WANT:
        _WANT[seed] = A.oracle_hits(c)
    return c, _WANT[seed]


def routes_named(d):
    """the routes a describe() text names"""
    out = set(name for name, phrase in WIDE.items() if phrase in d)
    if WILD in d:
        out.add("wild")
    if SHORT_EDIT in d:
        out.add("short_edit")
    if SHORT_SUB in d:
        out.add("short_sub")
    if d.startswith(EDIT_PAIR) and (" tiles=1 " not in d.split(" with ")[0] or " tests=2 " in d):
        out.add("edit_pair")                                          # more than one tile, or -k 1: what the bit adds to -k 2 on one tile
    classes = len(out & set(WIDE)) > 0, "wild" in out, bool(out & {"short_edit", "short_sub"}), RESIDUE in d
    if RESIDUE in d and any(classes[:3]):
        out.add("residue")
    return out, sum(classes)


def differ(c, got, want, note=""):
    sg, sw = set(got), set(want)
    return "%s [%s]%s: %d hits, oracle %d; only GPU %s; only oracle %s" % (
        AC.describe(c), c["kernel_desc"][:50], note, len(got), len(want), sorted(sg - sw)[:6], sorted(sw - sg)[:6])


def test_class_cases_cover_the_space():
    """(CPU) the fixed seeds reach every style, mode, engine, option, knob and record cap at least twice, and the oracle's
    hits reach the classes: conditions on the generator and the seed range, checked against the oracle alone"""
    seen = collections.Counter()
    accepted = rejected = long_hit = short_hit = degenerate_hit = 0
    for seed in SEEDS:
        c, want = case(seed)
        assert 600 <= c["n"] <= 8000 and 8 <= len(c["patterns"]) <= 162 and set(c["route"]) == set(AC.BITS)
        seen["style%d" % c["style"]] += 1
        seen["mode%d" % c["mode"]] += 1
        seen["sem_" + c["sname"]] += 1
        seen["k%d%s" % (c["k"], "e" if c["indels"] else "")] += 1
        seen["cap%d" % c["cap"]] += 1
        for f in ("zones", "wild", "with_n", "raw", "host"):
            seen[f] += bool(c[f])
        seen["eos0"] += bool(c["table"] and c["table"][:1] == b"\n")
        seen["all_bits"] += all(c["route"].values())
        for b in AC.BITS:
            seen["without_" + b] += not c["route"][b]
        for e, v in c["env"].items():
            seen[e + "=" + v] += 1
        for p in c["patterns"]:
            seen["kind_" + AC.kind(p)] += 1
        if want is None:
            rejected += 1
            continue
        accepted += 1
        lens = set(c["lens"][pid - 1] for _, pid, _ in want)
        long_hit += any(33 <= L <= 64 for L in lens)
        short_hit += any(16 <= L <= 19 for L in lens)
        degenerate_hit += any(AC.kind(c["patterns"][pid - 1]) == "degenerate" and 16 <= c["lens"][pid - 1] <= 32 for pid in set(h[1] for h in want))
    need = ["style0", "style1", "style2", "style3", "mode0", "mode1", "mode2", "mode3", "sem_auto", "sem_sai", "sem_fbv", "sem_halves", "sem_bases",
            "k0", "k1", "k1e", "k2", "k2e", "zones", "wild", "with_n", "raw", "host", "eos0", "cap1024", "cap16384", "cap1048576",
            "kind_plain", "kind_expanded", "kind_degenerate"]
    need += ["%s=%s" % (name, v) for name, vals in A.KNOBS for v in set(vals) if v is not None] + ["without_" + b for b in AC.BITS]
    assert all(seen[x] >= 2 for x in need), {x: seen[x] for x in need}
    assert 0.65 * len(SEEDS) <= seen["all_bits"] <= 0.85 * len(SEEDS), seen["all_bits"]
    assert rejected <= len(SEEDS) // 20, rejected
    assert long_hit >= 0.8 * accepted and short_hit >= 0.8 * accepted, (accepted, long_hit, short_hit)
    assert degenerate_hit >= 40, degenerate_hit


DESCRIBED = {}                                                        # seed -> describe() of the handle that gave the compared hits
FALLBACK = {}                                                         # seed -> the case's mode where it fell back to the resumable scan
RAN = collections.Counter()                                           # cases per mode that gave hits


def run_case(seed):
    c, want = case(seed)
    try:
        got = A.gpu_hits(c, kernel=AUTO, route=c["route"])
    except sat_amd.PmError as e:
        if want is None and e.code in (-6, -2):
            return                                                    # the reference rejects this option set too (select.cc:87-90)
        if e.code != -2 or c["mode"] < 2:
            raise
        # the device finalize / the owned-shard form does not take this option set (or a chain crosses the shard's guard
        # band): said loudly; the case still goes through the resumable scan
        FALLBACK[seed] = c["mode"]
        got = A.gpu_hits(c, kernel=AUTO, mode=1, route=c["route"])
    assert want is not None, ("the oracle rejects what the library accepts", AC.describe(c))
    DESCRIBED[seed] = c["kernel_desc"]
    RAN[c["mode"]] += 1
    assert got == want, differ(c, got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_class_case_vs_oracle(seed):
    run_case(seed)


@pytest.mark.gpu
def test_the_classes_did_run():
    """(after the cases above) the routes were taken, side by side, and modes 2 and 3 mostly in their own form: neither the
    fall-back to the resumable scan nor the routing hides a class from the comparison"""
    if len(DESCRIBED) < len(SEEDS) // 2:
        pytest.skip("the cases did not run in this process")
    named, several = collections.Counter(), 0
    for d in DESCRIBED.values():
        routes, classes = routes_named(d)
        named.update(routes)
        several += classes >= 2
    fell = collections.Counter(FALLBACK.values())
    print("class cases: %d described, routes %s, two or more non-main classes %d, modes %s, fall-backs %s" % (
        len(DESCRIBED), dict(sorted(named.items())), several, dict(sorted(RAN.items())), dict(sorted(fell.items()))))
    for name in ("pair", "exact", "edits", "halves", "wild", "edit_pair", "short_edit", "short_sub", "residue"):
        assert named[name] >= 10, (name, dict(named))
    assert several >= 30, several
    for mode in (2, 3):
        assert RAN[mode] > 0 and 2 * fell[mode] <= RAN[mode], (mode, RAN[mode], fell[mode])


SPLITS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS[:100])
def test_class_case_vs_oracle_with_ranges_cut_by_the_library(seed, monkeypatch):
    """pm_scan in three ranges, each scanned in pieces where its record lists would outgrow PM_DENSE_BOUND (pm_api.cpp
    scan_range): every class's records per piece, the same hits"""
    c, want = case(seed)
    if want is None:
        pytest.skip("the reference rejects this option set")
    for bound in (400, 6000, 400000):
        monkeypatch.setenv("PM_DENSE_BOUND", str(bound))
        stats = {}
        try:
            got = A.gpu_hits(c, kernel=AUTO, mode=0, stats=stats, route=c["route"])
            break
        except sat_amd.PmError as e:
            if e.code != -2 or "smaller ranges" not in str(e) or bound == 400000:
                raise
    SPLITS[seed] = stats.get("range_splits", 0)
    assert got == want, differ(c, got, want, " (%d cuts)" % SPLITS[seed])


@pytest.mark.gpu
def test_the_library_did_cut_class_ranges():
    if len(SPLITS) < 60:
        pytest.skip("the cases did not run in this process")
    cut = sum(1 for v in SPLITS.values() if v > 0)
    assert cut >= 8, (cut, sorted(SPLITS.items())[:40])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS[100:200])
def test_class_case_vs_oracle_in_tiny_ranges_at_the_stream_edges(seed):
    """The host-made records of the two stream ends, per class, in ranges of 1 .. 30 positions (see the test of this name in
    test_gpu_adversarial.py); 64, 66, 70 and n - 70, n - 66: a primer of 64 characters with two edits is longer than any first
    range of that test's list.  gpu_hits asserts that no hit lies beyond the scanned-to position."""
    c, want = case(seed)
    if want is None:
        pytest.skip("the reference rejects this option set")
    n = c["n"]
    got = A.gpu_hits(c, kernel=AUTO, route=c["route"],
                     cuts=[1, 3, 7, 19, 33, 60, 64, 66, 70, n // 2, n - 70, n - 66, n - 61, n - 30, n - 5, n - 3, n - 2, n - 1])
    assert got == want, differ(c, got, want)


@pytest.mark.gpu
def test_oracle_hits_of_class_cases_realigned_on_the_device():
    """pm_align_hits_device with long_align: the oracle's hits of the cases with indels among the first 150 seeds, re-aligned
    on the device (the wide banded DP for primers of 33..64 characters, the host list for longer ones) against the oracle's
    own re-alignment and against the host's pm_align_hits / pm_align_hits_text"""
    cases = hits_long = longer_cases = total = 0
    for seed in SEEDS[:150]:
        c, want_hits = case(seed)
        if not (c["indels"] and c["k"] >= 1) or not want_hits:
            continue
        cases += 1
        total += len(want_hits)
        hits = AD.hit_array(want_hits)
        pm = AD.make_handle(c, route=dict(c["route"], long_align=True))
        try:
            al, ops, txt = pm.align_hits_device_numpy(hits, text=True)
            want = AD.oracle_alignments(c, want_hits)
            for i, (st, en, ed, _) in enumerate(want):
                assert (int(al["start"][i]), int(al["end"][i]), int(al["editdist"][i])) == (st, en, ed), (AC.describe(c), want_hits[i], al[i], want[i])
            AD.check_against_host(pm, hits, al, ops, txt, AC.describe(c))
            _, _, info = pm.counts()
        finally:
            pm.close()
        lens = np.array(c["lens"])[hits["pid"].astype(np.int64) - 1]
        hits_long += int(((lens >= 33) & (lens <= 64)).sum())
        if (lens >= 65).any():
            longer_cases += 1
            assert info["aligned_host"] >= int((lens >= 65).sum()), (AC.describe(c), info)
    print("class align_device: %d cases, %d hits, %d of primers of 33..64 characters, %d cases with a hit of a longer primer" % (cases, total, hits_long, longer_cases))
    assert hits_long >= 1000 and longer_cases >= 1, (cases, total, hits_long, longer_cases)
