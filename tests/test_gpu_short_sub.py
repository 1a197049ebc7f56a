"""GPU: primers of 16..19 characters under -K 1 / -K 2 on pm_short_sub_scan (csrc/pm_short.hip).

The pair plan takes primers of 20..32 characters; one shorter primer used to send the whole list to the Bloom plan
(pm_seed_scan).  Primers of 16..19 characters are now a class of their own beside a main class on the pair plan: the last
16 bases as four fields of four, the plan's field pairs, 8-byte run entries, and the pair plan's exact verify with fields
of four bases.  Here: every text within two substitutions of a 16-, 17-, 18- and 19-mer, a mixed list on text with
repeats and N runs through every interface, exact zones and IUPAC letters on short primers, the stream's edges, the
candidate records against the former route's (PM_SHORT_SUB=off), a class cut into tiles, and the routing rules.
Expected values come from the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import count_rule
import sat_amd
import synth
from oracle import pmoracle as O
from test_gpu_exhaustive import TABLE, entry_bounds, stream_of, substitution_variants
from test_gpu_short_primers import dense_case
from test_gpu_windowed import min_window

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = list("ACGT")
PATTERNS = {
    16: "ACGTTGCAAGCTTAGG",
    17: "ACGTTGCAAGCTTAGGC",
    18: "ACGTTGCAAGCTTAGGCT",
    19: "ACGTTGCAAGCTTAGGCTC",
}
# option sets: (k, semantics asked for, semantics selected, the oracle's engine; None = its automatic choice)
BITVEC2 = (2, sat_amd.SEM_AUTO, sat_amd.SEM_FILTER_BITVEC, None)
INEXACT2 = (2, sat_amd.SEM_SHIFT_AND_INEXACT, sat_amd.SEM_SHIFT_AND_INEXACT, O.SHIFT_AND_INEXACT)
BITVEC1 = (1, sat_amd.SEM_FILTER_BITVEC, sat_amd.SEM_FILTER_BITVEC, 5)
HALVES1 = (1, sat_amd.SEM_AUTO, sat_amd.SEM_EXACT_HALVES, None)


def rand_seq(rng, n):
    return "".join(rng.choice(BASES, size=n).tolist())


def engine(pats, k, sem=sat_amd.SEM_AUTO, kernel=sat_amd.KERNEL_AUTO, zones=None, indels=False, wildcards=False):
    pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sem, kernel=kernel, wildcards=wildcards)
    for i, p in enumerate(pats):
        z = zones[i] if zones else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    return pm


def oracle_hits(codes, table, pats, k, eng, zones=None, wildcards=False):
    text = O.Text(codes, table)
    E = [z[0] for z in zones] if zones else None
    F = [z[1] for z in zones] if zones else None
    if eng is None:
        eng = O.pick_engine(text, pats, k, False, E, F)
    return O.sorted_tuples(O.find_all(text, pats, engine=eng, k=k, indels=False, esb=E, eeb=F, wildcards=wildcards))


# ---- 1. exhaustive ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [16, 17, 18, 19])
def test_every_text_within_two_substitutions_of_a_short_primer(L):
    rng = np.random.default_rng(800 + L)
    p = PATTERNS[L]
    variants = sorted(set().union(*(substitution_variants(p, k) for k in (0, 1, 2))))
    if L == 16:
        assert len(variants) == 1129
    if L == 19:
        assert len(variants) == 1597
    parts = stream_of(variants, rng)
    codes = synth.normalize(synth.stream(parts), TABLE)
    decoys = [rand_seq(rng, 20) for _ in range(1500)] + [rand_seq(rng, int(rng.integers(16, 20))) for _ in range(500)]
    pats = [p] + decoys
    bounds = entry_bounds(parts)
    for k, sem, selected, eng in (BITVEC2, INEXACT2, BITVEC1, HALVES1):
        want = oracle_hits(codes, TABLE, pats, k, eng)
        pm = engine(pats, k, sem)
        try:
            pm.init(codes, TABLE)
            assert pm.selected() == (selected, sat_amd.KERNEL_SEED)
            d = pm.describe()
            assert "pm_pair_scan" in d and "pm_short_sub_scan for 501 patterns of 16..19 characters" in d and "does not take" not in d, d
            got = sat_amd.sorted_tuples(pm.find_all())
            stats = pm.scan_stats()
        finally:
            pm.close()
        print("exhaustive L %d k %d sem %d: %d hits (oracle %d), between stages %d [%s]" % (L, k, sem, len(got), len(want), stats["between_stages"], d))
        assert got == want, (L, k, sem, len(got), len(want))
        if k == 2:                                                   # conditions on the oracle's own output
            own = [(e, dist) for e, pid, dist in want if pid == 1]
            ends = np.array(sorted({e for e, _ in own}))
            for (a, b) in bounds:
                i = np.searchsorted(ends, a, side="right")
                assert i < ends.size and ends[i] <= b, (L, sem, a, b)
            assert {dist for _, dist in own} == {0, 1, 2}


# ---- 2. a mixed list on text with repeats and N runs, through every interface ------------------------------------------
_MIXED = {}
MIXED_OPTS = {"bitvec2": BITVEC2, "inexact2": INEXACT2, "halves1": HALVES1}


def mixed_case():
    """120 planted 21..24-mers and 60 planted 16..19-mers (substitutions only), both strands, a duplicate and a
    reverse-complement pair among the short ones, on synth text with repeats and N runs; the oracle's hits of every
    option set are computed once"""
    if not _MIXED:
        rng = np.random.default_rng(78)
        ents = synth.make_entries(rng, 3, 12000, n_runs=3, repeats=True, short=True)
        long_p = synth.make_patterns(rng, ents, 120, length=24, minlen=21, planted=0.9, indel_frac=0, extras=False)
        short_p = synth.make_patterns(rng, ents, 60, length=19, minlen=16, planted=0.9, indel_frac=0, extras=False)
        short_p[1], short_p[3] = short_p[0], synth.revcomp(short_p[0])
        pats = long_p + short_p
        allp = pats + [synth.revcomp(p) for p in pats]
        table = synth.table_for(ents)
        codes = synth.normalize(synth.stream(ents), table)
        _MIXED.update(ents=ents, pats=allp, table=table, codes=codes, want={})
    return _MIXED


def mixed_want(name):
    c = mixed_case()
    if name not in c["want"]:
        k, _, _, eng = MIXED_OPTS[name]
        c["want"][name] = oracle_hits(c["codes"], c["table"], c["pats"], k, eng)
    return c["want"][name]


def mixed_engine(name, pats=None):
    c = mixed_case()
    k, sem, _, _ = MIXED_OPTS[name]
    return engine(c["pats"] if pats is None else pats, k, sem)


def check_mixed_route(pm, name):
    d = pm.describe()
    assert pm.selected() == (MIXED_OPTS[name][2], sat_amd.KERNEL_SEED), d
    assert "pm_pair_scan" in d and "pm_short_sub_scan for 120 patterns of 16..19 characters" in d and "does not take" not in d, d


def test_mixed_list_condition():
    """the oracle reports hits of short primers at each of the distances 0, 1, 2, and hits of long ones"""
    c = mixed_case()
    want = mixed_want("bitvec2")
    assert {dist for _, pid, dist in want if len(c["pats"][pid - 1]) < 20} == {0, 1, 2}
    assert any(len(c["pats"][pid - 1]) >= 20 for _, pid, _ in want)
    for name in ("inexact2", "halves1"):
        assert any(len(c["pats"][pid - 1]) < 20 for _, pid, _ in mixed_want(name))


@pytest.mark.parametrize("name", list(MIXED_OPTS))
@pytest.mark.parametrize("chunk", [1 << 26, 5000, 193])
def test_mixed_list_find_all(name, chunk):
    c = mixed_case()
    want = mixed_want(name)
    pm = mixed_engine(name)
    try:
        pm.init(c["codes"], c["table"])
        check_mixed_route(pm, name)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
    finally:
        pm.close()
    assert got == want, (name, chunk, len(got), len(want))


@pytest.mark.parametrize("name", list(MIXED_OPTS))
def test_mixed_list_device_stages(name):
    """scan_candidates + finalize_device: pm_cluster_reduce, the exact_halves rule and the automaton's pass-through take
    the short primers' records: in one range, and for the first and the last in two ranges and position-sharded"""
    c = mixed_case()
    want = mixed_want(name)
    n = c["codes"].size
    pm = mixed_engine(name)
    try:
        pm.init(c["codes"], c["table"])
        pm.scan_candidates(0, n, to_host=False)
        assert sat_amd.sorted_tuples(pm.finalize_device(n)) == want
        if name != "halves1":                                        # (exact_halves' rule on the device takes the whole range in one call)
            pm.reset()                                               # two ranges: what is open at the cut is carried
            pm.scan_candidates(0, n // 2, to_host=False)
            first = sat_amd.sorted_tuples(pm.finalize_device(n // 2, last=False))
            pm.scan_candidates(n // 2, n, to_host=False)
            second = sat_amd.sorted_tuples(pm.finalize_device(n))
            assert sorted(first + second) == want
            cut, guard, parts = n // 3 + 5, 200, []                  # position shards with guard margins
            for own_lo, own_hi in ((0, cut), (cut, n)):
                g_lo, g_hi = max(0, own_lo - guard), min(n, own_hi + guard)
                pm.reset()
                pm.scan_candidates(g_lo, g_hi, to_host=False)
                parts += sat_amd.sorted_tuples(pm.finalize_device(0, sort=True, owned=(own_lo, own_hi, g_lo, None if g_hi == n else g_hi)))
            assert sorted(parts) == want
    finally:
        pm.close()


@pytest.mark.parametrize("packed,windowed", [(False, True), (True, False), (True, True)])
def test_mixed_list_windowed_and_packed(packed, windowed):
    c = mixed_case()
    want = mixed_want("bitvec2")
    n = c["codes"].size
    window = min_window(c["pats"], 2, False) if windowed else None
    pm = mixed_engine("bitvec2")
    try:
        if packed:
            bits = max(1, (len(c["table"]) - 1).bit_length())
            pm.init_packed(sat_amd.pack_codes(c["codes"], bits), bits, n, c["table"], window=window)
        else:
            pm.init(c["codes"], c["table"], window=window)
        check_mixed_route(pm, "bitvec2")
        got = sat_amd.sorted_tuples(pm.find_all(chunk=700 if windowed else 1 << 26))
        res = pm.residency()
    finally:
        pm.close()
    if windowed:
        assert res["window"] > 0 and res["loads"] > 1, res
    if packed:
        assert res["bits"] > 0, res
    assert got == want, (packed, windowed, len(got), len(want))


@pytest.mark.parametrize("M", [0, 1, 3])
def test_mixed_list_counts(M):
    c = mixed_case()
    want = mixed_want("bitvec2")
    if "eds" not in c:
        text = O.Text(c["codes"], c["table"])
        c["eds"] = [O.cli_align(text, c["pats"][pid - 1], end, 2, False)[3] for end, pid, _ in want]
    wc, wcap, winfo = count_rule.tally(want, lambda i: c["eds"][i], len(c["pats"]), 2, M)
    pm = mixed_engine("bitvec2")
    try:
        pm.init(c["codes"], c["table"])
        check_mixed_route(pm, "bitvec2")
        counts, capped, info = pm.count_all(max_count=M)
    finally:
        pm.close()
    assert counts.tolist() == wc
    assert capped.tolist() == wcap
    for f in ("tallied", "skipped", "bogus"):
        assert info[f] == winfo[f], (f, info[f], winfo[f])


# ---- 3. exact zones and IUPAC letters on short primers ----------------------------------------------------------------
def test_zones_on_short_primers():
    """the mixed list with exact_start_bases / exact_end_bases on every third short primer, and a primer of 18 A with
    three exact start bases on a run of A: the window that starts one base early has its substitution inside the zone,
    chains with its neighbours all the same (filter_bitvec.cc:103-116) and is never the chain's hit"""
    c = mixed_case()
    rng = np.random.default_rng(81)
    ents = c["ents"] + [rand_seq(rng, 40) + "C" + "A" * 24 + "G" + rand_seq(rng, 40)]
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    pats = c["pats"] + ["A" * 18]
    zones = [(0, 0)] * len(pats)
    for n, i in enumerate(j for j, p in enumerate(pats) if len(p) < 20):
        if n % 3 == 0:
            zones[i] = [(4, 0), (0, 5), (3, 3)][(n // 3) % 3]
    zones[-1] = (3, 0)
    apid = len(pats)
    halves = (1, sat_amd.SEM_EXACT_HALVES, sat_amd.SEM_EXACT_HALVES, 12)
    for name, (k, sem, selected, eng) in (("bitvec2", (2, sat_amd.SEM_FILTER_BITVEC, sat_amd.SEM_FILTER_BITVEC, 5)), ("bitvec1", BITVEC1), ("halves1", halves)):
        want = oracle_hits(codes, table, pats, k, eng, zones)
        if name == "bitvec2":
            # condition, from the oracle alone: a chain of the A primer's windows (the automaton's candidates, consecutive
            # ends) holds a filter_bitvec hit and a window whose mismatch lies in the exact zone
            cand = sorted(e for e, pid, _ in oracle_hits(codes, table, pats, k, O.SHIFT_AND_INEXACT) if pid == apid)
            letters = bytes(table[x] for x in codes.tolist()).decode()
            viol = {e for e in cand if any(letters[e - 18 + i] != "A" for i in range(3))}
            hits = {e for e, pid, _ in want if pid == apid}
            chains, run = [], []
            for e in cand:
                if run and e != run[-1] + 1:
                    chains.append(run)
                    run = []
                run.append(e)
            chains.append(run)
            assert any(set(ch) & viol and set(ch) & hits for ch in chains), (cand, viol, hits)
        for chunk in (1 << 26, 193):
            pm = engine(pats, k, sem, zones=zones)
            try:
                pm.init(codes, table)
                d = pm.describe()
                assert pm.selected() == (selected, sat_amd.KERNEL_SEED) and "pm_short_sub_scan for 121 patterns" in d, d
                got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
            finally:
                pm.close()
            assert got == want, (name, chunk, len(got), len(want))


def test_iupac_letters_in_short_primers():
    """-w: one and two IUPAC letters in every fourth short primer (expanded into their variants, as in the main class)"""
    c = mixed_case()
    rng = np.random.default_rng(82)
    pats = list(c["pats"][:len(c["pats"]) // 2])
    amb = 0
    for n, i in enumerate(j for j, p in enumerate(pats) if len(p) < 20):
        if n % 4 == 0:
            p = list(pats[i])
            for _ in range(1 + (n // 4) % 2):
                p[int(rng.integers(0, len(p)))] = str(rng.choice(list("RYKMSWBDHV")))
            pats[i] = "".join(p)
            amb += 1
    assert amb >= 10
    allp = pats + [synth.revcomp_iupac(q) for q in pats]
    want = O.sorted_tuples(O.find_all(O.Text(c["codes"], c["table"]), allp, engine=5, k=2, indels=False, wildcards=True, text_n=False))
    assert any(set(allp[pid - 1]) - set("ACGT") for _, pid, _ in want)     # a hit of a primer with an IUPAC letter
    for chunk in (1 << 26, 997):
        pm = engine(allp, 2, wildcards=True)
        try:
            pm.init(c["codes"], c["table"])
            d = pm.describe()
            assert pm.selected()[1] == sat_amd.KERNEL_SEED and "pm_short_sub_scan for 120 patterns" in d and "does not take" not in d, d
            got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        finally:
            pm.close()
        assert got == want, (chunk, len(got), len(want))


# ---- 4. the stream's edges ------------------------------------------------------------------------------------------
def edge_primers(t, L, rng):
    """the primer cut from the text, the same shifted by one character to either side, and with a substitution"""
    other = lambda ch: BASES[(BASES.index(ch) + 1 + int(rng.integers(0, 3))) % 4]
    mid = L // 2
    return [t, other(t[0]) + t[:-1], t[1:] + other(t[-1]), t[:mid] + other(t[mid]) + t[mid + 1:]]


@pytest.mark.parametrize("L", [16, 17, 18, 19])
def test_stream_edges(L):
    rng = np.random.default_rng(900 + L)
    e0, e1, e2 = rand_seq(rng, 70), rand_seq(rng, 45), rand_seq(rng, 60)
    raw = (e0 + "\n" + e1 + "\n" + e2).encode()                      # the stream starts and ends with a base
    codes = synth.normalize(raw, TABLE)
    n = codes.size
    # first / last L bases of the stream (the last plant leaves fewer than 32 bytes behind its start), right behind /
    # right in front of an end-of-sequence character, and straddling one
    sites = [e0[:L], e2[-L:], e1[:L], e0[-L:]]
    straddle = e0[-(L // 2):] + "A" + e1[:L - L // 2 - 1]
    shorts = [p for t in sites for p in edge_primers(t, L, rng)] + [straddle]
    pats = shorts + [rand_seq(rng, 22) for _ in range(5)] + [e1[10:32]]
    for k, sem, selected, eng in (BITVEC2, INEXACT2, BITVEC1, HALVES1):
        want = oracle_hits(codes, TABLE, pats, k, eng)
        assert {pid for _, pid, _ in want} >= {1, 5, 9, 13}          # the exact occurrences at least
        assert len(shorts) not in {pid for _, pid, _ in want}        # nothing matches across an end-of-sequence character
        for chunk in (1 << 26, 37, 3):
            pm = engine(pats, k, sem)
            try:
                pm.init(codes, TABLE)
                assert pm.selected() == (selected, sat_amd.KERNEL_SEED) and "pm_short_sub_scan" in pm.describe(), pm.describe()
                got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
                pm.reset()                                           # ranges of a few positions at both ends, through the candidate stage
                few = []
                for b, e in ((0, 3), (3, L + 2), (n - L - 1, n - 2), (n - 2, n)):
                    r = pm.scan_candidates(b, e)
                    assert all(b < x <= e or x > n for x in r["end"].tolist()), (b, e, r["end"].tolist())
                    few.append(len(r))
            finally:
                pm.close()
            assert got == want, (L, k, sem, chunk, got, want)
        assert sum(few) > 0


def test_dense_stream():
    """test_gpu_short_primers.dense_case: the wave's queue fills between two rounds of one block (k = 2: one round queues
    exactly the queue's capacity inside the homopolymer, the next one drains mid-block and the windows are then taken
    from the queuing lanes' words) and at a block's end (k = 1); a range edge inside the homopolymer"""
    codes, pats = dense_case()
    for k, sem, selected, eng in (BITVEC2, INEXACT2, BITVEC1, HALVES1):
        want = oracle_hits(codes, TABLE, pats, k, eng)
        assert {pid for _, pid, _ in want} == set(range(1, len(pats) + 1))   # every pattern has hits
        for chunk in (1 << 26, 1500):
            pm = engine(pats, k, sem)
            try:
                pm.init(codes, TABLE)
                d = pm.describe()
                assert pm.selected() == (selected, sat_amd.KERNEL_SEED) and "pm_short_sub_scan for 7 patterns of 16..19 characters" in d, d
                got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
            finally:
                pm.close()
            assert got == want, (k, sem, chunk, len(got), len(want))


@pytest.mark.parametrize("L", [16, 19])
def test_tiny_streams(L):
    """streams shorter than 32 bytes: shorter than the primer, exactly the primer, the primer with an end missing"""
    rng = np.random.default_rng(950 + L)
    p = rand_seq(rng, L)
    pats = [p, rand_seq(rng, L), p[:9] + rand_seq(rng, L - 9), rand_seq(rng, 21), p + "ACGT"]
    for raw in (p[:10], p, p[1:], p[:-2], "G" + p + "T"):
        codes = synth.normalize(raw.encode(), TABLE)
        for k, sem, selected, eng in (BITVEC2, INEXACT2, HALVES1):
            want = oracle_hits(codes, TABLE, pats, k, eng)
            pm = engine(pats, k, sem)
            try:
                pm.init(codes, TABLE)
                assert pm.selected() == (selected, sat_amd.KERNEL_SEED) and "pm_short_sub_scan" in pm.describe(), pm.describe()
                got = sat_amd.sorted_tuples(pm.find_all())
            finally:
                pm.close()
            assert got == want, (L, raw, k, sem, got, want)
    codes = synth.normalize(p.encode(), TABLE)
    assert (L, 1, 0) in oracle_hits(codes, TABLE, pats, 2, O.SHIFT_AND_INEXACT)


# ---- 5. differential: the candidate records are the former route's ----------------------------------------------------
CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r]
try:
    import torch
except Exception:
    pass
import numpy as np
import sat_amd
c = json.load(open(sys.argv[1]))
pm = sat_amd.PatternMatch(k=c["k"], indels=False, semantics=c["sem"])
for i, p in enumerate(c["pats"]):
    pm.add_pattern(p, i + 1)
codes = np.array(c["codes"], dtype=np.uint8)
pm.init(codes, c["table"].encode())
r = pm.scan_candidates(0, codes.size)
recs = sorted((int(e), int(p), int(d), int(a[0]), int(a[1]), int(a[2])) for e, p, d, a in zip(r["end"], r["pid"], r["k"], r["aux"]))
out = {"selected": list(pm.selected()), "describe": pm.describe(), "records": recs}
pm.close()
print("RESULT " + json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "tests"))


def run_child(case, env):
    r = subprocess.run([sys.executable, "-c", CHILD, str(case)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


@pytest.mark.parametrize("name", ["bitvec2", "halves1"])
def test_candidate_records_equal_the_former_routes(name, tmp_path):
    """PM_SHORT_SUB=off in a fresh process (the environment is read by pm_create): the Bloom plan's description, and the
    same candidate records, aux bytes included"""
    c = mixed_case()
    k, sem, selected, _ = MIXED_OPTS[name]
    case = tmp_path / "case.json"
    case.write_text(json.dumps({"pats": c["pats"], "codes": c["codes"].tolist(), "table": c["table"].decode(), "k": k, "sem": selected}))
    env = {x: v for x, v in os.environ.items() if x != "PM_SHORT_SUB"}
    on = run_child(case, env)
    off = run_child(case, dict(env, PM_SHORT_SUB="off"))
    assert on["selected"] == off["selected"] == [selected, sat_amd.KERNEL_SEED]
    assert "pm_short_sub_scan for 120 patterns" in on["describe"] and "pm_pair_scan" in on["describe"], on["describe"]
    assert "pm_short_sub_scan" not in off["describe"] and "pm_seed_scan" in off["describe"], off["describe"]
    assert any(len(c["pats"][r[1] - 1]) < 20 for r in on["records"]) and any(len(c["pats"][r[1] - 1]) >= 20 for r in on["records"])
    assert on["records"] == off["records"], (name, len(on["records"]), len(off["records"]))


# ---- 6. a class cut into tiles -----------------------------------------------------------------------------------------
def test_tiles(monkeypatch):
    c = mixed_case()
    want = mixed_want("bitvec2")
    monkeypatch.setenv("PM_SHORT_TILE", "64")
    pm = mixed_engine("bitvec2")
    try:
        pm.init(c["codes"], c["table"])
        d = pm.describe()
        assert "pm_short_sub_scan for 120 patterns of 16..19 characters (tiles=2, pairs=6)" in d, d
        got = sat_amd.sorted_tuples(pm.find_all())
    finally:
        pm.close()
    assert got == want


# ---- 7. routing ----------------------------------------------------------------------------------------------------------
def test_routing(monkeypatch):
    """lists and option sets the class does not apply to keep their route: describe() is byte-equal with PM_SHORT_SUB=off"""
    rng = np.random.default_rng(12)
    ents = synth.make_entries(rng, 2, 6000)
    codes = synth.normalize(synth.stream(ents), TABLE)
    longs = synth.make_patterns(rng, ents, 30, length=24, minlen=20, planted=0.8, extras=False)
    shorts = synth.make_patterns(rng, ents, 30, length=19, minlen=16, planted=0.8, extras=False)
    mixed = longs + shorts

    def outcome(pats, k=2, **kw):
        pm = engine(pats, k, **kw)
        try:
            pm.init(codes, TABLE)
            pm.scan_candidates(0, codes.size, to_host=False)         # (the description holds the launch geometry)
            return pm.selected(), pm.describe()
        except sat_amd.PmError as e:
            return e.code, str(e)
        finally:
            pm.close()

    z6 = [(6, 0)] * len(mixed)
    cases = {
        "no short primer": dict(pats=longs),
        "only short primers": dict(pats=shorts),
        "a primer of 15": dict(pats=mixed + [ents[0][300:315]]),
        "a primer of 10": dict(pats=mixed + [ents[0][400:410]]),
        "more short primers than the cap": dict(pats=mixed + [rand_seq(rng, 18) for _ in range(24001 - len(shorts))]),
        "exact_bases": dict(pats=mixed, sem=sat_amd.SEM_EXACT_BASES, zones=z6),
        "seed kernels on request": dict(pats=mixed, kernel=sat_amd.KERNEL_SEED),
        "bit-parallel kernels on request": dict(pats=mixed, kernel=sat_amd.KERNEL_BITPAR),
        "k = 0": dict(pats=mixed, k=0),
        "-k": dict(pats=mixed, indels=True),
    }
    seen = {}
    for off in (False, True):
        if off:
            monkeypatch.setenv("PM_SHORT_SUB", "off")
        else:
            monkeypatch.delenv("PM_SHORT_SUB", raising=False)
        for what, kw in cases.items():
            seen[what, off] = outcome(**kw)
        seen["mixed", off] = outcome(mixed)
        seen["mixed + residue", off] = outcome(mixed + ["ACGTNACGTTGACCATGATT", "ACGTTGCA" * 5])
    for what in cases:
        assert seen[what, False] == seen[what, True], (what, seen[what, False], seen[what, True])
        assert "pm_short_sub_scan" not in seen[what, False][1], (what, seen[what, False])
    for what in ("mixed", "mixed + residue"):
        assert "pm_pair_scan" in seen[what, False][1] and "pm_short_sub_scan for 30 patterns of 16..19 characters (tiles=1, pairs=6)" in seen[what, False][1], seen[what, False]
        assert "pm_short_sub_scan" not in seen[what, True][1] and "pm_seed_scan" in seen[what, True][1], seen[what, True]
    assert "for 2 patterns the seed plan does not take" in seen["mixed + residue", False][1], seen["mixed + residue", False]
    monkeypatch.delenv("PM_SHORT_SUB")                               # (the loop above ends with the knob off)
    at_cap = outcome(mixed + [rand_seq(rng, 18) for _ in range(24000 - len(shorts))])   # the largest class the routing takes
    assert "pm_short_sub_scan for 24000 patterns of 16..19 characters (tiles=1, pairs=6)" in at_cap[1], at_cap


def test_residue_beside_both_classes():
    """a primer with an N and one of 40 characters go to the bit-parallel kernel after both classes: the oracle's hits"""
    c = mixed_case()
    pats = c["pats"] + [c["ents"][0][500:509] + "N" + c["ents"][0][510:518], c["ents"][1][100:140]]
    want = oracle_hits(c["codes"], c["table"], pats, 2, None)
    assert {len(pats) - 1, len(pats)} & {pid for _, pid, _ in want}
    pm = engine(pats, 2)
    try:
        pm.init(c["codes"], c["table"])
        d = pm.describe()
        assert "pm_short_sub_scan for 120 patterns" in d and "for 2 patterns the seed plan does not take" in d, d
        got = sat_amd.sorted_tuples(pm.find_all(chunk=5000))
    finally:
        pm.close()
    assert got == want
