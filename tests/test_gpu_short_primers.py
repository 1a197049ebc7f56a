"""GPU: primers of 16..19 characters under -k 1 / -k 2 on pm_short_edit_scan (csrc/pm_short.hip).

The edit plan's main class seeds on the last 20 pattern bases; shorter primers used to be "patterns the seed plan does
not take" and went to the bit-parallel residue kernel.  They are now a class of their own: the last 16 bases as four
fields of four, the pair-edit plan's 14 (field pair, displacement) tests, a q-gram count, the k-error automaton.  Here:
every text within two edits of a 16-, 17-, 18- and 19-mer (completeness is decided by this test, not by argument), a
mixed list on text with repeats through every interface, the stream's edges, the routing rules, the candidate records
against the bit-parallel kernel's, and a class cut into two tiles.  Expected values come from the oracle."""
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
from test_gpu_exhaustive import TABLE, edit_variants, entry_bounds, stream_of
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


def rand_seq(rng, n):
    return "".join(rng.choice(BASES, size=n).tolist())


def planted(rng, ents, n, lo, hi, frac=0.9):
    """n primers of lo..hi characters, most of them windows of the text with up to two edits (synth.make_patterns; its
    insertions and deletions change a primer's length: only those still inside lo..hi are kept)"""
    out = []
    while len(out) < n:
        out += [p for p in synth.make_patterns(rng, ents, n, length=hi, minlen=lo, planted=frac, indel_frac=0.5, extras=False) if lo <= len(p) <= hi]
    return out[:n]


def engine(pats, k, sem=sat_amd.SEM_AUTO, kernel=sat_amd.KERNEL_AUTO):
    pm = sat_amd.PatternMatch(k=k, indels=True, semantics=sem, kernel=kernel)
    for i, p in enumerate(pats):
        pm.add_pattern(p, i + 1)
    return pm


def oracle_hits(codes, table, pats, k, sem):
    text = O.Text(codes, table)
    eng = {sat_amd.SEM_AUTO: None, sat_amd.SEM_SHIFT_AND_INEXACT: O.SHIFT_AND_INEXACT, sat_amd.SEM_FILTER_BITVEC: 5}[sem]
    if eng is None:
        eng = O.pick_engine(text, pats, k, True)
    return O.sorted_tuples(O.find_all(text, pats, engine=eng, k=k, indels=True))


# ---- 1. exhaustive ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [16, 17, 18, 19])
def test_every_text_within_two_edits_of_a_short_primer(L):
    rng = np.random.default_rng(300 + L)
    p = PATTERNS[L]
    variants = sorted(edit_variants(p, 2))
    if L == 16:
        assert len(variants) == 5890
    if L == 19:
        assert len(variants) == 8378
    parts = stream_of(variants, rng)
    codes = synth.normalize(synth.stream(parts), TABLE)
    decoys = [rand_seq(rng, 20) for _ in range(1500)] + [rand_seq(rng, int(rng.integers(16, 20))) for _ in range(500)]
    pats = [p] + decoys
    bounds = entry_bounds(parts)
    for k, sem in ((2, sat_amd.SEM_AUTO), (2, sat_amd.SEM_SHIFT_AND_INEXACT), (1, sat_amd.SEM_FILTER_BITVEC)):
        want = oracle_hits(codes, TABLE, pats, k, sem)
        pm = engine(pats, k, sem)
        try:
            pm.init(codes, TABLE)
            assert pm.selected()[1] == sat_amd.KERNEL_SEED
            d = pm.describe()
            assert "does not take" not in d, d
            assert "pm_short_edit_scan for 501 patterns of 16..19 characters" in d, d
            got = sat_amd.sorted_tuples(pm.find_all())
            stats = pm.scan_stats()
        finally:
            pm.close()
        print("exhaustive L %d k %d sem %d: %d hits (oracle %d), between stages %d [%s]" % (L, k, sem, len(got), len(want), stats["between_stages"], d))
        assert got == want, (L, k, sem, len(got), len(want))
        own = [(e, dist) for e, pid, dist in want if pid == 1]
        if k == 2:                                                   # conditions on the oracle's own output: every variant is found, at every distance
            ends = np.array(sorted({e for e, _ in own}))
            for (a, b) in bounds:
                i = np.searchsorted(ends, a, side="right")
                assert i < ends.size and ends[i] <= b, (L, sem, a, b)
        if k == 2 and sem == sat_amd.SEM_AUTO:
            assert {dist for _, dist in own} == {0, 1, 2}
        if k == 2 and sem == sat_amd.SEM_SHIFT_AND_INEXACT:          # at least one candidate of pattern 1 inside every entry
            ends = np.array(sorted({e for e, pid, _ in got if pid == 1}))
            for (a, b) in bounds:
                i = np.searchsorted(ends, a, side="right")
                assert i < ends.size and ends[i] <= b, (L, a, b)


# ---- 2. a mixed list on text with repeats, through every interface -----------------------------------------------------
_MIXED = {}


def mixed_case():
    """120 planted 21..24-mers and 60 planted 16..19-mers with indels, both strands, on synth text with repeats and N runs;
    the oracle's hits are computed once"""
    if not _MIXED:
        rng = np.random.default_rng(77)
        ents = synth.make_entries(rng, 3, 12000, n_runs=3, repeats=True, short=True)
        long_p = planted(rng, ents, 120, 21, 24)
        long_p[1], long_p[3] = long_p[0], synth.revcomp(long_p[0])   # a duplicate and a reverse-complement pair
        short_p = planted(rng, ents, 60, 16, 19)
        short_p[1] = short_p[0]
        pats = long_p + short_p
        allp = pats + [synth.revcomp(p) for p in pats]
        table = synth.table_for(ents)
        codes = synth.normalize(synth.stream(ents), table)
        want = oracle_hits(codes, table, allp, 2, sat_amd.SEM_AUTO)
        _MIXED.update(ents=ents, pats=allp, table=table, codes=codes, want=want)
    return _MIXED


def test_mixed_list_condition():
    """the oracle reports a hit of a short primer at each of the distances 0, 1, 2"""
    c = mixed_case()
    dists = {dist for _, pid, dist in c["want"] if len(c["pats"][pid - 1]) < 20}
    assert dists == {0, 1, 2}, dists
    assert any(len(c["pats"][pid - 1]) >= 20 for _, pid, _ in c["want"])


@pytest.mark.parametrize("chunk", [1 << 26, 5000, 193])
def test_mixed_list_find_all(chunk):
    c = mixed_case()
    pm = engine(c["pats"], 2)
    try:
        pm.init(c["codes"], c["table"])
        assert pm.selected() == (sat_amd.SEM_FILTER_BITVEC, sat_amd.KERNEL_SEED)
        d = pm.describe()
        assert "pm_short_edit_scan for 120 patterns" in d and "does not take" not in d, d
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
    finally:
        pm.close()
    assert got == c["want"], (chunk, len(got), len(c["want"]))


def test_mixed_list_device_stages():
    """scan_candidates + finalize_device: the device cluster stage takes the short primers' records"""
    c = mixed_case()
    n = c["codes"].size
    pm = engine(c["pats"], 2)
    try:
        pm.init(c["codes"], c["table"])
        pm.scan_candidates(0, n, to_host=False)
        got = sat_amd.sorted_tuples(pm.finalize_device(n))
        assert got == c["want"]
        pm.reset()                                                   # two ranges: the clusters at the cut are carried
        pm.scan_candidates(0, n // 2, to_host=False)
        first = sat_amd.sorted_tuples(pm.finalize_device(n // 2, last=False))
        pm.scan_candidates(n // 2, n, to_host=False)
        second = sat_amd.sorted_tuples(pm.finalize_device(n))
        assert sorted(first + second) == c["want"]
    finally:
        pm.close()


@pytest.mark.parametrize("packed,windowed", [(False, True), (True, False), (True, True)])
def test_mixed_list_windowed_and_packed(packed, windowed):
    c = mixed_case()
    n = c["codes"].size
    window = min_window(c["pats"], 2, True) if windowed else None
    pm = engine(c["pats"], 2)
    try:
        if packed:
            bits = max(1, (len(c["table"]) - 1).bit_length())
            pm.init_packed(sat_amd.pack_codes(c["codes"], bits), bits, n, c["table"], window=window)
        else:
            pm.init(c["codes"], c["table"], window=window)
        assert "pm_short_edit_scan" in pm.describe()
        got = sat_amd.sorted_tuples(pm.find_all(chunk=700 if windowed else 1 << 26))
        res = pm.residency()
    finally:
        pm.close()
    if windowed:
        assert res["window"] > 0 and res["loads"] > 1, res
    if packed:
        assert res["bits"] > 0, res
    assert got == c["want"], (packed, windowed, len(got), len(c["want"]))


@pytest.mark.parametrize("M", [0, 3])
def test_mixed_list_counts(M):
    c = mixed_case()
    if "eds" not in c:
        text = O.Text(c["codes"], c["table"])
        c["eds"] = [O.cli_align(text, c["pats"][pid - 1], end, 2, True)[3] for end, pid, _ in c["want"]]
    wc, wcap, winfo = count_rule.tally(c["want"], lambda i: c["eds"][i], len(c["pats"]), 2, M)
    pm = engine(c["pats"], 2)
    try:
        pm.init(c["codes"], c["table"])
        counts, capped, info = pm.count_all(max_count=M)
    finally:
        pm.close()
    assert counts.tolist() == wc
    assert capped.tolist() == wcap
    for f in ("tallied", "skipped", "bogus"):
        assert info[f] == winfo[f], (f, info[f], winfo[f])
    assert info["aligned_host"] == 0, info


# ---- 3. the stream's edges ------------------------------------------------------------------------------------------
def edge_primers(text_at, L, rng):
    """the primer cut from the text, the same with its first / last character missing from the text, and with a substitution"""
    t = text_at
    other = lambda ch: BASES[(BASES.index(ch) + 1 + int(rng.integers(0, 3))) % 4]
    mid = L // 2
    return [t, other(t[0]) + t[:-1], t[1:] + other(t[-1]), t[:mid] + other(t[mid]) + t[mid + 1:]]


@pytest.mark.parametrize("L", [16, 17, 18, 19])
def test_stream_edges(L):
    rng = np.random.default_rng(500 + L)
    e0, e1, e2 = rand_seq(rng, 70), rand_seq(rng, 45), rand_seq(rng, 60)
    raw = (e0 + "\n" + e1 + "\n" + e2).encode()                      # the stream starts and ends with a base
    codes = synth.normalize(raw, TABLE)
    sites = [e0[:L], e2[-L:], e1[:L], e0[-L:]]                       # first / last L bases of the stream, right behind / right in front of an end-of-sequence character
    shorts = [p for t in sites for p in edge_primers(t, L, rng)]
    for with_main in (False, True):
        pats = shorts + ([rand_seq(rng, 22) for _ in range(5)] + [e1[10:32]] if with_main else [])
        for k, sem in ((2, sat_amd.SEM_AUTO), (2, sat_amd.SEM_SHIFT_AND_INEXACT), (1, sat_amd.SEM_SHIFT_AND_INEXACT)):
            want = oracle_hits(codes, TABLE, pats, k, sem)
            assert {pid for _, pid, _ in want} >= {1, 5, 9, 13}          # the exact occurrences at least
            for chunk in (1 << 26, 37):
                pm = engine(pats, k, sem)
                try:
                    pm.init(codes, TABLE)
                    assert pm.selected()[1] == sat_amd.KERNEL_SEED and "pm_short_edit_scan" in pm.describe()
                    got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
                finally:
                    pm.close()
                assert got == want, (L, with_main, k, sem, chunk, got, want)


DENSE_UNIT = PATTERNS[16]


def dense_case():
    """a stream where one wave queues more key hits than its queue holds: a homopolymer (every window of it has every
    test's key, and one key's run holds four patterns) and a tandem repeat of a 16-mer, about 10,000 bases"""
    raw = ("T" * 50 + "A" * 5000 + "\n" + DENSE_UNIT * 300 + "C" * 40).encode()
    u = DENSE_UNIT
    pats = ["A" * 16, "A" * 17, "A" * 18, "A" * 19, u, u[3:] + u[:3], u + "ACG", "A" * 22, u + u[:6]]
    return synth.normalize(raw, TABLE), pats


def test_dense_stream():
    """the wave's queue fills between two rounds of one block (k = 2: one round queues exactly the queue's capacity inside
    the homopolymer, the next one drains mid-block) and at a block's end (k = 1); a range edge inside the homopolymer"""
    codes, pats = dense_case()
    for k, sem in ((2, sat_amd.SEM_AUTO), (2, sat_amd.SEM_SHIFT_AND_INEXACT), (1, sat_amd.SEM_SHIFT_AND_INEXACT)):
        want = oracle_hits(codes, TABLE, pats, k, sem)
        assert {pid for _, pid, _ in want} == set(range(1, len(pats) + 1))   # every pattern has hits
        for chunk in (1 << 26, 1500):
            pm = engine(pats, k, sem)
            try:
                pm.init(codes, TABLE)
                d = pm.describe()
                assert pm.selected()[1] == sat_amd.KERNEL_SEED and "pm_short_edit_scan for 7 patterns of 16..19 characters" in d, d
                got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
            finally:
                pm.close()
            assert got == want, (k, sem, chunk, len(got), len(want))


@pytest.mark.parametrize("L", [16, 19])
def test_tiny_streams(L):
    rng = np.random.default_rng(600 + L)
    p = rand_seq(rng, L)
    pats = [p, rand_seq(rng, L), p[:9] + rand_seq(rng, L - 9)]
    for raw in (p[:10], p, p[1:], p[:-2]):                           # shorter than 16 bases; exactly L bases; the primer with an end missing
        codes = synth.normalize(raw.encode(), TABLE)
        for k, sem in ((2, sat_amd.SEM_AUTO), (2, sat_amd.SEM_SHIFT_AND_INEXACT), (1, sat_amd.SEM_SHIFT_AND_INEXACT)):
            want = oracle_hits(codes, TABLE, pats, k, sem)
            pm = engine(pats, k, sem)
            try:
                pm.init(codes, TABLE)
                assert pm.selected()[1] == sat_amd.KERNEL_SEED
                got = sat_amd.sorted_tuples(pm.find_all())
            finally:
                pm.close()
            assert got == want, (L, raw, k, sem, got, want)
    codes = synth.normalize(p.encode(), TABLE)
    assert (L, 1, 0) in oracle_hits(codes, TABLE, pats, 2, sat_amd.SEM_SHIFT_AND_INEXACT)


# ---- 4. routing --------------------------------------------------------------------------------------------------------
def routing_case():
    rng = np.random.default_rng(9)
    ents = synth.make_entries(rng, 2, 6000)
    codes = synth.normalize(synth.stream(ents), TABLE)
    shorts = planted(rng, ents, 40, 16, 19, 0.8)
    return ents, codes, shorts


def test_routing():
    ents, codes, shorts = routing_case()
    rng = np.random.default_rng(10)

    def selected(pats, **kw):
        pm = engine(pats, 2, **kw)
        try:
            pm.init(codes, TABLE)
            return pm.selected()[1], pm.describe(), sat_amd.sorted_tuples(pm.find_all())
        finally:
            pm.close()

    # an all-short list: the short engine alone
    kern, d, got = selected(shorts)
    assert kern == sat_amd.KERNEL_SEED and d.startswith("kernel=pm_short_edit_scan+pm_edits_verify for 40 patterns of 16..19 characters"), d
    assert got == oracle_hits(codes, TABLE, shorts, 2, sat_amd.SEM_AUTO)
    # all-short plus one primer with an N: nothing for the main class, something for the residue -> one engine
    withn = shorts + ["ACGTNACGTTGACCATGA"]
    kern, d, got = selected(withn)
    assert kern == sat_amd.KERNEL_BITPAR and "pm_short_edit_scan" not in d, d
    assert got == oracle_hits(codes, TABLE, withn, 2, sat_amd.SEM_AUTO)
    # the seed family on request takes 18-mers, alone and beside 22-mers
    p18 = [p for p in shorts if len(p) == 18] + [rand_seq(rng, 18)]
    for pats in (p18, p18 + [ents[0][100:122], rand_seq(rng, 22)]):
        kern, d, got = selected(pats, kernel=sat_amd.KERNEL_SEED)
        assert kern == sat_amd.KERNEL_SEED and "pm_short_edit_scan" in d, d
        assert got == oracle_hits(codes, TABLE, pats, 2, sat_amd.SEM_AUTO)
    with pytest.raises(sat_amd.PmError) as e:                        # ... and still no 15-mer
        selected(p18 + ["ACGTTGCAAGCTTAG"], kernel=sat_amd.KERNEL_SEED)
    assert e.value.code == -2
    # a 15-mer in a mixed list is still the residue's
    mixed = shorts + [ents[1][50:72], rand_seq(rng, 22), ents[0][300:315]]
    kern, d, got = selected(mixed)
    assert kern == sat_amd.KERNEL_SEED, d
    assert "for 1 patterns the seed plan does not take" in d and "pm_short_edit_scan for 40 patterns of 16..19 characters" in d, d
    assert got == oracle_hits(codes, TABLE, mixed, 2, sat_amd.SEM_AUTO)


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
pm = sat_amd.PatternMatch(k=2, indels=True)
for i, p in enumerate(c["pats"]):
    pm.add_pattern(p, i + 1)
pm.init(np.array(c["codes"], dtype=np.uint8), c["table"].encode())
out = {"kernel": pm.selected()[1], "describe": pm.describe(), "hits": [[int(x) for x in h] for h in sat_amd.sorted_tuples(pm.find_all())]}
pm.close()
print("RESULT " + json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_short_scan_knob_sends_the_class_back_to_the_residue(tmp_path):
    """PM_SHORT_SCAN=bitpar in a fresh process (the environment is read by pm_create): the description of before, the same hits"""
    ents, codes, shorts = routing_case()
    pats = shorts + [ents[1][50:72], ents[0][900:922]]
    case = tmp_path / "case.json"
    case.write_text(json.dumps({"pats": pats, "codes": codes.tolist(), "table": TABLE.decode()}))
    env = dict(os.environ, PM_SHORT_SCAN="bitpar")
    r = subprocess.run([sys.executable, "-c", CHILD, str(case)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert out["kernel"] == sat_amd.KERNEL_SEED
    assert "pm_short_edit_scan" not in out["describe"] and "for 40 patterns the seed plan does not take" in out["describe"], out["describe"]
    pm = engine(pats, 2)
    try:
        pm.init(codes, TABLE)
        assert "pm_short_edit_scan for 40 patterns" in pm.describe()
        got = sat_amd.sorted_tuples(pm.find_all())
    finally:
        pm.close()
    assert [tuple(h) for h in out["hits"]] == got
    assert got == oracle_hits(codes, TABLE, pats, 2, sat_amd.SEM_AUTO)


# ---- 5. differential: the candidate records are the bit-parallel kernel's ------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_candidate_records_equal_the_bit_parallel_kernels(k):
    c = mixed_case()
    n = c["codes"].size
    recs = {}
    for kernel in (sat_amd.KERNEL_AUTO, sat_amd.KERNEL_BITPAR):
        pm = engine(c["pats"], k, sat_amd.SEM_SHIFT_AND_INEXACT, kernel)
        try:
            pm.init(c["codes"], c["table"])
            assert pm.selected()[1] == (sat_amd.KERNEL_SEED if kernel == sat_amd.KERNEL_AUTO else sat_amd.KERNEL_BITPAR)
            r = pm.scan_candidates(0, n)
            recs[kernel] = sorted({(int(e), int(p), int(d)) for e, p, d in zip(r["end"], r["pid"], r["k"])})
        finally:
            pm.close()
    assert recs[sat_amd.KERNEL_AUTO] == recs[sat_amd.KERNEL_BITPAR]
    assert any(len(c["pats"][pid - 1]) < 20 for _, pid, _ in recs[sat_amd.KERNEL_BITPAR])


# ---- 6. a class cut into two tiles -------------------------------------------------------------------------------------
def test_two_tiles(monkeypatch):
    rng = np.random.default_rng(11)
    ents = synth.make_entries(rng, 2, 8000, n_runs=1)
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    shorts = planted(rng, ents, 200, 16, 19, 0.7)
    pats = shorts + planted(rng, ents, 20, 22, 26, 0.7)
    want = oracle_hits(codes, table, pats, 2, sat_amd.SEM_AUTO)
    assert sum(len(pats[pid - 1]) < 20 for _, pid, _ in want) >= 50
    got = {}
    for tile in (0, 128):
        if tile:
            monkeypatch.setenv("PM_SHORT_TILE", str(tile))
        pm = engine(pats, 2)
        try:
            pm.init(codes, table)
            d = pm.describe()
            assert "pm_short_edit_scan for 200 patterns of 16..19 characters (tiles=%d, tests=14)" % (2 if tile else 1) in d, d
            got[tile] = sat_amd.sorted_tuples(pm.find_all())
        finally:
            pm.close()
    assert got[0] == want and got[128] == want
