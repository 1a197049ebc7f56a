"""GPU: primers of 33..64 characters under -K 1 / -K 2 on the pair plan (pm_config.long_patterns; csrc/pm_pair.hip
pm_pair_verify_wide, csrc/pm_verify.h pair_verify<5, 64>).

The pair plan's scan looks at a primer's last 20 bases, so a primer of up to 64 characters needs no pass of its own: it
joins the plan's tiles, and a tile that holds one is verified on rows of 64 characters.  The route is a permission of the
caller (long_patterns=True), off by default.  Here: every text within two substitutions of a 33-mer and of a 64-mer, a
mixed list (20..32, 33..64, 16..19, a primer with an N, a 70-mer) on text with repeats and N runs through every
interface, the stream's edges, exact zones on either side of index 32, IUPAC letters, a list of 40-mers and 18-mers, the
routing rules, the final hits against the former route's, a wide tile beside a narrow one, and the counts with their
re-alignment on the device.  Expected values come from the oracle."""
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
from test_gpu_align_device import check_against_host, hit_array
from test_gpu_exhaustive import TABLE, entry_bounds, stream_of, substitution_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = list("ACGT")
LONG_PHRASE = "of 33..64 characters"
# option sets: (k, semantics asked for, semantics selected, the oracle's engine; None = its automatic choice)
BITVEC2 = (2, sat_amd.SEM_FILTER_BITVEC, sat_amd.SEM_FILTER_BITVEC, 5)
INEXACT2 = (2, sat_amd.SEM_SHIFT_AND_INEXACT, sat_amd.SEM_SHIFT_AND_INEXACT, O.SHIFT_AND_INEXACT)
BITVEC1 = (1, sat_amd.SEM_FILTER_BITVEC, sat_amd.SEM_FILTER_BITVEC, 5)
HALVES1 = (1, sat_amd.SEM_EXACT_HALVES, sat_amd.SEM_EXACT_HALVES, 12)


def rand_seq(rng, n):
    return "".join(rng.choice(BASES, size=n).tolist())


def engine(pats, k, sem=sat_amd.SEM_AUTO, kernel=sat_amd.KERNEL_AUTO, zones=None, indels=False, wildcards=False, long_patterns=True):
    pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sem, kernel=kernel, wildcards=wildcards, long_patterns=long_patterns)
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


def nlong(pats):
    return sum(1 for p in pats if 33 <= len(p) <= 64)


def long_route(pm, pats, selected, residue=0):
    """the handle runs the long primers on the pair plan, and the bit-parallel kernel `residue` primers"""
    d = pm.describe()
    assert pm.selected() == (selected, sat_amd.KERNEL_SEED), d
    assert "pm_pair_scan" in d and ("%d patterns %s" % (nlong(pats), LONG_PHRASE)) in d and "pm_pair_verify_wide" in d, d
    if residue:
        assert ("for %d patterns the seed plan does not take" % residue) in d, d
    else:
        assert "does not take" not in d, d
    return d


# ---- 1. exhaustive ---------------------------------------------------------------------------------------------------
_EXH = {}


def exhaustive_case(L):
    if L not in _EXH:
        rng = np.random.default_rng(3300 + L)
        p = rand_seq(rng, L)
        variants = sorted(set().union(*(substitution_variants(p, k) for k in (0, 1, 2))))
        parts = stream_of(variants, rng)
        codes = synth.normalize(synth.stream(parts), TABLE)
        decoys = [rand_seq(rng, 20) for _ in range(1500)] + [rand_seq(rng, int(rng.integers(33, 65))) for _ in range(200)]
        _EXH[L] = dict(p=p, nvar=len(variants), codes=codes, pats=[p] + decoys, bounds=entry_bounds(parts))
    return _EXH[L]


@pytest.mark.parametrize("opts", [BITVEC2, INEXACT2, BITVEC1, HALVES1], ids=["bitvec2", "inexact2", "bitvec1", "halves1"])
@pytest.mark.parametrize("L", [33, 64])
def test_every_text_within_two_substitutions_of_a_long_primer(L, opts):
    c = exhaustive_case(L)
    assert c["nvar"] == {33: 4852, 64: 18337}[L]
    k, sem, selected, eng = opts
    want = oracle_hits(c["codes"], TABLE, c["pats"], k, eng)
    pm = engine(c["pats"], k, sem)
    try:
        pm.init(c["codes"], TABLE)
        d = long_route(pm, c["pats"], selected)
        got = sat_amd.sorted_tuples(pm.find_all())
    finally:
        pm.close()
    print("exhaustive L %d k %d sem %d: %d hits (oracle %d) [%s]" % (L, k, sem, len(got), len(want), d))
    assert got == want, (L, k, sem, len(got), len(want))
    if k == 2:                                                       # conditions on the oracle's own output
        own = [(e, dist) for e, pid, dist in want if pid == 1]
        ends = np.array(sorted({e for e, _ in own}))
        for (a, b) in c["bounds"]:
            i = np.searchsorted(ends, a, side="right")
            assert i < ends.size and ends[i] <= b, (L, sem, a, b)
        assert {dist for _, dist in own} == {0, 1, 2}


# ---- 2. a mixed list on text with repeats and N runs, through every interface ------------------------------------------
_MIXED = {}
MIXED_OPTS = {"bitvec2": BITVEC2, "inexact2": INEXACT2, "halves1": HALVES1}


def mixed_case():
    """planted primers of 21..32, 33..64 and 16..19 characters (substitutions only), both strands, lengths 33, 63 and 64
    among them, a duplicate and a reverse-complement pair among the long ones; `rest`: a primer with an N and a 70-mer,
    which no option set takes onto the pair plan (exact_halves keeps no residue: its list goes without them)"""
    if not _MIXED:
        rng = np.random.default_rng(3364)
        ents = synth.make_entries(rng, 3, 12000, n_runs=3, repeats=True, short=True)
        mid_p = synth.make_patterns(rng, ents, 60, length=32, minlen=21, planted=0.9, indel_frac=0, extras=False)
        long_p = synth.make_patterns(rng, ents, 60, length=64, minlen=33, planted=0.9, indel_frac=0, extras=False)
        for i, L in enumerate((33, 63, 64, 47)):
            a = 700 + 300 * i
            long_p[4 + i] = synth.mutate(rng, ents[i % 3][a:a + L].replace("N", "A"), nsub=i % 3)
        long_p[1], long_p[3] = long_p[0], synth.revcomp(long_p[0])
        short_p = synth.make_patterns(rng, ents, 30, length=19, minlen=16, planted=0.9, indel_frac=0, extras=False)
        pats = mid_p + long_p + short_p
        allp = pats + [synth.revcomp(p) for p in pats]
        rest = [ents[0][500:509] + "N" + ents[0][510:530], ents[1][100:170].replace("N", "A")]
        assert len(rest[1]) == 70
        table = synth.table_for(ents)
        codes = synth.normalize(synth.stream(ents), table)
        _MIXED.update(ents=ents, main=allp, rest=rest, table=table, codes=codes, want={})
    return _MIXED


def mixed_pats(name, rest=True):
    c = mixed_case()
    return c["main"] + (c["rest"] if rest and name != "halves1" else [])


def mixed_want(name, rest=True):
    c = mixed_case()
    key = (name, rest and name != "halves1")
    if key not in c["want"]:
        k, _, _, eng = MIXED_OPTS[name]
        c["want"][key] = oracle_hits(c["codes"], c["table"], mixed_pats(name, rest), k, eng)
    return c["want"][key]


def mixed_engine(name, rest=True, **kw):
    k, sem, _, _ = MIXED_OPTS[name]
    return engine(mixed_pats(name, rest), k, sem, **kw)


def check_mixed_route(pm, name, rest=True):
    pats = mixed_pats(name, rest)
    d = long_route(pm, pats, MIXED_OPTS[name][2], residue=len(pats) - len(mixed_case()["main"]))
    assert "pm_short_sub_scan for 60 patterns of 16..19 characters" in d, d


def test_mixed_list_condition():
    """the oracle reports hits of long primers at each of the distances 0, 1, 2, hits of the other classes and of the
    residue, and under exact_halves hits of long primers"""
    pats = mixed_pats("bitvec2")
    want = mixed_want("bitvec2")
    assert {dist for _, pid, dist in want if 33 <= len(pats[pid - 1]) <= 64} == {0, 1, 2}
    for lo, hi in ((16, 19), (20, 32), (70, 70)):
        assert any(lo <= len(pats[pid - 1]) <= hi for _, pid, _ in want), (lo, hi)
    assert {len(pats[pid - 1]) for _, pid, _ in want} >= {33, 63, 64}
    for name in ("inexact2", "halves1"):
        p2 = mixed_pats(name)
        assert any(len(p2[pid - 1]) > 32 for _, pid, _ in mixed_want(name))


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
    """scan_candidates + finalize_device: pm_cluster_reduce (with the level-3 records of zone violations, see the zones
    test), the exact_halves rule and the automaton's pass-through take the long primers' records: in one range, and for
    the first two in two ranges and position-sharded"""
    c = mixed_case()
    want = mixed_want(name, rest=False)
    n = c["codes"].size
    pm = mixed_engine(name, rest=False)
    try:
        pm.init(c["codes"], c["table"])
        check_mixed_route(pm, name, rest=False)
        pm.scan_candidates(0, n, to_host=False)
        assert sat_amd.sorted_tuples(pm.finalize_device(n)) == want
        if name != "halves1":                                        # (exact_halves' rule on the device takes the whole range in one call)
            pm.reset()                                               # two ranges: what is open at the cut is carried
            pm.scan_candidates(0, n // 2, to_host=False)
            first = sat_amd.sorted_tuples(pm.finalize_device(n // 2, last=False))
            pm.scan_candidates(n // 2, n, to_host=False)
            second = sat_amd.sorted_tuples(pm.finalize_device(n))
            assert sorted(first + second) == want
            cut, guard, parts = n // 3 + 5, 400, []                  # position shards with guard margins
            for own_lo, own_hi in ((0, cut), (cut, n)):
                g_lo, g_hi = max(0, own_lo - guard), min(n, own_hi + guard)
                pm.reset()
                pm.scan_candidates(g_lo, g_hi, to_host=False)
                parts += sat_amd.sorted_tuples(pm.finalize_device(0, sort=True, owned=(own_lo, own_hi, g_lo, None if g_hi == n else g_hi)))
            assert sorted(parts) == want
    finally:
        pm.close()


def min_window(pats, k):
    pm = engine(pats, k)
    pm.init(np.zeros(64, dtype=np.uint8), TABLE, window=1)
    w = pm.residency()["window"]
    pm.close()
    return w


@pytest.mark.parametrize("packed,windowed", [(False, True), (True, False), (True, True)])
def test_mixed_list_windowed_and_packed(packed, windowed):
    c = mixed_case()
    want = mixed_want("bitvec2")
    n = c["codes"].size
    window = min_window(mixed_pats("bitvec2"), 2) if windowed else None
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


# ---- 3. the stream's edges ------------------------------------------------------------------------------------------
def edges_case():
    """long primers at the stream's first and last characters, with the first one or two characters missing in front of
    the stream (the automaton's end = L - d), hanging over the stream's end by 1 and by len2 = 32 characters
    (exact_halves), and across an end-of-sequence character that lies at index 40 of the window"""
    rng = np.random.default_rng(3370)
    other = lambda ch: BASES[(BASES.index(ch) + 1 + int(rng.integers(0, 3))) % 4]
    e0, e1, e2 = rand_seq(rng, 150), rand_seq(rng, 90), rand_seq(rng, 130)
    raw = (e0 + "\n" + e1 + "\n" + e2).encode()                      # the stream starts and ends with a base
    codes = synth.normalize(raw, TABLE)
    n = codes.size
    pats = []
    for L in (33, 40, 64):
        pats += [e0[:L], other(e0[0]) + e0[1:L],                     # the stream's first characters; the first one substituted
                 rand_seq(rng, 1) + e0[:L - 1], rand_seq(rng, 2) + e0[:L - 2],   # the first one / two missing in front of the stream
                 e2[-L:], e2[-L:-1] + other(e2[-1]),                 # ends at the last byte; its last character substituted
                 e2[-(L - 1):] + "A"]                                # hangs over the end by one (code 0 = A)
    pats += [e2[-32:] + "A" * 32, e2[-63:] + "A", e2[-33:] + "A" * 31]           # L = 64: overhangs of len2 = 32, of 1, of 31
    pats += [e0[-40:] + "A" + e1[:23], e1[:40], e1[-40:]]            # EOS at index 40; right behind / in front of an EOS
    pats += [rand_seq(rng, 22) for _ in range(5)] + [e1[10:32], e0[5:23]]
    return dict(codes=codes, table=TABLE, pats=pats, eos64=pats.index(e0[-40:] + "A" + e1[:23]) + 1)


def test_stream_edges():
    c = edges_case()
    codes, pats, n = c["codes"], c["pats"], c["codes"].size
    seen_start = seen_over = False
    for k, sem, selected, eng in (BITVEC2, INEXACT2, BITVEC1, HALVES1):
        want = oracle_hits(codes, TABLE, pats, k, eng)
        assert c["eos64"] not in {pid for _, pid, _ in want}             # nothing matches across an end-of-sequence character
        seen_start = seen_start or any(e < len(pats[pid - 1]) for e, pid, _ in want)
        seen_over = seen_over or any(e > n for e, pid, _ in want)
        for chunk in (1 << 26, 37, 3):
            pm = engine(pats, k, sem)
            try:
                pm.init(codes, TABLE)
                long_route(pm, pats, selected)
                got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
                pm.reset()                                           # ranges of a few positions at both ends, through the candidate stage
                for b, e in ((0, 3), (3, 70), (n - 66, n - 2), (n - 2, n)):
                    r = pm.scan_candidates(b, e)
                    assert all(b < x <= e or x > n for x in r["end"].tolist()), (b, e, r["end"].tolist())
            finally:
                pm.close()
            assert got == want, (k, sem, chunk, got, want)
    assert seen_start and seen_over                                  # the oracle has hits with end < L and with end > n


@pytest.mark.parametrize("nbytes", [20, 33, 63, 64, 65])
def test_tiny_streams(nbytes):
    """streams of 20, 33, 63, 64 and 65 bytes against a list with a 64-mer, a 33-mer and a 20-mer cut from them"""
    rng = np.random.default_rng(3380 + nbytes)
    p = rand_seq(rng, 64)
    raw = {20: p[:20], 33: p[:33], 63: p[1:], 64: p, 65: "G" + p}[nbytes]
    assert len(raw) == nbytes
    pats = [p, p[:33], p[:20], p[31:], rand_seq(rng, 40), p[:30] + rand_seq(rng, 34), rand_seq(rng, 21)]
    codes = synth.normalize(raw.encode(), TABLE)
    for k, sem, selected, eng in (BITVEC2, INEXACT2, HALVES1):
        want = oracle_hits(codes, TABLE, pats, k, eng)
        pm = engine(pats, k, sem)
        try:
            pm.init(codes, TABLE)
            long_route(pm, pats, selected)
            got = sat_amd.sorted_tuples(pm.find_all())
        finally:
            pm.close()
        assert got == want, (nbytes, k, sem, got, want)
    if nbytes == 63:
        assert (63, 1, 1) in oracle_hits(codes, TABLE, pats, 2, O.SHIFT_AND_INEXACT)   # the 64-mer with its first character missing


# ---- 4. exact zones and IUPAC letters on long primers -----------------------------------------------------------------
def zones_case():
    """-3 8 and -5 8 on primers of 40..64 characters: the zone bits lie below index 32 (exact start bases) and above it
    (exact end bases).  Every primer is planted exact, with a substitution inside its zone and with one outside it."""
    rng = np.random.default_rng(3390)
    other = lambda ch: BASES[(BASES.index(ch) + 1 + int(rng.integers(0, 3))) % 4]
    prim, zones, ents = [], [], []
    for i in range(24):
        L = (40, 47, 63, 64)[i % 4]
        p = rand_seq(rng, L)
        z = [(8, 0), (0, 8), (8, 8)][i % 3]
        inside = int(rng.integers(0, 8)) if z[0] and (i % 2 == 0 or not z[1]) else L - 1 - int(rng.integers(0, 8))
        outside = int(rng.integers(9, L - 9))
        sub = lambda s, j: s[:j] + other(s[j]) + s[j + 1:]
        ents += [rand_seq(rng, 30) + p + rand_seq(rng, 30), rand_seq(rng, 30) + sub(p, inside) + rand_seq(rng, 30),
                 rand_seq(rng, 30) + sub(p, outside) + rand_seq(rng, 30), rand_seq(rng, 30) + sub(sub(p, outside), inside) + rand_seq(rng, 30)]
        prim.append(p)
        zones.append(z)
    pats = prim + [rand_seq(rng, 24) for _ in range(40)]
    zones += [(0, 0)] * 40
    return dict(codes=synth.normalize(synth.stream(ents), TABLE), table=TABLE, pats=pats, zones=zones)


def test_zones_on_long_primers():
    c = zones_case()
    codes, pats, zones = c["codes"], c["pats"], c["zones"]
    for name, (k, sem, selected, eng) in (("bitvec2", BITVEC2), ("bitvec1", BITVEC1), ("halves1", HALVES1)):
        want = oracle_hits(codes, TABLE, pats, k, eng, zones)
        free = oracle_hits(codes, TABLE, pats, k, eng)
        assert len(want) < len(free), name                           # the zones remove hits, and leave some
        assert len({pid for _, pid, _ in want if pid <= 24}) == 24   # every zoned primer keeps a hit
        for chunk in (1 << 26, 193):
            pm = engine(pats, k, sem, zones=zones)
            try:
                pm.init(codes, TABLE)
                long_route(pm, pats, selected)
                got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
                if chunk == 193 and name == "bitvec2":               # pm_cluster_reduce takes the level-3 records of zone violations
                    pm.reset()
                    r = pm.scan_candidates(0, codes.size)
                    assert 3 in set(r["k"].tolist())
                    pm.scan_candidates(0, codes.size, to_host=False)
                    assert sat_amd.sorted_tuples(pm.finalize_device(codes.size)) == want
            finally:
                pm.close()
            assert got == want, (name, chunk, len(got), len(want))


def iupac_case():
    """-w on a plain stream: 40-mers with one and two IUPAC letters (expanded into their variants, as in the main class)"""
    rng = np.random.default_rng(3391)
    ents = synth.make_entries(rng, 2, 6000)
    codes = synth.normalize(synth.stream(ents), TABLE)
    pats = synth.make_patterns(rng, ents, 40, length=40, planted=0.9, indel_frac=0, extras=False) + \
        synth.make_patterns(rng, ents, 40, length=24, minlen=20, planted=0.9, indel_frac=0, extras=False)
    amb = 0
    for i in range(0, 40, 3):
        p = list(pats[i])
        for j in (5, 36)[:1 + (i // 3) % 2]:                         # index 5, and index 36 beyond the first dword
            p[j] = {"A": "R", "C": "Y", "G": "K", "T": "W"}[p[j]]
        pats[i] = "".join(p)
        amb += 1
    assert amb >= 10
    return dict(codes=codes, table=TABLE, pats=pats + [synth.revcomp_iupac(q) for q in pats], wildcards=True)


def test_iupac_letters_in_long_primers():
    c = iupac_case()
    codes, allp = c["codes"], c["pats"]
    want = O.sorted_tuples(O.find_all(O.Text(codes, TABLE), allp, engine=5, k=2, indels=False, wildcards=True, text_n=False))
    assert any(set(allp[pid - 1]) - set("ACGT") and len(allp[pid - 1]) == 40 for _, pid, _ in want)   # a hit of a 40-mer with an IUPAC letter
    for chunk in (1 << 26, 997):
        pm = engine(allp, 2, wildcards=True)
        try:
            pm.init(codes, TABLE)
            d = pm.describe()
            assert pm.selected()[1] == sat_amd.KERNEL_SEED and ("80 patterns " + LONG_PHRASE) in d and "does not take" not in d, d
            got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        finally:
            pm.close()
        assert got == want, (chunk, len(got), len(want))


# ---- 5. 40-mers and 18-mers only ---------------------------------------------------------------------------------------
def forty_eighteen_case():
    """no primer of 20..32 characters: the 40-mers are the main class, the 18-mers run on pm_short_sub_scan"""
    rng = np.random.default_rng(3392)
    ents = synth.make_entries(rng, 2, 8000, n_runs=2)
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    pats = synth.make_patterns(rng, ents, 50, length=40, planted=0.9, indel_frac=0, extras=False) + \
        synth.make_patterns(rng, ents, 50, length=18, planted=0.9, indel_frac=0, extras=False)
    return dict(codes=codes, table=table, pats=pats)


def test_forty_mers_and_eighteen_mers_only():
    c = forty_eighteen_case()
    codes, table, pats = c["codes"], c["table"], c["pats"]
    for k, sem, selected, eng in (BITVEC2, INEXACT2, HALVES1):
        want = oracle_hits(codes, table, pats, k, eng)
        assert {len(pats[pid - 1]) for _, pid, _ in want} == {18, 40}
        pm = engine(pats, k, sem)
        try:
            pm.init(codes, table)
            d = long_route(pm, pats, selected)
            assert "50 patterns " + LONG_PHRASE in d and "pm_short_sub_scan for 50 patterns of 16..19 characters" in d, d
            got = sat_amd.sorted_tuples(pm.find_all(chunk=4000))
        finally:
            pm.close()
        assert got == want, (k, sem, len(got), len(want))


# ---- 6. routing, and the final hits against the former route's ---------------------------------------------------------
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
out = []
for case in c["cases"]:
    pm = sat_amd.PatternMatch(k=case["k"], indels=False, semantics=case["sem"], wildcards=case.get("wildcards", False), long_patterns=case["long"])
    for i, p in enumerate(case["pats"]):
        z = case["zones"][i] if case.get("zones") else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    codes = np.load(case["codes"]) if "codes" in case else np.array(c["codes"], dtype=np.uint8)
    pm.init(codes, case.get("table", c.get("table", "")).encode())
    hits = sat_amd.sorted_tuples(pm.find_all())
    out.append({"selected": list(pm.selected()), "describe": pm.describe(), "hits": [list(h) for h in hits]})
    pm.close()
print("RESULT " + json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "tests"))


def run_child(case, env):
    r = subprocess.run([sys.executable, "-c", CHILD, str(case)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def outcome(codes, table, pats, k=2, **kw):
    pm = engine(pats, k, **kw)
    try:
        pm.init(codes, table)
        hits = sat_amd.sorted_tuples(pm.find_all())                  # (the description holds the launch geometry)
        return pm.selected(), pm.describe(), hits
    except sat_amd.PmError as e:
        return e.code, str(e), None
    finally:
        pm.close()


def test_without_the_permission_the_route_is_the_former_one(tmp_path):
    """long_patterns=False, and long_patterns=True with PM_LONG_SUB=off in a fresh process (the environment is read by
    pm_create): selected() and describe() of the handle without the flag, and -- the differential -- the same final hits
    as the long route gives in this process"""
    c = mixed_case()
    cases, here = [], []
    for name in MIXED_OPTS:
        k, sem, selected, _ = MIXED_OPTS[name]
        pats = mixed_pats(name)
        cases.append(dict(k=k, sem=sem, pats=pats, long=True))
        off = outcome(c["codes"], c["table"], pats, k, sem=sem, long_patterns=False)
        on = outcome(c["codes"], c["table"], pats, k, sem=sem, long_patterns=True)
        here.append((off, on))
        assert LONG_PHRASE not in off[1] and LONG_PHRASE in on[1], (off[1], on[1])
        assert off[2] == on[2] == mixed_want(name), (name, len(off[2]), len(on[2]))
        if name != "halves1":
            assert ("for %d patterns the seed plan does not take" % (nlong(pats) + 2)) in off[1], off[1]
        else:
            assert off[0] == (selected, sat_amd.KERNEL_BITPAR), off[:2]   # one long primer takes an exact_halves list to the bit-parallel family
    case = tmp_path / "case.json"
    case.write_text(json.dumps({"cases": cases, "codes": c["codes"].tolist(), "table": c["table"].decode()}))
    env = {x: v for x, v in os.environ.items() if x != "PM_LONG_SUB"}
    knob = run_child(case, dict(env, PM_LONG_SUB="off"))
    for (off, on), child in zip(here, knob):
        assert (tuple(child["selected"]), child["describe"]) == (off[0], off[1]), (child["describe"], off[1])
        assert [tuple(h) for h in child["hits"]] == off[2]


OTHER_LISTS = {
    "every text within two substitutions of a 33-mer": lambda: dict(exhaustive_case(33), table=TABLE),
    "every text within two substitutions of a 64-mer": lambda: dict(exhaustive_case(64), table=TABLE),
    "the stream's edges": edges_case,
    "exact zones": zones_case,
    "IUPAC letters": iupac_case,
    "40-mers and 18-mers": forty_eighteen_case,
}


@pytest.mark.parametrize("what", list(OTHER_LISTS))
def test_without_the_permission_every_list_keeps_its_former_route(what, tmp_path):
    """each list of the tests above, under -K 2 filter_bitvec and (A,C,G,T lists) -K 1 exact_halves: without the permission
    the long primers are residue or take the list to the bit-parallel family, as before; with the permission and
    PM_LONG_SUB=off in a fresh process selected() and describe() are the same, byte for byte, and so are the final hits"""
    c = OTHER_LISTS[what]()
    wild = bool(c.get("wildcards"))
    opts = [(2, sat_amd.SEM_AUTO)] if wild else [(2, sat_amd.SEM_FILTER_BITVEC), (1, sat_amd.SEM_EXACT_HALVES)]
    np.save(tmp_path / "codes.npy", c["codes"])
    cases, here = [], []
    for k, sem in opts:
        kw = dict(sem=sem, zones=c.get("zones"), wildcards=wild)
        off = outcome(c["codes"], c["table"], c["pats"], k, long_patterns=False, **kw)
        on = outcome(c["codes"], c["table"], c["pats"], k, long_patterns=True, **kw)
        assert LONG_PHRASE not in off[1] and LONG_PHRASE in on[1] and off[2] is not None, (what, k, off[:2], on[:2])
        if sem == sat_amd.SEM_EXACT_HALVES or c.get("zones"):        # (zones on a pattern outside 20..32: the text-based verify)
            assert off[0][1] == sat_amd.KERNEL_BITPAR, (what, off[:2])
        else:
            assert ("for %d patterns the seed plan does not take" % nlong(c["pats"])) in off[1], (what, off[1])
        here.append(off)
        cases.append(dict(k=k, sem=sem, pats=c["pats"], zones=c.get("zones"), wildcards=wild, long=True,
                          codes=str(tmp_path / "codes.npy"), table=bytes(c["table"]).decode()))
    case = tmp_path / "case.json"
    case.write_text(json.dumps({"cases": cases}))
    env = {x: v for x, v in os.environ.items() if x != "PM_LONG_SUB"}
    for off, child in zip(here, run_child(case, dict(env, PM_LONG_SUB="off"))):
        assert (tuple(child["selected"]), child["describe"]) == (off[0], off[1]), (what, child["describe"], off[1])
        assert [tuple(h) for h in child["hits"]] == off[2], what


def test_routing():
    """lists and option sets the route does not apply to: selected() and describe() are those of the handle without the
    permission, byte for byte"""
    rng = np.random.default_rng(3393)
    ents = synth.make_entries(rng, 2, 6000)
    codes = synth.normalize(synth.stream(ents), TABLE)
    mids = synth.make_patterns(rng, ents, 30, length=24, minlen=20, planted=0.8, extras=False)
    longs = synth.make_patterns(rng, ents, 10, length=64, minlen=33, planted=0.8, indel_frac=0, extras=False)
    mixed = mids + longs
    z6 = [(6, 0)] * len(mixed)
    cases = {
        "k = 0": dict(pats=mixed, k=0),
        "-k": dict(pats=mixed, indels=True),
        "-k 1 exact_halves": dict(pats=mixed, k=1, indels=True, sem=sat_amd.SEM_EXACT_HALVES),
        "exact_bases": dict(pats=mixed, sem=sat_amd.SEM_EXACT_BASES, zones=z6),
        "seed kernels on request": dict(pats=mixed, kernel=sat_amd.KERNEL_SEED),
        "bit-parallel kernels on request": dict(pats=mixed, kernel=sat_amd.KERNEL_BITPAR),
        "no long primer": dict(pats=mids),
        "the only long primer has 65 characters": dict(pats=mids + [ents[0][200:265]]),
        "the same under exact_halves": dict(pats=mids + [ents[0][200:265]], k=1, sem=sat_amd.SEM_EXACT_HALVES),
        "a primer of 12 beside the long ones": dict(pats=mixed + [ents[0][400:412]]),
        "keyword tree": dict(pats=mixed, k=0, sem=sat_amd.SEM_KEYWORD_TREE),
    }
    for what, kw in cases.items():
        off = outcome(codes, TABLE, long_patterns=False, **kw)
        on = outcome(codes, TABLE, long_patterns=True, **kw)
        assert off[:2] == on[:2], (what, off[:2], on[:2])
        assert LONG_PHRASE not in on[1], (what, on[1])
        assert off[2] == on[2], what
    on = outcome(codes, TABLE, mixed + [ents[0][200:265]], long_patterns=True)       # 65 characters: residue beside the long route
    assert ("10 patterns " + LONG_PHRASE) in on[1] and "for 1 patterns the seed plan does not take" in on[1], on[1]


# ---- 7. a wide tile beside a narrow one ------------------------------------------------------------------------------
def test_two_tiles(monkeypatch):
    """PM_SEED_TILE cuts the main class in two: the first tile holds primers of 21..32 characters only and is built and
    verified as ever, the second one holds the long primers"""
    c = mixed_case()
    pats = mixed_pats("bitvec2", rest=False)
    order = sorted(range(len(pats)), key=lambda i: (len(pats[i]) > 32, i))   # (ids stay: the list is added in this order)
    main = [i for i in order if len(pats[i]) >= 20]
    monkeypatch.setenv("PM_SEED_TILE", str((len(main) + 1) // 2))
    assert all(len(pats[i]) <= 32 for i in main[:(len(main) + 1) // 2])
    pm = sat_amd.PatternMatch(k=2, indels=False, semantics=sat_amd.SEM_FILTER_BITVEC, long_patterns=True)
    for i in order:
        pm.add_pattern(pats[i], i + 1)
    try:
        pm.init(c["codes"], c["table"])
        d = pm.describe()
        assert "tiles=2 " in d and "wide tiles=1)" in d, d
        got = sat_amd.sorted_tuples(pm.find_all())
    finally:
        pm.close()
    assert got == mixed_want("bitvec2", rest=False)


# ---- 8. counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rest", [False, True])
@pytest.mark.parametrize("M", [0, 2])
def test_mixed_list_counts(M, rest):
    """count_all: the count rule on the oracle's hits; without the 70-mer and the primer with an N no record goes to the
    host for its re-alignment"""
    c = mixed_case()
    pats = mixed_pats("bitvec2", rest)
    want = mixed_want("bitvec2", rest)
    key = ("eds", rest)
    if key not in c:
        text = O.Text(c["codes"], c["table"])
        c[key] = [O.cli_align(text, pats[pid - 1], end, 2, False)[3] for end, pid, _ in want]
    wc, wcap, winfo = count_rule.tally(want, lambda i: c[key][i], len(pats), 2, M)
    pm = mixed_engine("bitvec2", rest)
    try:
        pm.init(c["codes"], c["table"])
        check_mixed_route(pm, "bitvec2", rest)
        counts, capped, info = pm.count_all(max_count=M)
    finally:
        pm.close()
    assert counts.tolist() == wc
    assert capped.tolist() == wcap
    for f in ("tallied", "skipped", "bogus"):
        assert info[f] == winfo[f], (f, info[f], winfo[f])
    if not rest:
        assert info["aligned_host"] == 0 and info["aligned_device"] > 0, info
    else:
        assert info["aligned_host"] > 0, info


def test_realignment_of_long_primers_on_the_device():
    """align_hits_device_numpy(text=True) against align_hits / align_hits_text, field for field: the final hits of the
    zoned list (test_zones_on_long_primers' construction in small), and records made up so that the re-alignment fails:
    a substitution inside an exact zone, three substitutions, an end-of-sequence character inside the window, an end in
    front of the pattern's length ("Bogus" hits of the caller's tally)"""
    rng = np.random.default_rng(3394)
    other = lambda ch: BASES[(BASES.index(ch) + 1 + int(rng.integers(0, 3))) % 4]
    sub = lambda s, j: s[:j] + other(s[j]) + s[j + 1:]
    prim, zones, ents, made = [], [], [], []
    pos = 1                                                          # (synth.stream: an EOS in front of the first entry)
    for i in range(12):
        L = (33, 40, 63, 64)[i % 4]
        p = rand_seq(rng, L)
        z = [(8, 0), (0, 8), (0, 0)][i % 3]
        forms = [p, sub(p, 20), sub(sub(p, 12), 40 if L > 48 else 22), sub(p, 3 if z[0] else L - 3), sub(sub(sub(p, 10), 15), 30)]
        for f in forms:
            ents.append(rand_seq(rng, 5) + f + rand_seq(rng, 5))
            made.append((pos + 5 + L, i + 1, 0))
            pos += len(ents[-1]) + 1
        made.append((pos + 3, i + 1, 0))                             # a window that reaches across the end-of-sequence character (the last one: beyond the stream)
        prim.append(p)
        zones.append(z)
    made += [(10, 1, 0), (32, 4, 0)]                                 # ends in front of the pattern's length
    codes = synth.normalize(synth.stream(ents), TABLE)
    pm = engine(prim, 2, sat_amd.SEM_FILTER_BITVEC, zones=zones)
    try:
        pm.init(codes, TABLE)
        long_route(pm, prim, sat_amd.SEM_FILTER_BITVEC)
        final = pm.find_all()
        assert final.size >= 30
        pm.reset()
        on_device = 0
        for what, hits in (("final hits", final), ("made-up records", hit_array(made))):
            al, ops, txt = pm.align_hits_device_numpy(hits, text=True)
            _, _, info = pm.counts()
            on_device += hits.size                                   # (the handle's counters run on from call to call)
            assert info["aligned_host"] == 0 and info["aligned_device"] == on_device, (what, info)
            with_alignment = check_against_host(pm, hits, al, ops, txt, what)
            text = O.Text(codes, TABLE)
            for i in range(hits.size):                               # the independent check: the oracle's re-alignment
                z = zones[int(hits["pid"][i]) - 1]
                _, st, en, ed, _ = O.cli_align(text, prim[int(hits["pid"][i]) - 1], int(hits["end"][i]), 2, False, esb=z[0], eeb=z[1])
                assert (int(al["start"][i]), int(al["end"][i]), int(al["editdist"][i])) == (st, en, ed), (what, hits[i], al[i], (st, en, ed))
            if what == "made-up records":
                eds = al["editdist"].tolist()
                assert {0, 1, 2} <= set(eds) and sum(1 for e in eds if e > 2) >= 12 + 12 + 2, eds   # three substitutions, across the EOS, too early
                assert 0 < with_alignment < hits.size
    finally:
        pm.close()
