"""GPU: primers of 33..64 characters under -k 1 / -k 2 on the edit plan (bit 2 of pm_config.long_patterns,
long_edits=True; csrc/pm_edits.h edits_verify<uint64_t> and device_editdist<64>, csrc/pm_seed.hip pm_edits_verify_wide,
csrc/pm_cluster.hip pm_cluster_dp<64>).

The first stages of the edit plan key on a primer's last 20 bases, so a primer of up to 64 characters needs no pass of
its own: it joins the plan's tiles, and a tile that holds one gets 64-byte automaton records and 64-bit rows.  The route
is a permission of the caller, off by default.  Here: every text within two edits of a 33-mer, the one- and (at the
places where the width matters) two-edit texts of a 64-mer, a mixed list through every interface, the stream's edges,
zones, IUPAC letters, the routing rules, the final hits against the former route's, a wide tile beside a narrow one and
the counts.  Expected values come from the oracle.

Option sets: `-k 2` auto and `-k 1` auto are filter_bitvec here.  Under -k 1 the automatic choice is exact_halves for a
list whose primers all have 12 characters or more (select.cc:121-126) -- an option set the route does not apply to --
so the lists of the -k 1 auto cases hold one 11-mer (residue), with which the choice is filter_bitvec."""
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

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = b"ACGT\n"
BASES = list("ACGT")
LONG_PHRASE = "of 33..64 characters"
WIDE_PHRASE = "(pm_edits_verify_wide, wide tiles="
ELEVEN = "ACGGTCATTGA"
# option sets: (k, semantics asked for, semantics selected, the oracle's engine, primers added to the list)
AUTO2 = (2, sat_amd.SEM_AUTO, sat_amd.SEM_FILTER_BITVEC, 5, [])
INEXACT2 = (2, sat_amd.SEM_SHIFT_AND_INEXACT, sat_amd.SEM_SHIFT_AND_INEXACT, O.SHIFT_AND_INEXACT, [])
BITVEC1 = (1, sat_amd.SEM_FILTER_BITVEC, sat_amd.SEM_FILTER_BITVEC, 5, [])
AUTO1 = (1, sat_amd.SEM_AUTO, sat_amd.SEM_FILTER_BITVEC, 5, [ELEVEN])
OPTS = {"k2_auto": AUTO2, "k2_inexact": INEXACT2, "k1_bitvec": BITVEC1, "k1_auto": AUTO1}


# ---- helpers (as tests/test_gpu_exhaustive.py builds its streams) ------------------------------------------------------
def one_edit(w, lo=0, hi=None):
    """texts one edit away from w, the edit at an index in [lo, hi) (insertions: in front of lo .. hi)"""
    hi = len(w) if hi is None else min(hi, len(w))
    out = set()
    for i in range(lo, hi):
        out.add(w[:i] + w[i + 1:])
        for c in "ACGT":
            if c != w[i]:
                out.add(w[:i] + c + w[i + 1:])
    for i in range(lo, hi + 1):
        for c in "ACGT":
            out.add(w[:i] + c + w[i:])
    return out


def edit_variants(p, k, lo=0, hi=None):
    hi = len(p) if hi is None else hi
    level, seen = {p}, {p}
    for _ in range(k):
        nxt = set()
        for w in level:
            nxt |= one_edit(w, lo, hi + len(w) - len(p))
        level = nxt - seen
        seen |= nxt
    return seen


def stream_of(variants, rng):
    """variants between end-of-sequence characters, two to four random bases in front of each and up to three behind (the
    automaton cannot delete a pattern's first characters right behind an end-of-sequence character)"""
    parts = []
    for v in variants:
        pad_l = "".join(rng.choice(BASES, size=int(rng.integers(2, 5))).tolist())
        pad_r = "".join(rng.choice(BASES, size=int(rng.integers(0, 4))).tolist())
        parts.append(pad_l + v + pad_r)
    return parts


def entry_bounds(parts):
    b, at = [], 1
    for s in parts:
        b.append((at, at + len(s)))
        at += len(s) + 1
    return b


def rand_seq(rng, n):
    return "".join(rng.choice(BASES, size=n).tolist())


def engine(pats, k, sem=sat_amd.SEM_AUTO, bits=4, zones=None, ids=None, indels=True, **kw):
    """bits: pm_config.long_patterns (1: -K, 2: k = 0, 4: -k)"""
    pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sem, long_patterns=bool(bits & 1), long_exact=bool(bits & 2),
                              long_edits=bool(bits & 4), **kw)
    for i, p in enumerate(pats):
        z = zones[i] if zones else (0, 0)
        pm.add_pattern(p, ids[i] if ids else i + 1, z[0], z[1])
    return pm


def oracle_hits(codes, table, pats, k, eng, zones=None, wildcards=False):
    esb = [z[0] for z in zones] if zones else None
    eeb = [z[1] for z in zones] if zones else None
    return O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=eng, k=k, indels=True, esb=esb, eeb=eeb, wildcards=wildcards))


def nlong(pats):
    return sum(1 for p in pats if 33 <= len(p) <= 64 and set(p) <= set(BASES))


def nresidue(pats):
    return sum(1 for p in pats if len(p) > 64 or len(p) < 16 or not set(p) <= set(BASES))


def long_route(pm, pats, selected, n_long=None, residue=None, wide_tiles=None):
    d = pm.describe()
    n_long = nlong(pats) if n_long is None else n_long
    residue = nresidue(pats) if residue is None else residue
    assert pm.selected() == (selected, sat_amd.KERNEL_SEED), d
    assert ("with %d patterns %s %s" % (n_long, LONG_PHRASE, WIDE_PHRASE)) in d, d
    assert "pm_edits_verify" in d.split(" with ")[0], d
    if residue:
        assert ("for %d patterns the seed plan does not take" % residue) in d, d
    else:
        assert "does not take" not in d, d
    if wide_tiles is not None:
        assert ("wide tiles=%d)" % wide_tiles) in d, d
    return d


def run(pm, codes, table, chunk=1 << 26):
    pm.init(codes, table)
    return sat_amd.sorted_tuples(pm.find_all(chunk=chunk))


# ---- 1. every text within two edits of a 33-mer ---------------------------------------------------------------------------
_EX = {}


def exhaustive33():
    if 33 not in _EX:
        rng = np.random.default_rng(5533)
        p = rand_seq(rng, 33)
        variants = sorted(edit_variants(p, 2))
        parts = stream_of(variants, rng)
        codes = synth.normalize(synth.stream(parts), TABLE)
        decoys = [rand_seq(rng, int(rng.integers(20, 33))) for _ in range(300)] + [rand_seq(rng, int(rng.integers(33, 65))) for _ in range(100)]
        _EX[33] = dict(p=p, nvar=len(variants), parts=parts, codes=codes, pats=[p] + decoys, want={})
    return _EX[33]


def exhaustive64():
    """every one-edit text of a 64-mer, and every two-edit text whose edits both lie in the first 3 characters, the 4
    around index 32 or the last 22: last = 1 << 63, the word boundary of 32-bit rows, the seeded fields"""
    if 64 not in _EX:
        rng = np.random.default_rng(5564)
        p = rand_seq(rng, 64)
        vs = edit_variants(p, 1) | edit_variants(p, 2, 0, 3) | edit_variants(p, 2, 30, 34) | edit_variants(p, 2, 42, 64)
        variants = sorted(vs)
        parts = stream_of(variants, rng)
        codes = synth.normalize(synth.stream(parts), TABLE)
        decoys = [rand_seq(rng, int(rng.integers(20, 33))) for _ in range(150)] + [rand_seq(rng, int(rng.integers(33, 65))) for _ in range(50)]
        _EX[64] = dict(p=p, nvar=len(variants), parts=parts, codes=codes, pats=[p] + decoys, want={})
    return _EX[64]


def check_exhaustive(c, name):
    k, sem, selected, eng, extra = OPTS[name]
    pats = c["pats"] + extra
    if name not in c["want"]:
        c["want"][name] = oracle_hits(c["codes"], TABLE, pats, k, eng)
    want = c["want"][name]
    pm = engine(pats, k, sem)
    try:
        got = run(pm, c["codes"], TABLE)
        d = long_route(pm, pats, selected, wide_tiles=1)
    finally:
        pm.close()
    print("%s: %d variants, %d hits (oracle %d) [%s]" % (name, c["nvar"], len(got), len(want), d))
    assert got == want, (name, len(got), len(want))
    assert sum(1 for h in want if h[1] == 1) > 1000
    if name == "k2_inexact":                                         # every variant is within two edits: one candidate each at least
        ends = np.array(sorted({e for e, pid, _ in got if pid == 1}))
        for (a, b) in entry_bounds(c["parts"]):
            i = np.searchsorted(ends, a, side="right")
            assert i < ends.size and ends[i] <= b, (a, b)


@pytest.mark.parametrize("name", list(OPTS))
def test_every_text_within_two_edits_of_a_33_mer(name):
    c = exhaustive33()
    assert c["nvar"] > 20000                                         # (about 24,000: some of the two-edit texts coincide)
    check_exhaustive(c, name)


@pytest.mark.parametrize("name", ["k2_auto", "k2_inexact", "k1_bitvec"])
def test_edits_of_a_64_mer_at_the_places_where_the_width_matters(name):
    c = exhaustive64()
    assert c["nvar"] > 3 * 64 + 64 + 4 * 65 - 80                     # (every one-edit text; some coincide)
    check_exhaustive(c, name)


# ---- 2. a mixed list on text with repeats and N runs, through every interface ------------------------------------------------
_MIXED = {}
MIXED_OPTS = {"k2_bitvec": (2, sat_amd.SEM_FILTER_BITVEC, sat_amd.SEM_FILTER_BITVEC, 5, []), "k2_inexact": INEXACT2, "k1_bitvec": BITVEC1}


def mixed_case():
    """primers of 21..32, 33..64 (33, 63 and 64 among them) and 16..19 characters cut from the stream with up to two edits,
    both strands; `rest`: a primer with an N and a 70-mer, which stay residue"""
    if not _MIXED:
        rng = np.random.default_rng(5570)
        ents = synth.make_entries(rng, 3, 12000, n_runs=3, repeats=True, short=True)

        def cut(n, lo, hi, fixed=()):
            out = []
            while len(out) < n:
                e = ents[int(rng.integers(0, 3))]
                L = fixed[len(out)] if len(out) < len(fixed) else int(rng.integers(lo, hi + 1))
                a = int(rng.integers(0, len(e) - L - 2))
                w = e[a:a + L + 2]
                if "N" in w:
                    continue
                ne = int(rng.integers(0, 3))
                w = synth.mutate(rng, w, nsub=int(ne > 0), nins=int(ne > 1 and rng.random() < 0.5), ndel=int(ne > 1 and rng.random() < 0.5))
                w = "".join(w)[:L]
                if len(w) == L:
                    out.append(w)
            return out
        long_p = cut(50, 33, 64, fixed=(33, 63, 64, 47, 34, 64))
        main = cut(50, 21, 32) + long_p + cut(24, 16, 19)
        allp = main + [synth.revcomp(p) for p in main]
        rest = [ents[0][500:509] + "N" + ents[0][510:530], ents[1][100:170].replace("N", "A")]
        assert len(rest[1]) == 70
        table = synth.table_for(ents)
        codes = synth.normalize(synth.stream(ents), table)
        _MIXED.update(ents=ents, main=allp, rest=rest, table=table, codes=codes, want={})
    return _MIXED


def mixed_pats(rest=True):
    c = mixed_case()
    return c["main"] + (c["rest"] if rest else [])


def mixed_want(name, rest=True):
    c = mixed_case()
    if (name, rest) not in c["want"]:
        k, _, _, eng, _ = MIXED_OPTS[name]
        c["want"][(name, rest)] = oracle_hits(c["codes"], c["table"], mixed_pats(rest), k, eng)
    return c["want"][(name, rest)]


def mixed_engine(name, rest=True, **kw):
    k, sem, _, _, _ = MIXED_OPTS[name]
    return engine(mixed_pats(rest), k, sem, **kw)


def check_mixed_route(pm, name, rest=True):
    d = long_route(pm, mixed_pats(rest), MIXED_OPTS[name][2], n_long=100, residue=2 if rest else 0)
    assert "pm_short_edit_scan for 48 patterns of 16..19 characters" in d, d
    return d


def test_mixed_list_condition():
    pats = mixed_pats()
    for name in MIXED_OPTS:
        want = mixed_want(name)
        for lo, hi in ((16, 19), (21, 32), (33, 64), (70, 70)):
            assert any(lo <= len(pats[pid - 1]) <= hi for _, pid, _ in want), (name, lo, hi)
        assert {len(pats[pid - 1]) for _, pid, _ in want} >= {33, 63, 64}, name
        assert len({pid for _, pid, _ in want if 33 <= len(pats[pid - 1]) <= 64}) >= 40
    assert any(d == 2 for _, pid, d in mixed_want("k2_bitvec") if len(pats[pid - 1]) > 32)


@pytest.mark.parametrize("name", list(MIXED_OPTS))
@pytest.mark.parametrize("chunk", [1 << 26, 5000, 193])
def test_mixed_list_find_all(name, chunk):
    c = mixed_case()
    want = mixed_want(name)
    pm = mixed_engine(name)
    try:
        got = run(pm, c["codes"], c["table"], chunk)
        check_mixed_route(pm, name)
    finally:
        pm.close()
    assert got == want, (name, chunk, len(got), len(want))


@pytest.mark.parametrize("name", ["k2_bitvec", "k1_bitvec"])
def test_mixed_list_device_stages(name):
    """scan_candidates + finalize_device (pm_cluster_dp<64>): in one range, in two ranges and the owned finalize on two
    position shards"""
    c = mixed_case()
    want = mixed_want(name, rest=False)
    n = c["codes"].size
    pm = mixed_engine(name, rest=False)
    try:
        pm.init(c["codes"], c["table"])
        pm.scan_candidates(0, n, to_host=False)
        check_mixed_route(pm, name, rest=False)
        assert sat_amd.sorted_tuples(pm.finalize_device(n)) == want
        pm.reset()
        pm.scan_candidates(0, n // 2, to_host=False)
        first = sat_amd.sorted_tuples(pm.finalize_device(n // 2, last=False))
        pm.scan_candidates(n // 2, n, to_host=False)
        second = sat_amd.sorted_tuples(pm.finalize_device(n))
        assert sorted(first + second) == want
        cut, guard, parts = n // 3 + 5, 400, []
        for own_lo, own_hi in ((0, cut), (cut, n)):
            g_lo, g_hi = max(0, own_lo - guard), min(n, own_hi + guard)
            pm.reset()
            pm.scan_candidates(g_lo, g_hi, to_host=False)
            parts += sat_amd.sorted_tuples(pm.finalize_device(0, sort=True, owned=(own_lo, own_hi, g_lo, None if g_hi == n else g_hi)))
        assert sorted(parts) == want
    finally:
        pm.close()


def min_window(pats, k, sem):
    pm = engine(pats, k, sem)
    pm.init(np.zeros(64, dtype=np.uint8), TABLE, window=1)
    w = pm.residency()["window"]
    pm.close()
    return w


@pytest.mark.parametrize("packed,windowed", [(False, True), (True, False), (True, True)])
def test_mixed_list_windowed_and_packed(packed, windowed):
    c = mixed_case()
    want = mixed_want("k2_bitvec")
    n = c["codes"].size
    window = min_window(mixed_pats(), 2, sat_amd.SEM_FILTER_BITVEC) if windowed else None
    pm = mixed_engine("k2_bitvec")
    try:
        if packed:
            bits = max(1, (len(c["table"]) - 1).bit_length())
            pm.init_packed(sat_amd.pack_codes(c["codes"], bits), bits, n, c["table"], window=window)
        else:
            pm.init(c["codes"], c["table"], window=window)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=700 if windowed else 1 << 26))
        check_mixed_route(pm, "k2_bitvec")
        res = pm.residency()
    finally:
        pm.close()
    if windowed:
        assert res["window"] > 0 and res["loads"] > 1, res
    if packed:
        assert res["bits"] > 0, res
    assert got == want, (packed, windowed, len(got), len(want))


@pytest.mark.parametrize("name", ["k1_bitvec", "k2_inexact"])
def test_a_wide_tile_beside_a_narrow_one(name, monkeypatch):
    """PM_SEED_TILE cuts the main class in two (the hashed-piece plan, pm_edit_scan, at k = 2 as well): the first tile
    holds primers of 21..32 characters only and is built and verified as ever, the second one holds the long primers"""
    c = mixed_case()
    pats = mixed_pats(rest=False)
    k, sem, _, _, _ = MIXED_OPTS[name]
    order = sorted(range(len(pats)), key=lambda i: (len(pats[i]) > 32, i))   # (ids stay: the list is added in this order)
    main = [i for i in order if len(pats[i]) >= 20]
    monkeypatch.setenv("PM_SEED_TILE", str((len(main) + 1) // 2))
    assert all(len(pats[i]) <= 32 for i in main[:(len(main) + 1) // 2])
    pm = sat_amd.PatternMatch(k=k, indels=True, semantics=sem, long_edits=True)
    for i in order:
        pm.add_pattern(pats[i], i + 1)
    try:
        pm.init(c["codes"], c["table"])
        d = pm.describe()
        assert d.startswith("kernel=pm_edit_scan+pm_edits_verify tiles=2 ") and "wide tiles=1)" in d, d
        got = sat_amd.sorted_tuples(pm.find_all())
    finally:
        pm.close()
    assert got == mixed_want(name, rest=False)


# ---- 3. edges and zones ------------------------------------------------------------------------------------------------
def edges_case():
    """long primers that end in the stream's first L + 2k + 2 characters (first characters missing too) and in its last
    four (trailing pattern characters deleted), one across an end-of-sequence character at index 40 of its window"""
    rng = np.random.default_rng(5571)
    e0, e1, e2 = rand_seq(rng, 150), rand_seq(rng, 90), rand_seq(rng, 130)
    raw = (e0 + "\n" + e1 + "\n" + e2).encode()                      # the stream starts and ends with a base
    codes = synth.normalize(raw, TABLE)
    pats = []
    for L in (33, 40, 63, 64):
        pats += [e0[:L], "G" + e0[:L - 1], "CA" + e0[:L - 2], e0[2:L + 2], e0[1:12] + e0[13:L + 2], e0[3:L + 3]]
        pats += [e2[-L:], e2[-L:-1] + "C", e2[-L + 2:] + "GT", e2[-L - 2:-2], e2[-L - 1:-12] + e2[-11:] + "A", e2[-L - 3:-3]]
    pats += [e0[-40:] + "A" + e1[:23], e1[:40], e1[-40:], e1[1:41], e0[-41:-1]]
    pats += [rand_seq(rng, 22) for _ in range(5)] + [e1[10:32], e0[5:28]]
    return dict(codes=codes, table=TABLE, pats=pats, eos64=pats.index(e0[-40:] + "A" + e1[:23]) + 1)


@pytest.mark.parametrize("name", ["k2_auto", "k2_inexact", "k1_bitvec"])
def test_stream_edges(name):
    c = edges_case()
    codes, pats, n = c["codes"], c["pats"], c["codes"].size
    k, sem, selected, eng, _ = OPTS[name]
    want = oracle_hits(codes, TABLE, pats, k, eng)
    assert c["eos64"] not in {pid for _, pid, _ in want}             # nothing matches across an end-of-sequence character
    assert any(e < len(pats[pid - 1]) for e, pid, _ in want)         # a long primer with its first characters missing
    assert any(e >= n - 3 and len(pats[pid - 1]) > 32 for e, pid, _ in want)
    for chunk in (1 << 26, 37, 3):
        pm = engine(pats, k, sem)
        try:
            pm.init(codes, TABLE)
            long_route(pm, pats, selected)
            got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        finally:
            pm.close()
        assert got == want, (name, chunk, got, want)


@pytest.mark.parametrize("nbytes", [20, 33, 63, 64, 65, 70])
def test_tiny_streams(nbytes):
    rng = np.random.default_rng(5580 + nbytes)
    p = rand_seq(rng, 64)
    raw = {20: p[:20], 33: p[:33], 63: p[1:], 64: p, 65: "G" + p, 70: "GAT" + p + "TCA"}[nbytes]
    assert len(raw) == nbytes
    pats = [p, p[:33], p[:20], p[31:], rand_seq(rng, 40), p[:30] + rand_seq(rng, 34), rand_seq(rng, 21), p[:40] + p[41:]]
    codes = synth.normalize(raw.encode(), TABLE)
    for name in ("k2_auto", "k2_inexact", "k1_bitvec"):
        k, sem, selected, eng, _ = OPTS[name]
        want = oracle_hits(codes, TABLE, pats, k, eng)
        pm = engine(pats, k, sem)
        try:
            pm.init(codes, TABLE)
            long_route(pm, pats, selected)
            got = sat_amd.sorted_tuples(pm.find_all())
        finally:
            pm.close()
        assert got == want, (nbytes, name, got, want)
    if nbytes == 63:
        assert (63, 1, 1) in oracle_hits(codes, TABLE, pats, 2, O.SHIFT_AND_INEXACT)   # the 64-mer with its first character missing


def zones_case():
    """-3 8 and -5 8 on primers of 40..64 characters; every primer is planted exact, with an edit inside its zone, with
    one outside it and with both"""
    rng = np.random.default_rng(5590)
    other = lambda ch: BASES[(BASES.index(ch) + 1 + int(rng.integers(0, 3))) % 4]
    prim, zones, ents = [], [], []
    for i in range(24):
        L = (40, 47, 63, 64)[i % 4]
        p = rand_seq(rng, L)
        z = [(8, 0), (0, 8), (8, 8)][i % 3]
        inside = int(rng.integers(1, 7)) if z[0] and (i % 2 == 0 or not z[1]) else L - 2 - int(rng.integers(0, 6))
        outside = int(rng.integers(10, L - 10))

        def edit(s, j, kind):
            return s[:j] + other(s[j]) + s[j + 1:] if kind == 0 else s[:j] + s[j + 1:] if kind == 1 else s[:j] + other(s[j]) + s[j:]
        kind = i % 3
        ents += [rand_seq(rng, 30) + p + rand_seq(rng, 30), rand_seq(rng, 30) + edit(p, inside, kind) + rand_seq(rng, 30),
                 rand_seq(rng, 30) + edit(p, outside, kind) + rand_seq(rng, 30), rand_seq(rng, 30) + edit(edit(p, outside, kind), inside, 0) + rand_seq(rng, 30)]
        prim.append(p)
        zones.append(z)
    pats = prim + [rand_seq(rng, 24) for _ in range(40)]
    zones += [(0, 0)] * 40
    return dict(codes=synth.normalize(synth.stream(ents), TABLE), table=TABLE, pats=pats, zones=zones)


def test_zones_on_long_primers():
    c = zones_case()
    codes, pats, zones = c["codes"], c["pats"], c["zones"]
    for k in (2, 1):
        want = oracle_hits(codes, TABLE, pats, k, 5, zones)
        free = oracle_hits(codes, TABLE, pats, k, 5)
        assert len(want) < len(free), k                              # the zones remove hits, and leave some
        assert len({pid for _, pid, _ in want if pid <= 24}) == 24
        for chunk in (1 << 26, 193):
            pm = engine(pats, k, sat_amd.SEM_FILTER_BITVEC, zones=zones)
            try:
                pm.init(codes, TABLE)
                long_route(pm, pats, sat_amd.SEM_FILTER_BITVEC)
                got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
                if chunk == 193:
                    pm.reset()
                    pm.scan_candidates(0, codes.size, to_host=False)
                    assert sat_amd.sorted_tuples(pm.finalize_device(codes.size)) == want
            finally:
                pm.close()
            assert got == want, (k, chunk, len(got), len(want))


def iupac_case():
    """-w on a plain stream: 40-mers with one and two IUPAC letters (expanded into their variants, as in the main class),
    and some with three (residue)"""
    rng = np.random.default_rng(5591)
    ents = synth.make_entries(rng, 2, 6000)
    codes = synth.normalize(synth.stream(ents), TABLE)
    pats = synth.make_patterns(rng, ents, 40, length=40, planted=0.9, indel_frac=0.3, extras=False) + \
        synth.make_patterns(rng, ents, 40, length=24, minlen=20, planted=0.9, indel_frac=0.3, extras=False)
    pats = [p for p in pats if len(p) >= 20]
    for i in range(0, 40, 3):
        p = list(pats[i])
        if len(p) < 38:
            continue
        for j in (5, 36)[:1 + (i // 3) % 2]:                         # index 5, and index 36 beyond the first dword
            p[j] = {"A": "R", "C": "Y", "G": "K", "T": "W"}[p[j]]
        pats[i] = "".join(p)
    return dict(codes=codes, table=TABLE, pats=pats + [synth.revcomp_iupac(q) for q in pats], wildcards=True)


def three_letters(p):
    """three Ns: 64 concrete variants, more than the 16 the seed family expands"""
    p = list(p)
    for j in (5, 15, 25):
        p[j] = "N"
    return "".join(p)


def test_iupac_letters_in_long_primers():
    c = iupac_case()
    codes, allp = c["codes"], c["pats"]
    want = oracle_hits(codes, TABLE, allp, 2, 5, wildcards=True)
    assert any(set(allp[pid - 1]) - set("ACGT") and len(allp[pid - 1]) > 32 for _, pid, _ in want)   # a hit of a long primer with an IUPAC letter
    n_long = sum(1 for p in allp if 33 <= len(p) <= 64)
    for chunk in (1 << 26, 997):
        pm = engine(allp, 2, wildcards=True)
        try:
            pm.init(codes, TABLE)
            d = pm.describe()
            assert pm.selected()[1] == sat_amd.KERNEL_SEED and ("%d patterns %s %s" % (n_long, LONG_PHRASE, WIDE_PHRASE)) in d and "does not take" not in d, d
            got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        finally:
            pm.close()
        assert got == want, (chunk, len(got), len(want))


# ---- 4. routing, and the final hits against the former route's --------------------------------------------------------------
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
    pm = sat_amd.PatternMatch(k=case["k"], indels=True, semantics=case["sem"], wildcards=case.get("wildcards", False), long_edits=True)
    for i, p in enumerate(case["pats"]):
        z = case["zones"][i] if case.get("zones") else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    pm.init(np.load(case["codes"]), case["table"].encode())
    hits = sat_amd.sorted_tuples(pm.find_all())
    out.append({"selected": list(pm.selected()), "describe": pm.describe(), "hits": [list(h) for h in hits]})
    pm.close()
print("RESULT " + json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "tests"))


def run_child(case, env):
    r = subprocess.run([sys.executable, "-c", CHILD, str(case)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def outcome(codes, table, pats, k=2, bits=4, **kw):
    pm = engine(pats, k, bits=bits, **kw)
    try:
        pm.init(codes, table)
        hits = sat_amd.sorted_tuples(pm.find_all())
        return pm.selected(), pm.describe(), hits
    except sat_amd.PmError as e:
        return e.code, str(e), None
    finally:
        pm.close()


def test_off_in_a_fresh_process_is_the_former_route(tmp_path):
    """long_edits=False here, and long_edits=True with PM_LONG_EDITS=off in a fresh process (the environment is read by
    pm_create): selected() and describe() of the handle without the bit, and the same final hits as the long route gives"""
    lists = {"mixed": dict(mixed_case(), pats=mixed_pats()), "edges": edges_case(), "zones": zones_case(), "iupac": iupac_case()}
    cases, here = [], []
    for what, c in lists.items():
        np.save(tmp_path / (what + ".npy"), c["codes"])
        wild = bool(c.get("wildcards"))
        for k, sem in ((2, sat_amd.SEM_FILTER_BITVEC), (1, sat_amd.SEM_FILTER_BITVEC)) + (() if wild else ((2, sat_amd.SEM_SHIFT_AND_INEXACT),)):
            zones = c.get("zones") if sem == sat_amd.SEM_FILTER_BITVEC else None
            kw = dict(sem=sem, zones=zones, wildcards=wild)
            off = outcome(c["codes"], c["table"], c["pats"], k, bits=0, **kw)
            on = outcome(c["codes"], c["table"], c["pats"], k, bits=4, **kw)
            assert LONG_PHRASE not in off[1] and LONG_PHRASE in on[1] and off[2] is not None, (what, k, off[:2], on[:2])
            assert off[2] == on[2], (what, k, sem)
            here.append(off)
            cases.append(dict(k=k, sem=sem, pats=c["pats"], zones=zones, wildcards=wild, codes=str(tmp_path / (what + ".npy")), table=bytes(c["table"]).decode()))
    case = tmp_path / "case.json"
    case.write_text(json.dumps({"cases": cases}))
    env = {x: v for x, v in os.environ.items() if x != "PM_LONG_EDITS"}
    for off, child in zip(here, run_child(case, dict(env, PM_LONG_EDITS="off"))):
        assert (tuple(child["selected"]), child["describe"]) == (off[0], off[1]), (child["describe"], off[1])
        assert [tuple(h) for h in child["hits"]] == off[2]


def routing_lists():
    rng = np.random.default_rng(5593)
    ents = synth.make_entries(rng, 2, 6000)
    codes = synth.normalize(synth.stream(ents), TABLE)
    mids = synth.make_patterns(rng, ents, 30, length=24, minlen=20, planted=0.8, extras=False)
    mids = [p for p in mids if len(p) >= 20]
    longs = synth.make_patterns(rng, ents, 10, length=64, minlen=33, planted=0.8, indel_frac=0, extras=False)
    return ents, codes, mids, longs


def test_each_bit_moves_its_own_option_set():
    """pm_config.long_patterns = 0 .. 7 on one list at k = 0, -K 2 and -k 2: a handle is on its long route exactly when
    the bit of its option set is given, and the hits never change"""
    ents, codes, mids, longs = routing_lists()
    mixed = mids + longs
    for own, kw in ((2, dict(k=0)), (1, dict(k=2, indels=False)), (4, dict(k=2, indels=True))):
        base = outcome(codes, TABLE, mixed, bits=0, **kw)
        assert LONG_PHRASE not in base[1], base[1]
        on = None
        for bits in range(1, 8):
            got = outcome(codes, TABLE, mixed, bits=bits, **kw)
            assert got[2] == base[2], (kw, bits)
            if bits & own:
                assert ("with 10 patterns " + LONG_PHRASE) in got[1], (kw, bits, got[1])
                on = on or got
                assert got[:2] == on[:2], (kw, bits)
            else:
                assert got[:2] == base[:2], (kw, bits, got[1], base[1])


def test_routing():
    """lists and option sets the route does not apply to: selected(), describe() and the hits are those of the handle
    without the bit, byte for byte"""
    ents, codes, mids, longs = routing_lists()
    mixed = mids + longs
    z6 = [(6, 0)] * len(mixed)
    cases = {
        "-k 2 exact_halves": dict(pats=mixed, sem=sat_amd.SEM_EXACT_HALVES),
        "-k 1 auto (exact_halves)": dict(pats=mixed, k=1),
        "-k 2 exact_bases": dict(pats=mixed, sem=sat_amd.SEM_EXACT_BASES, zones=z6),
        "k = 3": dict(pats=mixed, k=3),
        "-K 2": dict(pats=mixed, indels=False),
        "k = 0": dict(pats=mixed, k=0),
        "seed kernels on request": dict(pats=mixed, kernel=sat_amd.KERNEL_SEED),
        "bit-parallel kernels on request": dict(pats=mixed, kernel=sat_amd.KERNEL_BITPAR),
        "no long primer": dict(pats=mids),
        "the only long primer has 65 characters": dict(pats=mids + [ents[0][200:265]]),
        "long primers with three IUPAC letters": dict(pats=mids + [three_letters(p) for p in longs], wildcards=True),
    }
    for what, kw in cases.items():
        off = outcome(codes, TABLE, bits=0, **kw)
        on = outcome(codes, TABLE, bits=4, **kw)
        assert off[:2] == on[:2], (what, off[:2], on[:2])
        assert LONG_PHRASE not in on[1], (what, on[1])
        assert off[2] == on[2], what
    on = outcome(codes, TABLE, mixed + [ents[0][200:265]], bits=4)   # 65 characters: residue beside the long route
    assert ("10 patterns " + LONG_PHRASE) in on[1] and "for 1 patterns the seed plan does not take" in on[1], on[1]


# ---- 5. counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 2])
def test_mixed_list_counts(M):
    """count_all on a long-edit handle: the count rule on the oracle's hits (patterns beyond the device re-alignment's
    length go through the host's)"""
    c = mixed_case()
    pats = mixed_pats(False)
    want = mixed_want("k2_bitvec", False)
    if "eds" not in c:
        text = O.Text(c["codes"], c["table"])
        c["eds"] = [O.cli_align(text, pats[pid - 1], end, 2, True)[3] for end, pid, _ in want]
    wc, wcap, winfo = count_rule.tally(want, lambda i: c["eds"][i], len(pats), 2, M)
    pm = mixed_engine("k2_bitvec", False)
    try:
        pm.init(c["codes"], c["table"])
        check_mixed_route(pm, "k2_bitvec", False)
        counts, capped, info = pm.count_all(max_count=M)
    finally:
        pm.close()
    assert counts.tolist() == wc
    assert capped.tolist() == wcap
    for f in ("tallied", "skipped", "bogus"):
        assert info[f] == winfo[f], (f, info[f], winfo[f])
    assert info["aligned_host"] > 0, info
