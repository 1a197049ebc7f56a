"""GPU: exact_halves -k 1 / -k 2 lists with primers of 33..64 characters on the halves plan (bit 3 of
pm_config.long_patterns, long_halves=True; csrc/pm_halves.h, csrc/pm_seed.hip pm_half_scan<true> + pm_half_verify_wide and
the HALVES && WIDE instance of pm_seed_scan, csrc/pm_extend.hip pm_seed_extend<32>).

`-k 1` selects exact_halves by itself when every primer has 12 characters or more (select.cc:121-126), and exact_halves
keeps one engine: one long primer took the whole list to the bit-parallel family.  A seed of the plan is an exact
occurrence of a half; with the bit set a half of 16..32 characters is tested by pm_half_scan on the bases the lane
carries (a slot of a second kind), by pm_half_verify_wide on 64-byte records, and extended on rows of 32 codes.  The
route is a permission of the caller, off by default.  Here: every one-edit text of a 33-, a 64- and a 53-mer, every
two-edit text of the 33-mer, a mixed list through every interface, shared keys, a wide tile beside a narrow one, the
Bloom form, the stream's edges, N and end-of-sequence characters, zones, a raw stream, the routing rules, the final hits
against the former route's and the counts.  Expected values come from the oracle."""
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
WIDE_PHRASE = "(pm_half_verify_wide, wide tiles="
HALVES_ENGINES = range(O.EXACT_HALVES_KT, O.EXACT_HALVES_SA + 2)   # select.cc's 12 .. 15: exact_halves over one of its exact engines


# ---- helpers (as tests/test_gpu_long_edits.py builds its streams) --------------------------------------------------------
def one_edit(w):
    out = set()
    for i in range(len(w)):
        out.add(w[:i] + w[i + 1:])
        for c in "ACGT":
            if c != w[i]:
                out.add(w[:i] + c + w[i + 1:])
    for i in range(len(w) + 1):
        for c in "ACGT":
            out.add(w[:i] + c + w[i:])
    return out


def edit_variants(p, k):
    level, seen = {p}, {p}
    for _ in range(k):
        nxt = set()
        for w in level:
            nxt |= one_edit(w)
        level = nxt - seen
        seen |= nxt
    return seen


def stream_of(variants, rng):
    """variants between end-of-sequence characters, two to four random bases in front of each and up to three behind"""
    parts = []
    for v in variants:
        pad_l = "".join(rng.choice(BASES, size=int(rng.integers(2, 5))).tolist())
        pad_r = "".join(rng.choice(BASES, size=int(rng.integers(0, 4))).tolist())
        parts.append(pad_l + v + pad_r)
    return parts


def rand_seq(rng, n):
    return "".join(rng.choice(BASES, size=n).tolist())


def engine(pats, k, sem=sat_amd.SEM_AUTO, bits=8, zones=None, indels=True, **kw):
    """bits: pm_config.long_patterns (1: -K, 2: k = 0, 4: -k on the edit plan, 8: -k on the halves plan)"""
    pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sem, long_patterns=bool(bits & 1), long_exact=bool(bits & 2),
                              long_edits=bool(bits & 4), long_halves=bool(bits & 8), **kw)
    for i, p in enumerate(pats):
        z = zones[i] if zones else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    return pm


def oracle_hits(codes, table, pats, k, eng=None, zones=None):
    """eng None: the automatic choice, which has to be exact_halves"""
    esb = [z[0] for z in zones] if zones else None
    eeb = [z[1] for z in zones] if zones else None
    text = O.Text(codes, table)
    if eng is None:
        eng = O.pick_engine(text, pats, k, True, esb, eeb)
        assert eng in HALVES_ENGINES, eng
    return O.sorted_tuples(O.find_all(text, pats, engine=eng, k=k, indels=True, esb=esb, eeb=eeb))


def nlong(pats):
    return sum(1 for p in pats if 33 <= len(p) <= 64)


def long_route(pm, pats, wide_tiles=None, form=None):
    d = pm.describe()
    assert pm.selected() == (sat_amd.SEM_EXACT_HALVES, sat_amd.KERNEL_SEED), d
    assert ("with %d patterns %s %s" % (nlong(pats), LONG_PHRASE, WIDE_PHRASE)) in d, d
    assert "does not take" not in d, d
    if wide_tiles is not None:
        assert ("wide tiles=%d)" % wide_tiles) in d, d
    if form is not None:
        assert d.startswith("kernel=%s " % form), d
    return d


def run(pm, codes, table, chunk=1 << 26):
    pm.init(codes, table)
    return sat_amd.sorted_tuples(pm.find_all(chunk=chunk))


def check(pats, codes, table, k, sem=sat_amd.SEM_AUTO, eng=None, zones=None, chunks=(1 << 26,), form=None, want=None):
    want = oracle_hits(codes, table, pats, k, eng, zones) if want is None else want
    for chunk in chunks:
        pm = engine(pats, k, sem, zones=zones)
        try:
            got = run(pm, codes, table, chunk)
            long_route(pm, pats, form=form)
        finally:
            pm.close()
        assert got == want, (k, chunk, len(got), len(want), sorted(set(got) ^ set(want))[:10])
    return want


# ---- 1. every one-edit text of a 33-, a 64- and a 53-mer; every two-edit text of the 33-mer -------------------------------
@pytest.mark.parametrize("L", [33, 64, 53])
def test_every_one_edit_text_under_k1_auto(L):
    """33: halves 16 | 17, a short half with a long partner; 64: 32 | 32, the half starts at the first carried base;
    53: 26 | 27, one base more than the slot holds.  No 11-mer in the list: the automatic choice IS exact_halves"""
    rng = np.random.default_rng(5600 + L)
    p = rand_seq(rng, L)
    variants = sorted(edit_variants(p, 1))
    assert len(variants) > 3 * L + L + 3 * (L + 1) - 40
    codes = synth.normalize(synth.stream(stream_of(variants, rng)), TABLE)
    pats = [p] + [rand_seq(rng, int(rng.integers(20, 33))) for _ in range(300)] + [rand_seq(rng, int(rng.integers(33, 65))) for _ in range(100)]
    want = check(pats, codes, TABLE, 1, form="pm_half_scan+pm_half_verify")
    own = sum(1 for _, pid, _ in want if pid == 1)
    print("L = %d: %d one-edit texts, %d hits of the primer" % (L, len(variants), own))
    assert own == len(variants)                                      # one hit per text


def test_every_two_edit_text_of_a_33_mer_under_k2_exact_halves():
    rng = np.random.default_rng(5633)
    p = rand_seq(rng, 33)
    variants = sorted(edit_variants(p, 2))
    assert len(variants) > 20000
    codes = synth.normalize(synth.stream(stream_of(variants, rng)), TABLE)
    assert codes.size < 1200000
    pats = [p] + [rand_seq(rng, int(rng.integers(20, 33))) for _ in range(300)] + [rand_seq(rng, int(rng.integers(33, 65))) for _ in range(100)]
    want = check(pats, codes, TABLE, 2, sat_amd.SEM_EXACT_HALVES, O.EXACT_HALVES_KT)
    own = sum(1 for _, pid, _ in want if pid == 1)
    print("%d texts within two edits, %d hits of the primer" % (len(variants), own))
    assert own > 10000                                               # (two edits that touch both halves leave no exact half: no seed)


# ---- 2. a mixed list on text with repeats and N runs, through every interface ------------------------------------------------
_MIXED = {}


def mixed_case():
    """primers of 20..32, 33..64 (33, 34, 42, 52, 53, 63 and 64 among them) and 16..19 characters -- the Bloom form -- cut
    from the stream with up to two edits, both strands; no N, nothing above 64"""
    if not _MIXED:
        rng = np.random.default_rng(5670)
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
                ne = (len(out) // 7) % 2 if len(out) < len(fixed) else int(rng.integers(0, 3))   # (the fixed lengths: exact, then with one edit)
                w = synth.mutate(rng, w, nsub=int(ne > 0), nins=int(ne > 1 and rng.random() < 0.5), ndel=int(ne > 1 and rng.random() < 0.5))
                w = "".join(w)[:L]
                if len(w) == L and "N" not in w:
                    out.append(w)
            return out
        long_p = cut(40, 33, 64, fixed=(33, 34, 42, 52, 53, 63, 64) * 2)
        mids = cut(50, 20, 32)
        shorts = cut(12, 16, 19)
        table = synth.table_for(ents)
        codes = synth.normalize(synth.stream(ents), table)
        both = lambda ps: ps + [synth.revcomp(p) for p in ps]
        _MIXED.update(ents=ents, ranked=both(mids + long_p), bloom=both(mids + long_p + shorts), table=table, codes=codes, want={})
    return _MIXED


def mixed_want(which, k):
    c = mixed_case()
    if (which, k) not in c["want"]:
        c["want"][(which, k)] = oracle_hits(c["codes"], c["table"], c[which], k, None if k == 1 else O.EXACT_HALVES_KT)
    return c["want"][(which, k)]


FORM = {"ranked": "pm_half_scan+pm_half_verify", "bloom": "pm_seed_scan"}


def test_mixed_list_condition():
    c = mixed_case()
    for which in ("ranked", "bloom"):
        pats = c[which]
        for k in (1, 2):
            want = mixed_want(which, k)
            assert {len(pats[pid - 1]) for _, pid, _ in want} >= {33, 34, 42, 52, 53, 63, 64}, (which, k)
            assert any(20 <= len(pats[pid - 1]) <= 32 for _, pid, _ in want)
            assert any(d == k for _, pid, d in want if len(pats[pid - 1]) > 32), (which, k)
    assert any(len(c["bloom"][pid - 1]) < 20 for _, pid, _ in mixed_want("bloom", 1))


@pytest.mark.parametrize("which", ["ranked", "bloom"])
@pytest.mark.parametrize("k", [1, 2])
def test_mixed_list_find_all_in_ranges(which, k):
    """pm_scan in ranges of 2^26, 5,000 and 193"""
    c = mixed_case()
    check(c[which], c["codes"], c["table"], k, sat_amd.SEM_AUTO if k == 1 else sat_amd.SEM_EXACT_HALVES, chunks=(1 << 26, 5000, 193),
          form=FORM[which] if k == 1 else "pm_seed_scan", want=mixed_want(which, k))   # (k = 2: a fifth of the halves of 20..32 nt primers do not fit the partner test, under 90 % fit: the Bloom form)


@pytest.mark.parametrize("which", ["ranked", "bloom"])
def test_mixed_list_device_stages(which):
    """scan_candidates + finalize_device in one call (pm_halves_rule), and two shards' candidates through pm_finalize"""
    c = mixed_case()
    want = mixed_want(which, 1)
    n = c["codes"].size
    pm = engine(c[which], 1)
    try:
        pm.init(c["codes"], c["table"])
        pm.scan_candidates(0, n, to_host=False)
        long_route(pm, c[which], form=FORM[which])
        assert sat_amd.sorted_tuples(pm.finalize_device(n)) == want
        pm.reset()
        cuts = [0, n // 3 + 5, n]
        parts = [pm.scan_candidates(cuts[i], cuts[i + 1]) for i in range(2)]
        pm.reset()
        assert sat_amd.sorted_tuples(pm.finalize(np.concatenate(parts[::-1]), n, last=True)) == want
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
    pats = c["ranked"]
    want = mixed_want("ranked", 1)
    n = c["codes"].size
    window = min_window(pats, 1) if windowed else None
    pm = engine(pats, 1)
    try:
        if packed:
            bits = max(1, (len(c["table"]) - 1).bit_length())
            pm.init_packed(sat_amd.pack_codes(c["codes"], bits), bits, n, c["table"], window=window)
        else:
            pm.init(c["codes"], c["table"], window=window)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=700 if windowed else 1 << 26))
        long_route(pm, pats)
        res = pm.residency()
    finally:
        pm.close()
    if windowed:
        assert res["window"] > 0 and res["loads"] > 1, res
    if packed:
        assert res["bits"] > 0, res
    assert got == want, (packed, windowed, len(got), len(want))


@pytest.mark.parametrize("M", [0, 2])
def test_mixed_list_counts(M):
    """count_all on such a handle: the count rule on the oracle's hits (patterns beyond the device re-alignment's length go
    through the host's)"""
    c = mixed_case()
    pats = c["ranked"]
    want = mixed_want("ranked", 1)
    if "eds" not in c:
        text = O.Text(c["codes"], c["table"])
        c["eds"] = [O.cli_align(text, pats[pid - 1], end, 1, True)[3] for end, pid, _ in want]
    wc, wcap, winfo = count_rule.tally(want, lambda i: c["eds"][i], len(pats), 1, M)
    pm = engine(pats, 1)
    try:
        pm.init(c["codes"], c["table"])
        long_route(pm, pats)
        counts, capped, info = pm.count_all(max_count=M)
    finally:
        pm.close()
    assert counts.tolist() == wc
    assert capped.tolist() == wcap
    for f in ("tallied", "skipped", "bogus"):
        assert info[f] == winfo[f], (f, info[f], winfo[f])


def test_a_wide_tile_beside_a_narrow_one(monkeypatch):
    """PM_SEED_TILE cuts the halves in two tiles: the first holds halves of primers of 20..32 characters only and is built
    and scanned as ever, the second holds the long primers'"""
    c = mixed_case()
    pats = c["ranked"]
    order = sorted(range(len(pats)), key=lambda i: (len(pats[i]) > 32, i))   # (ids stay: the list is added in this order)
    nshort = sum(1 for p in pats if len(p) <= 32)
    assert nshort * 2 >= len(pats)
    monkeypatch.setenv("PM_SEED_TILE", str(2 * nshort))                     # halves per tile
    pm = sat_amd.PatternMatch(k=1, indels=True, long_halves=True)
    for i in order:
        pm.add_pattern(pats[i], i + 1)
    try:
        pm.init(c["codes"], c["table"])
        d = pm.describe()
        assert " tiles=2 " in d.split(" with ")[0] and "wide tiles=1)" in d, d   # (the narrow tile takes the form its own halves ask for)
        got = sat_amd.sorted_tuples(pm.find_all())
    finally:
        pm.close()
    assert got == mixed_want("ranked", 1)


# ---- 3. shared keys ------------------------------------------------------------------------------------------------------
def test_halves_that_share_their_key():
    """a 20-mer's half and a 40-mer's half share their last ten bases (a mixed chain of the two slot kinds), and nine
    halves share one key (the walk flag: pm_half_verify_wide resolves them)"""
    rng = np.random.default_rng(5680)
    key, key9 = rand_seq(rng, 10), rand_seq(rng, 10)
    p20 = rand_seq(rng, 10) + rand_seq(rng, 10)
    p20 = p20[:0] + key + p20[10:]                                   # left half = key
    p40 = rand_seq(rng, 10) + key + rand_seq(rng, 20)                # left half ends in key
    p40r = rand_seq(rng, 30) + key                                   # right half ends in key
    nine = [rand_seq(rng, 6 + i) + key9 + rand_seq(rng, 16 + i) for i in range(5)] + [rand_seq(rng, 17 + i) + rand_seq(rng, 7 + i) + key9 for i in range(4)]
    for q in nine[:5]:
        assert q[len(q) // 2 - 10:len(q) // 2] == key9, q
    for q in nine[5:]:
        assert q.endswith(key9)
    pats = [p20, p40, p40r] + nine + [rand_seq(rng, int(rng.integers(20, 50))) for _ in range(30)]
    assert any(len(q) > 32 for q in nine) and any(len(q) <= 32 for q in nine)
    ents = []
    for p in pats[:12]:
        for v in (p, p[:3] + p[4:], p[:-4] + "A" + p[-4:], p[:len(p) // 2 - 12] + "T" + p[len(p) // 2 - 12:]):
            ents.append(rand_seq(rng, 40) + v + rand_seq(rng, 40))
    ents.append(rand_seq(rng, 30) + key + rand_seq(rng, 30) + key9 + rand_seq(rng, 30))   # the keys alone
    codes = synth.normalize(synth.stream(ents), TABLE)
    for k in (1, 2):
        want = check(pats, codes, TABLE, k, sat_amd.SEM_AUTO if k == 1 else sat_amd.SEM_EXACT_HALVES, None if k == 1 else O.EXACT_HALVES_KT,
                     form="pm_half_scan+pm_half_verify")
        assert {pid for _, pid, _ in want} >= set(range(1, 13)), k


# ---- 4. the stream's edges, N and end-of-sequence characters, zones, a raw stream ---------------------------------------------
@pytest.mark.parametrize("nbytes", [20, 33, 40, 63, 64, 65, 70])
def test_tiny_streams(nbytes):
    rng = np.random.default_rng(5690 + nbytes)
    p = rand_seq(rng, 64)
    raw = {20: p[:20], 33: p[:33], 40: p[20:60], 63: p[1:], 64: p, 65: "G" + p, 70: "GAT" + p + "TCA"}[nbytes]
    assert len(raw) == nbytes
    pats = [p, p[:33], p[:20], p[31:], rand_seq(rng, 40), p[:30] + rand_seq(rng, 34), rand_seq(rng, 21), p[:40] + p[41:], p[20:60], p[24:60]]
    codes = synth.normalize(raw.encode(), TABLE)
    for k in (1, 2):
        check(pats, codes, TABLE, k, sat_amd.SEM_AUTO if k == 1 else sat_amd.SEM_EXACT_HALVES, None if k == 1 else O.EXACT_HALVES_KT)


def test_stream_edges():
    """long primers that end in the stream's last character (and hang over it: the extension reads the zero padding), and
    that start at index 0 with their first characters missing"""
    rng = np.random.default_rng(5691)
    e0, e1, e2 = rand_seq(rng, 150), rand_seq(rng, 90), rand_seq(rng, 130)
    raw = (e0 + "\n" + e1 + "\n" + e2).encode()                      # the stream starts and ends with a base
    codes = synth.normalize(raw, TABLE)
    n = codes.size
    pats = []
    for L in (33, 40, 53, 63, 64):
        pats += [e0[:L], "G" + e0[:L - 1], "CA" + e0[:L - 2], e0[2:L + 2], e0[1:12] + e0[13:L + 2], e0[3:L + 3]]
        pats += [e2[-L:], e2[-L:-1] + "C", e2[-L + 2:] + "AA", e2[-L - 2:-2], e2[-L - 1:-12] + e2[-11:],e2[-L - 3:-3], e2[-L + 1:] + "A"]
    pats += [e0[-40:] + "A" + e1[:23], e1[:40], e1[-40:], e1[1:41], e0[-41:-1]]
    pats += [rand_seq(rng, 22) for _ in range(5)] + [e1[10:32], e0[5:28]]
    assert all(16 <= len(p) <= 64 for p in pats)
    for k in (1, 2):
        want = check(pats, codes, TABLE, k, sat_amd.SEM_AUTO if k == 1 else sat_amd.SEM_EXACT_HALVES, None if k == 1 else O.EXACT_HALVES_KT,
                     chunks=(1 << 26, 37, 3))
        assert any(e == n and len(pats[pid - 1]) > 32 for e, pid, _ in want), k      # a long primer ending in the last character
        if k == 2:                                                   # one with its first character missing (the reference's DP prices that at 2)
            assert any(e < len(pats[pid - 1]) and pats[pid - 1][0] == "G" and pats[pid - 1][1:] == e0[:e] for e, pid, _ in want)
        assert pats.index(e0[-40:] + "A" + e1[:23]) + 1 not in {pid for _, pid, _ in want}


def test_n_and_eos_in_the_stream():
    """an end-of-sequence character inside the partner; an N in place of an `A` six bases in front of a half's key, on a
    table where the N's 2-bit word is the A's: the slot passes the window, the raw test rejects it"""
    rng = np.random.default_rng(5692)
    table = b"ACGTN\n"                                               # N = 4: the 2-bit word of A
    prim, ents = [], []
    for L in (33, 40, 53, 64, 34, 63):
        p = list(rand_seq(rng, L))
        h = L // 2
        p[h - 16] = "A"                                              # six bases in front of the left half's key
        p[L - 16] = "A"                                              # ... and of the right half's
        p = "".join(p)
        prim.append(p)
        pad = lambda: rand_seq(rng, 35)
        ents += [pad() + p + pad(),
                 pad() + p[:h - 16] + "N" + p[h - 15:] + pad(), pad() + p[:L - 16] + "N" + p[L - 15:] + pad(),
                 pad() + p[:h - 16] + "N" + p[h - 15:L - 16] + "N" + p[L - 15:] + pad(),
                 pad() + p[:h + 5] + "\n" + p[h + 6:] + pad(), pad() + p[:5] + "\n" + p[6:] + pad(),
                 pad() + p[:h + 5] + "\n" + p[h + 5:] + pad()]
    raw = ("\n" + "".join(e + "\n" for e in ents)).encode()
    codes = synth.normalize(raw, table)
    pats = prim + [rand_seq(rng, 24) for _ in range(20)]
    for k in (1, 2):
        want = check(pats, codes, table, k, sat_amd.SEM_AUTO if k == 1 else sat_amd.SEM_EXACT_HALVES, None if k == 1 else O.EXACT_HALVES_KT)
        assert {pid for _, pid, _ in want} >= set(range(1, 7))
    raw_codes = np.frombuffer(raw, dtype=np.uint8).copy()            # the same on the raw stream (N: the 2-bit word of G there)
    want = oracle_hits(raw_codes, None, pats, 1)
    pm = engine(pats, 1)
    try:
        pm.init(raw_codes)
        got = sat_amd.sorted_tuples(pm.find_all())
        long_route(pm, pats)
    finally:
        pm.close()
    assert got == want and len(want) >= 6


def test_zones_on_long_primers():
    """-5 8 and -3 8 on primers of 40..64 characters, and a 5' zone of 20 on a 33-mer (longer than its half); every primer
    is planted exact, with an edit inside its zone, with one outside it and with both"""
    rng = np.random.default_rng(5693)
    other = lambda ch: BASES[(BASES.index(ch) + 1 + int(rng.integers(0, 3))) % 4]
    prim, zones, ents = [], [], []
    for i in range(24):
        L = (40, 47, 63, 64, 33)[i % 5]
        p = rand_seq(rng, L)
        z = (20, 0) if L == 33 else [(8, 0), (0, 8), (8, 8)][i % 3]
        inside = int(rng.integers(1, z[0] - 1)) if z[0] and (i % 2 == 0 or not z[1]) else L - 2 - int(rng.integers(0, 6))
        outside = int(rng.integers(22, L - 10))

        def edit(s, j, kind):
            return s[:j] + other(s[j]) + s[j + 1:] if kind == 0 else s[:j] + s[j + 1:] if kind == 1 else s[:j] + other(s[j]) + s[j:]
        kind = i % 3
        ents += [rand_seq(rng, 30) + p + rand_seq(rng, 30), rand_seq(rng, 30) + edit(p, inside, kind) + rand_seq(rng, 30),
                 rand_seq(rng, 30) + edit(p, outside, kind) + rand_seq(rng, 30), rand_seq(rng, 30) + edit(edit(p, outside, kind), inside, 0) + rand_seq(rng, 30)]
        prim.append(p)
        zones.append(z)
    pats = prim + [rand_seq(rng, 24) for _ in range(40)]
    zones += [(0, 0)] * 40
    codes = synth.normalize(synth.stream(ents), TABLE)
    for k in (1, 2):
        eng = None if k == 1 else O.EXACT_HALVES_KT
        sem = sat_amd.SEM_AUTO if k == 1 else sat_amd.SEM_EXACT_HALVES
        want = check(pats, codes, TABLE, k, sem, eng, zones=zones, chunks=(1 << 26, 193))
        free = oracle_hits(codes, TABLE, pats, k, eng)
        assert len(want) < len(free), k                              # the zones remove hits, and leave some
        assert len({pid for _, pid, _ in want if pid <= 24}) == 24


# ---- 5. routing, and the final hits against the former route's --------------------------------------------------------------
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
    pm = sat_amd.PatternMatch(k=case["k"], indels=True, semantics=case["sem"], long_halves=True)
    for i, p in enumerate(case["pats"]):
        pm.add_pattern(p, i + 1)
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


def outcome(codes, table, pats, k=1, bits=8, **kw):
    pm = engine(pats, k, bits=bits, **kw)
    try:
        pm.init(codes, table)
        hits = sat_amd.sorted_tuples(pm.find_all())
        return pm.selected(), pm.describe(), hits
    except sat_amd.PmError as e:
        return e.code, str(e), None
    finally:
        pm.close()


def child_cases(tmp_path):
    c = mixed_case()
    np.save(tmp_path / "mixed.npy", c["codes"])
    cases = [dict(k=k, sem=sem, pats=c[which], codes=str(tmp_path / "mixed.npy"), table=bytes(c["table"]).decode(), which=which)
             for which in ("ranked", "bloom") for k, sem in ((1, sat_amd.SEM_AUTO), (2, sat_amd.SEM_EXACT_HALVES))]
    path = tmp_path / "case.json"
    path.write_text(json.dumps({"cases": cases}))
    return cases, path


def test_off_in_a_fresh_process_is_the_former_route(tmp_path):
    """long_halves=False here, and long_halves=True with PM_LONG_HALVES=off in a fresh process (the environment is read by
    pm_create): selected() and describe() of the handle without the bit -- the bit-parallel family -- and the same final
    hits as the long route gives and the oracle"""
    c = mixed_case()
    cases, path = child_cases(tmp_path)
    here = []
    for case in cases:
        off = outcome(c["codes"], c["table"], case["pats"], case["k"], bits=0, sem=case["sem"])
        on = outcome(c["codes"], c["table"], case["pats"], case["k"], bits=8, sem=case["sem"])
        assert off[0] == (sat_amd.SEM_EXACT_HALVES, sat_amd.KERNEL_BITPAR) and on[0] == (sat_amd.SEM_EXACT_HALVES, sat_amd.KERNEL_SEED), (off[:2], on[:2])
        assert LONG_PHRASE not in off[1] and LONG_PHRASE in on[1], (off[1], on[1])
        assert off[2] == on[2] == mixed_want(case["which"], case["k"]), (case["which"], case["k"])
        here.append(off)
    env = {x: v for x, v in os.environ.items() if x not in ("PM_LONG_HALVES", "PM_HALF_SCAN")}
    for off, child in zip(here, run_child(path, dict(env, PM_LONG_HALVES="off"))):
        assert (tuple(child["selected"]), child["describe"]) == (off[0], off[1]), (child["describe"], off[1])
        assert [tuple(h) for h in child["hits"]] == off[2]


def test_bloom_form_in_a_fresh_process(tmp_path):
    """PM_HALF_SCAN=bloom: the HALVES && WIDE instance of pm_seed_scan for every list"""
    cases, path = child_cases(tmp_path)
    env = {x: v for x, v in os.environ.items() if x not in ("PM_LONG_HALVES", "PM_HALF_SCAN")}
    for case, child in zip(cases, run_child(path, dict(env, PM_HALF_SCAN="bloom"))):
        d = child["describe"]
        assert d.startswith("kernel=pm_seed_scan ") and (LONG_PHRASE + " " + WIDE_PHRASE) in d, d
        assert [tuple(h) for h in child["hits"]] == mixed_want(case["which"], case["k"]), (case["which"], case["k"])


def routing_lists():
    rng = np.random.default_rng(5694)
    ents = synth.make_entries(rng, 2, 6000)
    codes = synth.normalize(synth.stream(ents), TABLE)
    mids = synth.make_patterns(rng, ents, 30, length=24, minlen=20, planted=0.8, extras=False)
    mids = [p for p in mids if len(p) >= 20]
    longs = synth.make_patterns(rng, ents, 10, length=64, minlen=33, planted=0.8, indel_frac=0, extras=False)
    longs = [p for p in longs if 33 <= len(p) <= 64]
    return ents, codes, mids, longs


def test_only_bit_8_moves_exact_halves_k_lists():
    """bits 1, 2, 4 and 7 leave an exact_halves -k list with a 40-mer on the bit-parallel family; bit 8 alone and in every
    sum takes it to the halves plan; the hits never change"""
    ents, codes, mids, longs = routing_lists()
    mixed = mids + longs + [ents[0][300:340]]
    for kw in (dict(k=1), dict(k=2, sem=sat_amd.SEM_EXACT_HALVES)):
        base = outcome(codes, TABLE, mixed, bits=0, **kw)
        assert base[0] == (sat_amd.SEM_EXACT_HALVES, sat_amd.KERNEL_BITPAR) and LONG_PHRASE not in base[1], base[:2]
        on = None
        for bits in range(1, 16):
            got = outcome(codes, TABLE, mixed, bits=bits, **kw)
            assert got[2] == base[2], (kw, bits)
            if bits & 8:
                assert ("with %d patterns %s %s" % (nlong(mixed), LONG_PHRASE, WIDE_PHRASE)) in got[1], (kw, bits, got[1])
                on = on or got
                assert got[:2] == on[:2], (kw, bits)
            else:
                assert got[:2] == base[:2], (kw, bits, got[1], base[1])


def test_bit_8_leaves_the_other_option_sets_alone():
    """-K 2, k = 0 and filter_bitvec -k handles: with bit 8 the handle of no bit, beside bits 1, 2 and 4 the handle of
    those bits"""
    ents, codes, mids, longs = routing_lists()
    mixed = mids + longs
    for kw in (dict(k=2, indels=False), dict(k=0), dict(k=2, sem=sat_amd.SEM_FILTER_BITVEC), dict(k=1, sem=sat_amd.SEM_FILTER_BITVEC),
               dict(k=1, indels=False, sem=sat_amd.SEM_EXACT_HALVES), dict(k=0, sem=sat_amd.SEM_EXACT_HALVES)):
        for without in (0, 7):
            off = outcome(codes, TABLE, mixed, bits=without, **kw)
            on = outcome(codes, TABLE, mixed, bits=without | 8, **kw)
            assert off == on, (kw, without, off[:2], on[:2])
            assert WIDE_PHRASE not in on[1]


def test_routing():
    """lists and option sets the route does not apply to: selected(), describe() and the hits are those of the handle
    without the bit, byte for byte"""
    ents, codes, mids, longs = routing_lists()
    mixed = mids + longs
    with_n = ents[0][500:509] + "N" + ents[0][510:540]
    cases = {
        "a 65-mer in the list": dict(pats=mixed + [ents[0][200:265]]),
        "a 15-mer in the list": dict(pats=mixed + [ents[0][700:715]]),
        "a primer with an N in the list": dict(pats=mixed + [with_n]),
        "k = 3": dict(pats=mixed, k=3, sem=sat_amd.SEM_EXACT_HALVES),
        "seed kernels on request": dict(pats=mids, kernel=sat_amd.KERNEL_SEED),
        "bit-parallel kernels on request": dict(pats=mixed, kernel=sat_amd.KERNEL_BITPAR),
        "no long primer": dict(pats=mids),
        "-w": dict(pats=mixed, wildcards=True),
        "-k 2 exact_bases": dict(pats=mixed, k=2, sem=sat_amd.SEM_EXACT_BASES, zones=[(6, 0)] * len(mixed)),
        "-k 2 auto (filter_bitvec)": dict(pats=mixed, k=2),
    }
    for what, kw in cases.items():
        off = outcome(codes, TABLE, bits=0, **kw)
        on = outcome(codes, TABLE, bits=8, **kw)
        assert off[:2] == on[:2], (what, off[:2], on[:2])
        assert LONG_PHRASE not in on[1], (what, on[1])
        assert off[2] == on[2], what
    refused = outcome(codes, TABLE, mixed, bits=8, kernel=sat_amd.KERNEL_SEED)   # asked for by name, the family refuses long primers as before
    assert refused[2] is None and refused == outcome(codes, TABLE, mixed, bits=0, kernel=sat_amd.KERNEL_SEED)
