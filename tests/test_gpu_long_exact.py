"""GPU: primers of 33..64 characters at k = 0 on the seed plan (bit 1 of pm_config.long_patterns, long_exact=True;
csrc/pm_seed.hip: wide tiles, the WIDE instances of pm_seed_scan, verify_exact_wide; csrc/pm_verify.h seed_verify<64>;
DESIGN.md 4.10).

pm_seed_scan keys on a primer's last bases (20, or as many as the list's shortest primer has), so a primer of up to 64
characters needs no pass of its own: it joins the plan's tiles, and a tile that holds one is verified on rows of 64
characters.  The route is a permission of the caller, off by default.  Here: a 33-, a 47- and a 64-mer against every
single-substitution variant of themselves, shared suffixes (bucket overflow, both scan forms), a mixed list through every
interface, the stream's edges, IUPAC letters, the routing rules, the final hits against the former route's, a wide tile
beside a narrow one, and the counts with their re-alignment on the device.  Expected values come from the oracle."""
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
from test_gpu_align_device import check_against_host
from test_gpu_exhaustive import TABLE, stream_of, substitution_variants

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASES = list("ACGT")
LONG_PHRASE = "of 33..64 characters"
# engines: (semantics asked for, semantics selected, the oracle's engine)
KT = (sat_amd.SEM_KEYWORD_TREE, sat_amd.SEM_KEYWORD_TREE, O.AUTO)
SA = (sat_amd.SEM_SHIFT_AND, sat_amd.SEM_SHIFT_AND, O.SHIFT_AND)
ENGINES = {"keyword_tree": KT, "shift_and": SA}


def rand_seq(rng, n):
    return "".join(rng.choice(BASES, size=n).tolist())


def engine(pats, sem=sat_amd.SEM_AUTO, k=0, bits=2, ids=None, **kw):
    """bits: pm_config.long_patterns (1 = the -K permission, 2 = the k = 0 one)"""
    pm = sat_amd.PatternMatch(k=k, semantics=sem, long_patterns=bool(bits & 1), long_exact=bool(bits & 2), **kw)
    for i, p in enumerate(pats):
        pm.add_pattern(p, ids[i] if ids else i + 1)
    return pm


def oracle_hits(codes, table, pats, eng=O.AUTO, ids=None, wildcards=False):
    return O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=eng, k=0, ids=ids, wildcards=wildcards))


def nlong(pats):
    """the primers of 33..64 characters the main class takes (A,C,G,T only; lists under -w are counted by hand)"""
    return sum(1 for p in pats if 33 <= len(p) <= 64 and set(p) <= set(BASES))


def nresidue(pats):
    return sum(1 for p in pats if len(p) > 64 or len(p) < 10 or not set(p) <= set(BASES))


def exact_route(pm, selected, n_long, residue=0, window=None, wide_tiles=None):
    """the handle runs n_long long primers on the seed plan, and the bit-parallel kernel `residue` primers"""
    d = pm.describe()
    assert pm.selected() == (selected, sat_amd.KERNEL_SEED), d
    assert d.startswith("kernel=pm_seed_scan ") and ("with %d patterns %s (wide rows, wide tiles=" % (n_long, LONG_PHRASE)) in d, d
    if residue:
        assert ("for %d patterns the seed plan does not take" % residue) in d, d
        assert d.index(LONG_PHRASE) < d.index("does not take"), d
    else:
        assert "does not take" not in d, d
    if window is not None:
        assert (" window=%d " % window) in d, d
    if wide_tiles is not None:
        assert ("wide tiles=%d)" % wide_tiles) in d, d
    return d


def run(pm, codes, table, chunk=1 << 26):
    pm.init(codes, table)
    return sat_amd.sorted_tuples(pm.find_all(chunk=chunk))


# ---- 1. near misses --------------------------------------------------------------------------------------------------
_NEAR = {}


def near_case(L):
    """the primer and all 3L texts one substitution away from it, each between end-of-sequence characters; the primer is
    primer 1 of a list with 1,500 random 20-mers and 200 long decoys"""
    if L not in _NEAR:
        rng = np.random.default_rng(4400 + L)
        p = rand_seq(rng, L)
        variants = sorted(substitution_variants(p, 0) | substitution_variants(p, 1))
        parts = stream_of(variants, rng)
        codes = synth.normalize(synth.stream(parts), TABLE)
        decoys = [rand_seq(rng, 20) for _ in range(1500)] + [rand_seq(rng, int(rng.integers(33, 65))) for _ in range(200)]
        _NEAR[L] = dict(p=p, nvar=len(variants), codes=codes, pats=[p] + decoys, want={})
    return _NEAR[L]


@pytest.mark.parametrize("name", list(ENGINES))
@pytest.mark.parametrize("L", [33, 47, 64])
def test_near_misses(L, name):
    c = near_case(L)
    assert c["nvar"] == 1 + 3 * L
    sem, selected, eng = ENGINES[name]
    want = oracle_hits(c["codes"], TABLE, c["pats"], eng)
    assert [pid for _, pid, _ in want].count(1) == 1                 # (the oracle: primer 1 hits its exact copy only)
    pm = engine(c["pats"], sem)
    try:
        got = run(pm, c["codes"], TABLE)
        d = exact_route(pm, selected, 201, window=20, wide_tiles=1)
    finally:
        pm.close()
    print("near misses L %d %s: %d hits (oracle %d) [%s]" % (L, name, len(got), len(want), d))
    assert got == want, (L, name, len(got), len(want))
    assert [h for h in got if h[1] == 1] == [h for h in want if h[1] == 1] and sum(1 for h in got if h[1] == 1) == 1


# ---- 2. shared suffixes ---------------------------------------------------------------------------------------------
_SUFFIX = {}


def occurrences(ents, p):
    """windows of the entries that equal p (a brute-force string search)"""
    return sum(1 for e in ents for a in range(len(e) - len(p) + 1) if e.startswith(p, a))


def suffix_case():
    """a 64-mer, its suffixes as primers of their own, copies of it that differ at one index, a duplicate under a second
    id, 40 long primers with one 20-base suffix (one key of the filter and of the bucket table: the probe sequence runs
    over five full buckets, probe_from) and every reverse complement; the stream holds each long primer once"""
    if not _SUFFIX:
        rng = np.random.default_rng(4470)
        other = lambda ch: BASES[(BASES.index(ch) + 1 + int(rng.integers(0, 3))) % 4]
        P = rand_seq(rng, 64)
        sub = lambda s, j: s[:j] + other(s[j]) + s[j + 1:]
        fam = [P] + [P[-n:] for n in (63, 40, 33, 32, 20)] + [sub(P, j) for j in (0, 31, 32, 43)]
        tail = rand_seq(rng, 20)
        shared = [rand_seq(rng, int(rng.integers(13, 45))) + tail for _ in range(40)]
        assert all(33 <= len(s) <= 64 for s in shared)
        fwd = fam + shared
        pats = fwd + [synth.revcomp(p) for p in fwd] + [P]           # the last one: P again, under another id
        planted = [p for p in fwd if len(p) > 32]
        ents = [rand_seq(rng, 40) + p + rand_seq(rng, 40) for p in planted] + [rand_seq(rng, 30) + synth.revcomp(P) + rand_seq(rng, 9)]
        ents += [rand_seq(rng, 3000)]
        codes = synth.normalize(synth.stream(ents), TABLE)
        _SUFFIX.update(pats=pats, twelve=P[-12:], codes=codes, ents=ents)
    return _SUFFIX


@pytest.mark.parametrize("name", list(ENGINES))
@pytest.mark.parametrize("twelve", [False, True], ids=["window20", "window12"])
def test_shared_suffixes(twelve, name):
    c = suffix_case()
    sem, selected, eng = ENGINES[name]
    pats = c["pats"] + ([c["twelve"]] if twelve else [])
    want = oracle_hits(c["codes"], TABLE, pats, eng)
    by = {}
    for e, pid, _ in want:
        by.setdefault(pid, []).append(e)
    # the oracle: P, its duplicate and every suffix of it hit wherever P or a copy that keeps them stands; a copy that
    # differs at one index hits its own plant alone; every planted long primer has a hit
    assert len(by[1]) == 1 and by[1] == by[len(c["pats"])]
    for j, idx in enumerate((0, 31, 32, 43)):                        # (their own plants; P's plant is none of them)
        assert by[7 + j] and not set(by[7 + j]) & set(by[1]), idx
    assert [len(by[i]) for i in (2, 3, 4, 5, 6)] == [3, 4, 5, 6, 8]   # suffixes of 63, 40, 33, 32, 20: P's plant and the copies that keep them
    for pid, p in enumerate(pats, 1):                                # every primer: as many hits as a string search finds
        assert len(by.get(pid, [])) == occurrences(c["ents"], p), (pid, p)
    assert all(pid in by for pid, p in enumerate(c["pats"][:51], 1) if len(p) > 32)
    pm = engine(pats, sem)
    try:
        got = run(pm, c["codes"], TABLE)
        exact_route(pm, selected, nlong(pats), window=12 if twelve else 20, wide_tiles=1)
    finally:
        pm.close()
    assert got == want, (twelve, name, len(got), len(want))


# ---- 3. a mixed list on text with repeats and N runs, through every interface ------------------------------------------
_MIXED = {}


def mixed_case():
    """exact copies of stream windows of 10..19, 20..32 and 33..64 characters, both strands, lengths 33, 63 and 64 among
    them, random primers beside them; `rest`: a primer with an N and a 70-mer, which stay residue"""
    if not _MIXED:
        rng = np.random.default_rng(4464)
        ents = synth.make_entries(rng, 3, 12000, n_runs=3, repeats=True, short=True)

        def cut(n, lo, hi):
            out = []
            while len(out) < n:
                e = ents[int(rng.integers(0, 3))]
                L = int(rng.integers(lo, hi + 1))
                a = int(rng.integers(0, len(e) - L))
                w = e[a:a + L]
                out.append(w if "N" not in w and rng.random() < 0.8 else rand_seq(rng, L))
            return out
        long_p = cut(60, 33, 64)
        for i, L in enumerate((33, 63, 64, 47)):
            a = 700 + 300 * i
            long_p[4 + i] = ents[i % 3][a:a + L].replace("N", "A")
        long_p[1], long_p[3] = long_p[0], synth.revcomp(long_p[0])
        short_p = cut(30, 10, 19)
        short_p[0] = ents[0][1000:1010].replace("N", "A")             # (a 10-mer: the window of the whole list)
        pats = short_p + cut(60, 20, 32) + long_p
        allp = pats + [synth.revcomp(p) for p in pats]
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
        c["want"][(name, rest)] = oracle_hits(c["codes"], c["table"], mixed_pats(rest), ENGINES[name][2])
    return c["want"][(name, rest)]


def check_mixed_route(pm, name, rest=True):
    return exact_route(pm, ENGINES[name][1], 120, residue=2 if rest else 0, window=10)


def test_mixed_list_condition():
    """the oracle reports hits of every class and of the residue, of primers of 33, 63 and 64 characters, and the same
    hits under both engines"""
    pats = mixed_pats()
    want = mixed_want("keyword_tree")
    for lo, hi in ((10, 19), (20, 32), (33, 64), (70, 70)):
        assert any(lo <= len(pats[pid - 1]) <= hi for _, pid, _ in want), (lo, hi)
    assert {len(pats[pid - 1]) for _, pid, _ in want} >= {33, 63, 64}
    assert len({pid for _, pid, _ in want if 33 <= len(pats[pid - 1]) <= 64}) >= 40
    assert want == mixed_want("shift_and")


@pytest.mark.parametrize("name", list(ENGINES))
@pytest.mark.parametrize("chunk", [1 << 26, 5000, 193])
def test_mixed_list_find_all(name, chunk):
    c = mixed_case()
    want = mixed_want(name)
    pm = engine(mixed_pats(), ENGINES[name][0])
    try:
        got = run(pm, c["codes"], c["table"], chunk)
        check_mixed_route(pm, name)
    finally:
        pm.close()
    assert got == want, (name, chunk, len(got), len(want))


@pytest.mark.parametrize("name", list(ENGINES))
def test_mixed_list_device_stages(name):
    """scan_candidates + finalize_device (the records are the hits): in one range, in two ranges and position-sharded"""
    c = mixed_case()
    want = mixed_want(name, rest=False)
    n = c["codes"].size
    pm = engine(mixed_pats(rest=False), ENGINES[name][0])
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
        cut, guard, parts = n // 3 + 5, 400, []                      # position shards with guard margins
        for own_lo, own_hi in ((0, cut), (cut, n)):
            g_lo, g_hi = max(0, own_lo - guard), min(n, own_hi + guard)
            pm.reset()
            pm.scan_candidates(g_lo, g_hi, to_host=False)
            parts += sat_amd.sorted_tuples(pm.finalize_device(0, sort=True, owned=(own_lo, own_hi, g_lo, None if g_hi == n else g_hi)))
        assert sorted(parts) == want
    finally:
        pm.close()


def min_window(pats):
    pm = engine(pats)
    pm.init(np.zeros(64, dtype=np.uint8), TABLE, window=1)
    w = pm.residency()["window"]
    pm.close()
    return w


@pytest.mark.parametrize("packed,windowed", [(False, True), (True, False), (True, True)])
def test_mixed_list_windowed_and_packed(packed, windowed):
    c = mixed_case()
    want = mixed_want("keyword_tree")
    n = c["codes"].size
    window = min_window(mixed_pats()) if windowed else None
    pm = engine(mixed_pats())
    try:
        if packed:
            bits = max(1, (len(c["table"]) - 1).bit_length())
            pm.init_packed(sat_amd.pack_codes(c["codes"], bits), bits, n, c["table"], window=window)
        else:
            pm.init(c["codes"], c["table"], window=window)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=700 if windowed else 1 << 26))
        check_mixed_route(pm, "keyword_tree")
        res = pm.residency()
    finally:
        pm.close()
    if windowed:
        assert res["window"] > 0 and res["loads"] > 1, res
    if packed:
        assert res["bits"] > 0, res
    assert got == want, (packed, windowed, len(got), len(want))


# ---- 4. the stream's edges ------------------------------------------------------------------------------------------
def edges_case():
    """long primers at the stream's first and last byte, one byte too long for the stream at either end, across an
    end-of-sequence character that lies at index 40 of the window, and over a text N at index 50"""
    rng = np.random.default_rng(4471)
    e0, e1, e2 = rand_seq(rng, 150), rand_seq(rng, 90), rand_seq(rng, 130)
    e1 = e1[:60] + "N" + e1[61:]
    raw = (e0 + "\n" + e1 + "\n" + e2).encode()                      # the stream starts and ends with a base
    table = b"ACGTN\n"
    codes = synth.normalize(raw, table)
    pats = []
    for L in (33, 40, 64):
        pats += [e0[:L], "A" + e0[:L - 1], e2[-L:], e2[-(L - 1):] + "A"]   # first byte; one too long in front; last byte; one too long behind
    pats += [e0[-40:] + "A" + e1[:23], e1[:40], e1[-29:] + "A" + e2[:10]]   # EOS at index 40 and at index 29 (code 0 = A in the primer); right behind an EOS
    pats += [e1[10:60] + "A" + e1[61:74], e1[10:60] + "N" + e1[61:74]]   # a text N at index 50: A,C,G,T primer, and one with an N (residue)
    pats += [e1[0:60], e1[61:]]                                      # up to the N and from behind it
    pats += [rand_seq(rng, 22) for _ in range(5)] + [e1[10:32], e0[5:23]]
    return dict(codes=codes, table=table, pats=pats, nohit=[2, 4, 6, 8, 10, 12, 13, 15, 16], hit=[1, 3, 5, 7, 9, 11, 14, 18, 19])


@pytest.mark.parametrize("name", list(ENGINES))
def test_stream_edges(name):
    c = edges_case()
    codes, table, pats, n = c["codes"], c["table"], c["pats"], c["codes"].size
    sem, selected, eng = ENGINES[name]
    want = oracle_hits(codes, table, pats, eng)
    pids = {pid for _, pid, _ in want}
    assert not pids & set(c["nohit"]) and pids >= set(c["hit"]), (sorted(pids), c["nohit"], c["hit"])
    for chunk in (1 << 26, 37, 3):
        pm = engine(pats, sem)
        try:
            got = run(pm, codes, table, chunk)
            assert (nlong(pats), nresidue(pats)) == (17, 1)
            exact_route(pm, selected, 17, residue=1, window=18)
            pm.reset()                                               # ranges of a few positions at both ends, through the candidate stage
            for b, e in ((0, 3), (3, 70), (n - 66, n - 2), (n - 2, n)):
                r = pm.scan_candidates(b, e)
                assert all(b < x <= e for x in r["end"].tolist()), (b, e, r["end"].tolist())
        finally:
            pm.close()
        assert got == want, (name, chunk, got, want)


@pytest.mark.parametrize("nbytes", [20, 33, 63, 64, 65])
def test_tiny_streams(nbytes):
    """streams of 20, 33, 63, 64 and 65 bytes against a list with a 64-mer, a 33-mer and a 20-mer cut from them"""
    rng = np.random.default_rng(4480 + nbytes)
    p = rand_seq(rng, 64)
    raw = {20: p[:20], 33: p[:33], 63: p[1:], 64: p, 65: "G" + p}[nbytes]
    assert len(raw) == nbytes
    pats = [p, p[:33], p[:20], p[31:], rand_seq(rng, 40), p[:30] + rand_seq(rng, 34), rand_seq(rng, 21)]
    codes = synth.normalize(raw.encode(), TABLE)
    for name, (sem, selected, eng) in ENGINES.items():
        want = oracle_hits(codes, TABLE, pats, eng)
        pm = engine(pats, sem)
        try:
            got = run(pm, codes, TABLE)
            exact_route(pm, selected, 5, window=20)
        finally:
            pm.close()
        assert got == want, (nbytes, name, got, want)
        assert ((nbytes, 1, 0) in want) == (nbytes >= 64)             # the 64-mer ends at the stream's last byte, or does not fit
        assert any(pid == 3 for _, pid, _ in want) == (nbytes != 63)


def test_long_primer_at_the_start_of_a_scan_chunk(monkeypatch):
    """PM_SEED_CHUNK at the smallest value the knob takes (16 waves x 1,024 positions): 64-mers that end at the first
    positions of the second and third chunk, so that the exact stage reads 63 bytes of the chunk in front"""
    chunk = 16 * 1024
    rng = np.random.default_rng(4490)
    raw = rand_seq(rng, 3 * chunk + 500)
    ends = [chunk + d for d in (1, 2, 3, 20)] + [2 * chunk + d for d in (1, 17, 63, 64)]   # end = index behind the window's last base
    pats = [raw[e - 64:e] for e in ends] + [raw[e - 33:e] for e in ends[:2]] + [rand_seq(rng, 20) for _ in range(50)] + [rand_seq(rng, 50) for _ in range(20)]
    codes = synth.normalize(raw.encode(), TABLE)
    want = oracle_hits(codes, TABLE, pats)
    assert [(e, pid) for e, pid, _ in want if pid <= 8] == sorted((e, i + 1) for i, e in enumerate(ends))
    monkeypatch.setenv("PM_SEED_CHUNK", str(chunk))
    pm = engine(pats)
    try:
        got = run(pm, codes, TABLE)
        d = exact_route(pm, sat_amd.SEM_KEYWORD_TREE, 30, window=20)
        assert ("chunk=%d " % chunk) in d and "nchunks=4 " in d, d
    finally:
        pm.close()
    assert got == want


# ---- 5. IUPAC letters --------------------------------------------------------------------------------------------------
def iupac_case():
    """-w on a plain stream: 40-mers with one and two IUPAC letters (expanded into their variants, as in the main class)
    join the wide tiles; three three-fold letters are 27 variants, more than the 16 the expansion takes: residue"""
    rng = np.random.default_rng(4491)
    ents = synth.make_entries(rng, 2, 6000)
    codes = synth.normalize(synth.stream(ents), TABLE)

    def cut(L):
        e = ents[int(rng.integers(0, 2))]
        a = int(rng.integers(0, len(e) - L))
        return e[a:a + L]
    pats = [cut(40) for _ in range(40)] + [cut(int(rng.integers(20, 25))) for _ in range(40)]
    two = {"A": "R", "C": "Y", "G": "K", "T": "W"}
    three = {"A": "D", "C": "B", "G": "V", "T": "H"}
    many = []
    for i in range(0, 40, 3):
        p = list(pats[i])
        if i % 9 == 6:                                               # three letters with three bases each
            for j in (5, 20, 36):
                p[j] = three[p[j]]
            many.append(i)
        else:
            for j in (5, 36)[:1 + (i // 3) % 2]:                     # index 5, and index 36 beyond the first dword
                p[j] = two[p[j]]
        pats[i] = "".join(p)
    assert len(many) >= 4
    allp = pats + [synth.revcomp_iupac(q) for q in pats]
    return dict(codes=codes, table=TABLE, pats=allp, residue=2 * len(many), wildcards=True)


def test_iupac_letters_in_long_primers():
    c = iupac_case()
    codes, allp = c["codes"], c["pats"]
    want = oracle_hits(codes, TABLE, allp, O.SHIFT_AND, wildcards=True)
    amb = lambda pid: len(set(allp[pid - 1]) - set("ACGT"))
    assert {amb(pid) for _, pid, _ in want if len(allp[pid - 1]) == 40} == {0, 1, 2, 3}   # hits of 40-mers with no, one, two and three IUPAC letters
    for chunk in (1 << 26, 997):
        pm = engine(allp, wildcards=True)
        try:
            got = run(pm, codes, TABLE, chunk)
            exact_route(pm, sat_amd.SEM_SHIFT_AND, 80 - c["residue"], residue=c["residue"], window=20)
        finally:
            pm.close()
        assert got == want, (chunk, len(got), len(want))


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
    pm = sat_amd.PatternMatch(k=0, semantics=case["sem"], wildcards=case.get("wildcards", False), long_exact=True)
    for i, p in enumerate(case["pats"]):
        pm.add_pattern(p, i + 1)
    pm.init(np.load(case["codes"]), case["table"].encode("latin-1"))
    hits = sat_amd.sorted_tuples(pm.find_all())
    out.append({"selected": list(pm.selected()), "describe": pm.describe(), "hits": [list(h) for h in hits]})
    pm.close()
print("RESULT " + json.dumps(out))
""" % (ROOT, os.path.join(ROOT, "tests"))


def run_child(case, env):
    r = subprocess.run([sys.executable, "-c", CHILD, str(case)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def outcome(codes, table, pats, k=0, bits=2, sem=sat_amd.SEM_AUTO, zones=None, **kw):
    pm = sat_amd.PatternMatch(k=k, semantics=sem, long_patterns=bool(bits & 1), long_exact=bool(bits & 2), **kw)
    for i, p in enumerate(pats):
        z = zones[i] if zones else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    try:
        pm.init(codes, table)
        hits = sat_amd.sorted_tuples(pm.find_all())                  # (the description holds the launch geometry)
        return pm.selected(), pm.describe(), hits
    except sat_amd.PmError as e:
        return e.code, str(e), None
    finally:
        pm.close()


def routing_lists():
    rng = np.random.default_rng(4493)
    ents = synth.make_entries(rng, 2, 6000)
    codes = synth.normalize(synth.stream(ents), TABLE)

    def cut(n, lo, hi):
        out = []
        for _ in range(n):
            e = ents[int(rng.integers(0, 2))]
            L = int(rng.integers(lo, hi + 1))
            a = int(rng.integers(0, len(e) - L))
            out.append(e[a:a + L])
        return out
    mids, longs = cut(30, 20, 24), cut(10, 33, 64)
    return ents, codes, mids, longs


def test_permission_bits():
    """bits 0, 1, 2 and 3 of pm_config.long_patterns on one list, at k = 0 and at -K 2: each bit acts on its own option set"""
    ents, codes, mids, longs = routing_lists()
    mixed = mids + longs
    at0 = [outcome(codes, TABLE, mixed, k=0, bits=b) for b in range(4)]
    atK = [outcome(codes, TABLE, mixed, k=2, bits=b, indels=False) for b in range(4)]
    assert at0[0] == at0[1] and at0[2] == at0[3], [o[1] for o in at0]                 # bit 0 alone leaves k = 0 as without it
    assert atK[0] == atK[2] and atK[1] == atK[3], [o[1] for o in atK]                 # bit 1 alone leaves -K 2 as without it
    assert LONG_PHRASE not in at0[0][1] and "for 10 patterns the seed plan does not take" in at0[0][1], at0[0][1]
    assert ("with 10 patterns %s (wide rows, wide tiles=1)" % LONG_PHRASE) in at0[2][1] and "does not take" not in at0[2][1], at0[2][1]
    assert LONG_PHRASE not in atK[0][1] and "pm_pair_verify_wide" in atK[1][1] and "wide rows" not in atK[1][1], (atK[0][1], atK[1][1])
    assert at0[0][2] == at0[2][2] == oracle_hits(codes, TABLE, mixed)                 # the final hits are equal on the two routes
    assert atK[0][2] == atK[1][2]
    assert len({pid for _, pid, _ in at0[2][2] if pid > 30}) == 10


def test_routing():
    """lists and option sets the route does not apply to: selected() and describe() are those of the handle with no bit
    set, byte for byte"""
    ents, codes, mids, longs = routing_lists()
    mixed = mids + longs
    z6 = [(6, 0)] * len(mixed)
    three = lambda p: p[:5] + "B" + p[6:20] + "D" + p[21:36] + "H" + p[37:]
    cases = {
        "-K 1": dict(pats=mixed, k=1, indels=False),
        "-K 2": dict(pats=mixed, k=2, indels=False),
        "-k 1": dict(pats=mixed, k=1),
        "-k 2": dict(pats=mixed, k=2),
        "shift_and_inexact at k = 0": dict(pats=mixed, sem=sat_amd.SEM_SHIFT_AND_INEXACT),
        "filter_bitvec at k = 0": dict(pats=mixed, sem=sat_amd.SEM_FILTER_BITVEC),
        "exact_bases at k = 0": dict(pats=mixed, sem=sat_amd.SEM_EXACT_BASES, zones=z6),
        "exact_halves at k = 0": dict(pats=mixed, sem=sat_amd.SEM_EXACT_HALVES),
        "seed kernels on request": dict(pats=mixed, kernel=sat_amd.KERNEL_SEED),
        "bit-parallel kernels on request": dict(pats=mixed, kernel=sat_amd.KERNEL_BITPAR),
        "no long primer": dict(pats=mids),
        "the only long primer has 65 characters": dict(pats=mids + [ents[0][200:265]]),
        "every long primer has three IUPAC letters": dict(pats=mids + [three(p) for p in longs], wildcards=True),
        "IUPAC letters without -w": dict(pats=mids + [p[:7] + "R" + p[8:] for p in longs]),
    }
    for what, kw in cases.items():
        off = outcome(codes, TABLE, bits=0, **kw)
        on = outcome(codes, TABLE, bits=2, **kw)
        assert off[:2] == on[:2], (what, off[:2], on[:2])
        assert LONG_PHRASE not in on[1], (what, on[1])
        assert off[2] == on[2], what
    assert outcome(codes, TABLE, mixed, kernel=sat_amd.KERNEL_SEED)[2] is None         # asked for by name the seed family refuses long primers
    on = outcome(codes, TABLE, mixed + [ents[0][200:265]])           # 65 characters: residue beside the long route
    assert ("with 10 patterns " + LONG_PHRASE) in on[1] and "for 1 patterns the seed plan does not take" in on[1], on[1]
    raw = synth.stream(ents)                                         # a raw ASCII stream is one seed_build takes as well
    on = outcome(np.frombuffer(raw, dtype=np.uint8), None, mixed)
    assert ("with 10 patterns " + LONG_PHRASE) in on[1] and on[2] == outcome(np.frombuffer(raw, dtype=np.uint8), None, mixed, bits=0)[2], on[1]


OTHER_LISTS = {
    "near misses of a 33-mer": lambda: dict(near_case(33), table=TABLE),
    "near misses of a 64-mer": lambda: dict(near_case(64), table=TABLE),
    "shared suffixes": lambda: dict(suffix_case(), table=TABLE),
    "the mixed list": lambda: dict(codes=mixed_case()["codes"], table=mixed_case()["table"], pats=mixed_pats()),
    "the stream's edges": edges_case,
    "IUPAC letters": iupac_case,
}


@pytest.mark.parametrize("what", list(OTHER_LISTS))
def test_without_the_permission_every_list_keeps_its_former_route(what, tmp_path):
    """each list of the tests above, under keyword_tree and shift_and: without the permission the long primers are residue,
    as before; with the permission and PM_LONG_EXACT=off in a fresh process (the environment is read by pm_create)
    selected() and describe() are the same, byte for byte, and so are the final hits -- which are the long route's"""
    c = OTHER_LISTS[what]()
    wild = bool(c.get("wildcards"))
    table = c["table"]
    np.save(tmp_path / "codes.npy", c["codes"])
    cases, here = [], []
    for sem in ([sat_amd.SEM_AUTO] if wild else [sat_amd.SEM_KEYWORD_TREE, sat_amd.SEM_SHIFT_AND]):
        off = outcome(c["codes"], table, c["pats"], bits=0, sem=sem, wildcards=wild)
        on = outcome(c["codes"], table, c["pats"], bits=2, sem=sem, wildcards=wild)
        assert LONG_PHRASE not in off[1] and LONG_PHRASE in on[1] and off[2] is not None, (what, off[:2], on[:2])
        assert "pm_seed_scan" in off[1] and "does not take" in off[1], (what, off[1])
        assert off[2] == on[2], (what, sem, len(off[2]), len(on[2]))
        here.append(off)
        cases.append(dict(sem=sem, pats=c["pats"], wildcards=wild, codes=str(tmp_path / "codes.npy"), table=bytes(table).decode("latin-1")))
    case = tmp_path / "case.json"
    case.write_text(json.dumps({"cases": cases}))
    env = {x: v for x, v in os.environ.items() if x != "PM_LONG_EXACT"}
    for off, child in zip(here, run_child(case, dict(env, PM_LONG_EXACT="off"))):
        assert (tuple(child["selected"]), child["describe"]) == (off[0], off[1]), (what, child["describe"], off[1])
        assert [tuple(h) for h in child["hits"]] == off[2], what


# ---- 7. a wide tile beside a narrow one ------------------------------------------------------------------------------
def test_two_tiles(monkeypatch):
    """PM_SEED_TILE cuts the main class in two: the first tile holds primers of 10..32 characters only and is built and
    verified as ever, the second one holds the long primers"""
    c = mixed_case()
    pats = mixed_pats(rest=False)
    order = sorted(range(len(pats)), key=lambda i: (len(pats[i]) > 32, i))   # (ids stay: the list is added in this order)
    narrow = sum(1 for p in pats if len(p) <= 32)
    monkeypatch.setenv("PM_SEED_TILE", str(narrow))                  # two tiles of half the list each (init_common evens them out)
    per = (len(order) + 1) // 2
    assert per <= narrow and all(len(pats[i]) <= 32 for i in order[:per]) and sum(len(pats[i]) > 32 for i in order[per:]) == 120
    pm = sat_amd.PatternMatch(k=0, long_exact=True)
    for i in order:
        pm.add_pattern(pats[i], i + 1)
    try:
        got = run(pm, c["codes"], c["table"])
        d = exact_route(pm, sat_amd.SEM_KEYWORD_TREE, 120, window=10, wide_tiles=1)
        assert " tiles=2 " in d, d
    finally:
        pm.close()
    assert got == mixed_want("keyword_tree", rest=False)


# ---- 8. counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [0, 2])
def test_mixed_list_counts(M):
    """count_all: the count rule on the oracle's hits; no record goes to the host for its re-alignment, the 70-mer's and
    the long primers' included"""
    c = mixed_case()
    pats = mixed_pats()
    want = mixed_want("keyword_tree")
    wc, wcap, winfo = count_rule.tally(want, lambda i: 0, len(pats), 0, M)      # (exact_alignment: every hit at distance 0)
    pm = engine(pats)
    try:
        pm.init(c["codes"], c["table"])
        counts, capped, info = pm.count_all(max_count=M)
        check_mixed_route(pm, "keyword_tree")
    finally:
        pm.close()
    assert counts.tolist() == wc
    assert capped.tolist() == wcap
    for f in ("tallied", "skipped", "bogus"):
        assert info[f] == winfo[f], (f, info[f], winfo[f])
    assert info["aligned_host"] == 0, info
    assert sum(sum(row) for row, p in zip(wc, pats) if 33 <= len(p) <= 64) > 0


def test_realignment_of_long_primers_on_the_device():
    """align_hits_device_numpy(text=True) against align_hits / align_hits_text, field for field, on the final hits of the
    mixed list, and against the oracle's re-alignment: start = end - L, distance 0"""
    c = mixed_case()
    pats = mixed_pats()
    pm = engine(pats)
    try:
        pm.init(c["codes"], c["table"])
        final = pm.find_all()
        check_mixed_route(pm, "keyword_tree")
        assert sat_amd.sorted_tuples(final) == mixed_want("keyword_tree")
        pm.reset()
        al, ops, txt = pm.align_hits_device_numpy(final, text=True)
        _, _, info = pm.counts()
        assert info["aligned_host"] == 0 and info["aligned_device"] == final.size, info
        assert check_against_host(pm, final, al, ops, txt, "final hits") > 0
        text = O.Text(c["codes"], c["table"])
        long_seen = 0
        for i in range(final.size):
            p = pats[int(final["pid"][i]) - 1]
            _, st, en, ed, _ = O.cli_align(text, p, int(final["end"][i]), 0)
            assert (int(al["start"][i]), int(al["end"][i]), int(al["editdist"][i])) == (st, en, ed), (final[i], al[i], (st, en, ed))
            if 33 <= len(p) <= 64:
                long_seen += 1
                assert en - st == len(p) and ed == 0, (final[i], al[i], txt[i])
        assert long_seen >= 40
    finally:
        pm.close()
