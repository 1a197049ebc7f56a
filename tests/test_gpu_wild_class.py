"""GPU: -w primers with three or more ambiguity letters on pm_wild_sub_scan (csrc/pm_short.hip).

Whole-primer expansion stops at 16 concrete variants, so a primer with more went to the bit-parallel residue.  With
wild_class=True (the PM_WILD_CLASS bit of pm_config.long_patterns) such primers of 16..32 characters are a class of their
own: keys expanded per field pair of the last 16 characters, everything else compared by class.  Here: parity with the
oracle through the C ABI on mixed lists (k = 0 on shift_and, -K 1 / -K 2 on filter_bitvec; whole and in small ranges),
the bit off and the knob, every placement of up to two substitutions, the stream's edges and the handle forms, the caps and
the option sets the class does not apply to, a class-only list, exact zones, and the stages behind the scan.
Expected values come from the oracle."""
import itertools

import numpy as np
import pytest

import count_rule
import sat_amd
import synth
from oracle import pmoracle as O

pytestmark = pytest.mark.gpu

TABLE = b"ACGT\n"
TABLE_N = b"ACGT\nN"
BASES = "ACGT"
LETTERS = "RYKMSWBDHVN"
CLASS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "K": "GT", "M": "AC", "S": "CG", "W": "AT",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
# option sets: (name, k, indels, semantics asked for, the oracle's engine)
OPTS = {"k0": (0, True, sat_amd.SEM_SHIFT_AND, 4), "K1": (1, False, sat_amd.SEM_FILTER_BITVEC, 5), "K2": (2, False, sat_amd.SEM_FILTER_BITVEC, 5)}


def rand_seq(rng, n):
    return "".join(rng.choice(list(BASES), size=n).tolist())


def variants(p):
    n = 1
    for ch in p:
        n *= len(CLASS[ch])
    return n


def pair_keys(p, fa, fb):
    t = p[-16:]
    n = 1
    for ch in t[4 * fa:4 * fa + 4] + t[4 * fb:4 * fb + 4]:
        n *= len(CLASS[ch])
    return n


def in_class(p, k, stream_has_n):
    """the routing rule restated: 16..32 characters, more than 16 concrete variants, at most 256 keys in every field pair
    of the plan, and under filter_bitvec no N primer on a stream with N"""
    pairs = list(itertools.combinations(range(4), 2)) if k == 2 else [(0, 1), (2, 3)]
    if not 16 <= len(p) <= 32 or variants(p) <= 16 or any(pair_keys(p, a, b) > 256 for a, b in pairs):
        return False
    return not (k > 0 and "N" in p and stream_has_n)


def add_letters(rng, p, n, alphabet=LETTERS):
    """n ambiguity letters at distinct places, each one a letter whose class holds the base it replaces"""
    p = list(p)
    for i in rng.choice(len(p), size=n, replace=False).tolist():
        p[i] = str(rng.choice([c for c in alphabet if p[i] in CLASS[c]]))
    return "".join(p)


def engine(pats, name, wild_class=True, zones=None, **kw):
    k, indels, sem, _ = OPTS[name]
    args = dict(k=k, indels=indels, semantics=sem, wildcards=True, wild_class=wild_class)
    args.update(kw)
    pm = sat_amd.PatternMatch(**args)
    for i, p in enumerate(pats):
        z = zones[i] if zones else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    return pm


def oracle_hits(codes, table, pats, name, zones=None, **kw):
    k, indels, _, eng = OPTS[name]
    args = dict(engine=eng, k=k, indels=indels, wildcards=True, text_n=False)
    args.update(kw)
    if zones:
        args.update(esb=[z[0] for z in zones], eeb=[z[1] for z in zones])
    return O.sorted_tuples(O.find_all(O.Text(codes, table), pats, **args))


def run(pats, name, codes, table, chunk=1 << 26, **kw):
    pm = engine(pats, name, **kw)
    try:
        pm.init(codes, table)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        return pm.selected(), pm.describe(), got                      # (the description holds the last scan's geometry)
    finally:
        pm.close()


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
_PARITY = {}
# generator seeds for which the oracle's output meets test_parity_condition (chosen on the CPU, with the oracle)
PARITY_SEEDS = [4127, 4463, 4468, 4843, 4854, 4938]


def parity_case(seed):
    """3 entries of 1,500..4,000 bases (odd seeds: with N runs), 300 primers of one length (16, 19, 20, 24, 32 in turn), every
    sixth with 3..6 ambiguity letters, every ninth with one or two, both strands; the oracle's hits per option set"""
    if seed not in _PARITY:
        rng = np.random.default_rng(PARITY_SEEDS[seed])
        ents = synth.make_entries(rng, 3, int(rng.integers(1500, 4000)), n_runs=3 if seed % 2 else 0)
        L = [16, 19, 20, 24, 32][seed % 5]
        pats = synth.make_patterns(rng, ents, 300, length=L, planted=0.9, extras=False)
        for i in range(len(pats)):
            if i % 6 == 0:
                pats[i] = add_letters(rng, pats[i], 3 + (i // 6) % 4)
            elif i % 9 == 0:
                pats[i] = add_letters(rng, pats[i], 1 + (i // 9) % 2)
        allp = pats + [synth.revcomp_iupac(p) for p in pats]
        table = synth.table_for(ents)
        _PARITY[seed] = dict(ents=ents, pats=allp, table=table, codes=synth.normalize(synth.stream(ents), table), want={}, L=L,
                             has_n=b"N" in table)
    return _PARITY[seed]


def parity_want(seed, name):
    c = parity_case(seed)
    if name not in c["want"]:
        c["want"][name] = oracle_hits(c["codes"], c["table"], c["pats"], name)
    return c["want"][name]


def class_counts(c, name):
    k = OPTS[name][0]
    members = [in_class(p, k, c["has_n"]) for p in c["pats"]]
    quirk = lambda p: k > 0 and "N" in p and c["has_n"]            # (filter_bitvec: an N primer on an N stream needs the text-based verify)
    rest = sum(1 for p, m in zip(c["pats"], members) if not m and (variants(p) > 16 or quirk(p)))
    return members, sum(members), rest


def check_route(c, name, selected, d):
    _, nclass, nrest = class_counts(c, name)
    assert selected[1] == sat_amd.KERNEL_SEED, d
    assert "pm_wild_sub_scan for %d patterns with more than 16 concrete variants" % nclass in d, (nclass, d)
    if nrest:
        assert "for %d patterns the seed plan does not take" % nrest in d, (nrest, d)
    else:
        assert "does not take" not in d, d


@pytest.mark.parametrize("name", list(OPTS))
@pytest.mark.parametrize("seed", range(6))
def test_parity_condition(seed, name):
    """the inputs: the oracle reports at least 20 hits of class primers per option set, at least 5 at each distance 0..K"""
    c = parity_case(seed)
    members, nclass, _ = class_counts(c, name)
    assert nclass >= 40, nclass
    own = [dist for _, pid, dist in parity_want(seed, name) if members[pid - 1]]
    assert len(own) >= 20, len(own)
    for dist in range(OPTS[name][0] + 1):
        assert own.count(dist) >= 5, (dist, own.count(dist))


@pytest.mark.parametrize("name", list(OPTS))
@pytest.mark.parametrize("seed", range(6))
def test_parity(seed, name):
    c = parity_case(seed)
    want = parity_want(seed, name)
    for chunk in (1 << 26, 997, 193):
        selected, d, got = run(c["pats"], name, c["codes"], c["table"], chunk=chunk)
        check_route(c, name, selected, d)
        assert got == want, (seed, name, chunk, len(got), len(want))


# ---- 2. the bit off ----------------------------------------------------------------------------------------------------
# describe() of the six parity lists on the commit before the class existed, after one whole scan: (list, option set) -> text
PARENT_DESCRIBE = {
    (0, "K1"): "kernel=pm_seed_scan tiles=1 combos=2 pieces=1-of-2 x 8 bases window=16 slots=4096 chunk=524288 nchunks=1 grid=2 block=1024 lds=161808 + pm_bitpar_scan<1,false> for 86 patterns the seed plan does not take",
    (0, "K2"): "kernel=pm_seed_scan tiles=1 combos=6 pieces=2-of-4 x 4 bases window=16 slots=4096 chunk=524288 nchunks=1 grid=6 block=1024 lds=161808 + pm_bitpar_scan<2,false> for 86 patterns the seed plan does not take",
    (0, "k0"): "kernel=pm_seed_scan tiles=1 combos=1 pieces=1-of-1 x 16 bases window=16 slots=4096 chunk=524288 nchunks=1 grid=1 block=1024 lds=161808 + pm_bitpar_scan<0,false> for 86 patterns the seed plan does not take",
    (1, "K1"): "kernel=pm_seed_scan tiles=1 combos=2 pieces=1-of-2 x 9 bases window=19 slots=2048 chunk=524288 nchunks=1 grid=2 block=1024 lds=161808 + pm_bitpar_scan<1,false> for 106 patterns the seed plan does not take",
    (1, "K2"): "kernel=pm_seed_scan tiles=1 combos=6 pieces=2-of-4 x 4 bases window=19 slots=2048 chunk=524288 nchunks=1 grid=6 block=1024 lds=161808 + pm_bitpar_scan<2,false> for 106 patterns the seed plan does not take",
    (1, "k0"): "kernel=pm_seed_scan tiles=1 combos=1 pieces=1-of-1 x 16 bases window=19 slots=4096 chunk=524288 nchunks=1 grid=1 block=1024 lds=161808 + pm_bitpar_scan<0,false> for 92 patterns the seed plan does not take",
    (2, "K1"): "kernel=pm_pair_scan tiles=1 combos=2 fields=2-of-4 x 5 bases window=20 row_slots=12 chunk=524288 nchunks=1 grid=2 block=1024 lds=163840 schedule=superchunk + pm_bitpar_scan<1,false> for 88 patterns the seed plan does not take",
    (2, "K2"): "kernel=pm_pair_scan tiles=1 combos=6 fields=2-of-4 x 5 bases window=20 row_slots=12 chunk=524288 nchunks=1 grid=6 block=1024 lds=163840 schedule=superchunk + pm_bitpar_scan<2,false> for 88 patterns the seed plan does not take",
    (2, "k0"): "kernel=pm_seed_scan tiles=1 combos=1 pieces=4-of-4 x 4 bases window=20 slots=4096 chunk=524288 nchunks=1 grid=1 block=1024 lds=161808 + pm_bitpar_scan<0,false> for 88 patterns the seed plan does not take",
    (3, "K1"): "kernel=pm_pair_scan tiles=1 combos=2 fields=2-of-4 x 5 bases window=20 row_slots=12 chunk=524288 nchunks=1 grid=2 block=1024 lds=163840 schedule=superchunk + pm_bitpar_scan<1,false> for 112 patterns the seed plan does not take",
    (3, "K2"): "kernel=pm_pair_scan tiles=1 combos=6 fields=2-of-4 x 5 bases window=20 row_slots=12 chunk=524288 nchunks=1 grid=6 block=1024 lds=163840 schedule=superchunk + pm_bitpar_scan<2,false> for 112 patterns the seed plan does not take",
    (3, "k0"): "kernel=pm_seed_scan tiles=1 combos=1 pieces=4-of-4 x 4 bases window=20 slots=4096 chunk=524288 nchunks=1 grid=1 block=1024 lds=161808 + pm_bitpar_scan<0,false> for 98 patterns the seed plan does not take",
    (4, "K1"): "kernel=pm_pair_scan tiles=1 combos=2 fields=2-of-4 x 5 bases window=20 row_slots=12 chunk=524288 nchunks=1 grid=2 block=1024 lds=163840 schedule=superchunk + pm_bitpar_scan<1,false> for 90 patterns the seed plan does not take",
    (4, "K2"): "kernel=pm_pair_scan tiles=1 combos=6 fields=2-of-4 x 5 bases window=20 row_slots=12 chunk=524288 nchunks=1 grid=6 block=1024 lds=163840 schedule=superchunk + pm_bitpar_scan<2,false> for 90 patterns the seed plan does not take",
    (4, "k0"): "kernel=pm_seed_scan tiles=1 combos=1 pieces=4-of-4 x 4 bases window=20 slots=4096 chunk=524288 nchunks=1 grid=1 block=1024 lds=161808 + pm_bitpar_scan<0,false> for 90 patterns the seed plan does not take",
    (5, "K1"): "kernel=pm_seed_scan tiles=1 combos=2 pieces=1-of-2 x 8 bases window=16 slots=2048 chunk=524288 nchunks=1 grid=2 block=1024 lds=161808 + pm_bitpar_scan<1,false> for 106 patterns the seed plan does not take",
    (5, "K2"): "kernel=pm_seed_scan tiles=1 combos=6 pieces=2-of-4 x 4 bases window=16 slots=2048 chunk=524288 nchunks=1 grid=6 block=1024 lds=161808 + pm_bitpar_scan<2,false> for 106 patterns the seed plan does not take",
    (5, "k0"): "kernel=pm_seed_scan tiles=1 combos=1 pieces=1-of-1 x 16 bases window=16 slots=4096 chunk=524288 nchunks=1 grid=1 block=1024 lds=161808 + pm_bitpar_scan<0,false> for 96 patterns the seed plan does not take",
}


@pytest.mark.parametrize("name", list(OPTS))
@pytest.mark.parametrize("seed", range(6))
def test_bit_off_is_the_parents_handle(seed, name, monkeypatch):
    """every parity list (Bloom and pair plan in the main class, streams with and without N) with the bit clear, and with the
    bit set and PM_WILD_CLASS=off: the parent's describe() text for that list, and the oracle's hits"""
    c = parity_case(seed)
    want = parity_want(seed, name)
    monkeypatch.delenv("PM_WILD_CLASS", raising=False)
    selected, d, got = run(c["pats"], name, c["codes"], c["table"], wild_class=False)
    assert d == PARENT_DESCRIBE[seed, name] and got == want, d
    monkeypatch.setenv("PM_WILD_CLASS", "off")
    selected, d, got = run(c["pats"], name, c["codes"], c["table"], wild_class=True)
    assert d == PARENT_DESCRIBE[seed, name] and got == want, d
    monkeypatch.delenv("PM_WILD_CLASS")
    selected, d, got = run(c["pats"], name, c["codes"], c["table"], wild_class=True)
    assert "pm_wild_sub_scan" in d and got == want, d


def test_parent_texts_cover_both_plans():
    assert sum("pm_pair_scan" in t for t in PARENT_DESCRIBE.values()) >= 4 and sum("pm_seed_scan" in t for t in PARENT_DESCRIBE.values()) >= 6


# ---- 3. every placement ------------------------------------------------------------------------------------------------
_PLACE = {}


def placement_case():
    """a 16-, a 20- and a 32-mer with one ambiguity letter in each field of the tail; per primer and placement of <= 2
    substitutions to a base outside the class at that position one text on a random concrete variant, and 500 texts with
    three such substitutions; texts are entries of their own"""
    if not _PLACE:
        rng = np.random.default_rng(4200)
        prim, texts, far, subs, owner = [], [], [], [], []
        for L, four in ((16, "RYKN"), (20, "BDMS"), (32, "WHVN")):
            p = list(rand_seq(rng, L))
            for f, letter in enumerate(four):
                p[L - 16 + 4 * f + int(rng.integers(0, 4))] = letter
            prim.append("".join(p))

        def text_of(p, where):
            t = [str(rng.choice(list(CLASS[ch]))) for ch in p]
            for i in where:
                t[i] = str(rng.choice([b for b in BASES if b not in CLASS[p[i]]]))
            return "".join(t)

        for p in prim:
            free = [i for i, ch in enumerate(p) if ch != "N"]        # (no base lies outside the class of N)
            for r in (0, 1, 2):
                for where in itertools.combinations(free, r):
                    texts.append(text_of(p, where))
                    subs.append(r)
        for _ in range(500):
            o = int(rng.integers(0, 3))
            p = prim[o]
            free = [i for i, ch in enumerate(p) if ch != "N"]
            far.append(text_of(p, rng.choice(free, size=3, replace=False).tolist()))
            owner.append(o + 1)
        decoys = [rand_seq(rng, int(rng.integers(18, 29))) for _ in range(200)]
        ents = texts + far
        bounds, at = [], 1                                            # (first base, end of the last base] of every entry in the stream
        for e in ents:
            bounds.append((at, at + len(e)))
            at += len(e) + 1
        _PLACE.update(pats=prim + decoys, ntexts=len(texts), nfar=len(far), codes=synth.normalize(synth.stream(ents), TABLE), ents=ents,
                      subs=subs, owner=owner, far_bounds=bounds[len(texts):])
    return _PLACE


@pytest.mark.parametrize("name", ["K2", "K1", "k0"])
def test_every_placement(name):
    c = placement_case()
    want = oracle_hits(c["codes"], TABLE, c["pats"], name)
    selected, d, got = run(c["pats"], name, c["codes"], TABLE)
    assert selected[1] == sat_amd.KERNEL_SEED and "pm_wild_sub_scan for 3 patterns" in d and "does not take" not in d, d
    assert got == want, (name, len(got), len(want))
    K = OPTS[name][0]
    own = [(end, pid) for end, pid, _ in got if pid <= 3]
    assert len(own) >= sum(1 for r in c["subs"] if r <= K), (name, len(own))   # a hit per text built within K substitutions, at least
    # no text with three substitutions holds a hit of its own primer (every hit is at distance <= K <= 2): each hit's end
    # is mapped to the text it lies in
    starts = np.array([a for a, _ in c["far_bounds"]])
    for end, pid in own:
        j = int(np.searchsorted(starts, end, side="right")) - 1
        if j >= 0:
            assert a_text_of_another_primer(c, j, end, pid), (name, end, pid, j)


def a_text_of_another_primer(c, j, end, pid):
    a, b = c["far_bounds"][j]
    return not (a < end <= b) or c["owner"][j] != pid


# ---- 4. edges ------------------------------------------------------------------------------------------------------------
def wild20(rng, t, with_n=True):
    """a class primer that matches the 20-mer t: four letters, one in each field of the tail"""
    p = list(t)
    for f, n in zip(range(4), rng.permutation(4).tolist()):
        i = len(t) - 16 + 4 * f + int(rng.integers(0, 4))
        p[i] = "N" if n == 0 and with_n else str(rng.choice([c for c in "BDHV" if t[i] in CLASS[c]]))
    return "".join(p)


@pytest.mark.parametrize("name", list(OPTS))
def test_tiny_streams_and_stream_ends(name):
    rng = np.random.default_rng(4300)
    t = rand_seq(rng, 20)
    p16 = wild20(rng, "ACGT" + t[:16])[4:]
    pats = [wild20(rng, t), p16, wild20(rng, rand_seq(rng, 20)), rand_seq(rng, 22), wild20(rng, t + "ACGTACGTACGT"[:12])[:32]]
    assert all(variants(p) > 16 for p in pats if set(p) - set(BASES))
    streams = [t[:15], t[:16], t[:17], "G" + t + rand_seq(rng, 10), t, t + "\n" + rand_seq(rng, 40) + t, "\n" + t]
    for raw in streams:
        codes = synth.normalize(raw.encode(), TABLE)
        want = oracle_hits(codes, TABLE, pats, name)
        for chunk in (1 << 26, 3):
            selected, d, got = run(pats, name, codes, TABLE, chunk=chunk)
            assert selected[1] == sat_amd.KERNEL_SEED and "pm_wild_sub_scan for 4 patterns" in d, d
            assert got == want, (name, raw, chunk, got, want)
    want = oracle_hits(synth.normalize(streams[5].encode(), TABLE), TABLE, pats, name)
    assert {pid for _, pid, _ in want} >= {1, 2}                     # a hit that starts at byte 0 and one that ends at the last byte


@pytest.mark.parametrize("name", list(OPTS))
def test_eos_and_n_inside_the_window(name):
    """an end-of-sequence character at every index of a 20-character window (never a hit), a text N at every index (a mismatch)"""
    rng = np.random.default_rng(4301)
    t = rand_seq(rng, 20)
    pats = [wild20(rng, t, with_n=False)] + [rand_seq(rng, 21) for _ in range(5)]   # (filter_bitvec keeps an N primer on an N stream in the residue)
    parts = []
    for i in range(20):
        parts += [rand_seq(rng, 7) + t[:i] + "\n" + t[i + 1:] + rand_seq(rng, 9), rand_seq(rng, 5) + t[:i] + "N" + t[i + 1:] + rand_seq(rng, 11)]
    raw = ("\n".join(parts) + "\n" + t).encode()
    codes = synth.normalize(raw, TABLE_N)
    want = oracle_hits(codes, TABLE_N, pats, name)
    k = OPTS[name][0]
    selected, d, got = run(pats, name, codes, TABLE_N)
    assert "pm_wild_sub_scan for 1 patterns" in d and "does not take" not in d, d
    assert got == want, (name, got, want)
    own = [x for x in want if x[1] == 1]
    assert len(own) == (1 if k == 0 else 21), own                    # the clean copy; under -K also the 20 with one N


@pytest.mark.parametrize("name", ["k0", "K2"])
def test_scan_ranges_and_handle_forms(name):
    """pm_scan in ranges of 1..5 positions across the hits, a windowed handle with a window smaller than the stream, a packed
    handle, and position shards with a hit on the seam"""
    c = parity_case(2)
    want = parity_want(2, name)
    n = c["codes"].size
    members, _, _ = class_counts(c, name)
    k = OPTS[name][0]
    pm = engine(c["pats"], name)
    try:
        pm.init(c["codes"], c["table"])
        got, pos, step = [], 0, 1
        while pos < n:                                                # ranges of 1, 2, .. 5, 1, .. positions
            e = min(n, pos + step)
            v = pm.scan_view(pos, e)
            got += list(zip(v["end"].tolist(), v["pid"].tolist(), v["k"].tolist()))
            pos, step = e, step % 5 + 1
        assert sorted(got) == want, (name, len(got), len(want))
        if name == "K2":                                             # shards: the seam right inside a class primer's hit
            seam = next(end for end, pid, _ in want if members[pid - 1] and end > 200) - 3
            parts, guard = [], 200
            for own_lo, own_hi in ((0, seam), (seam, n)):
                g_lo, g_hi = max(0, own_lo - guard), min(n, own_hi + guard)
                pm.reset()
                pm.scan_candidates(g_lo, g_hi, to_host=False)
                parts += sat_amd.sorted_tuples(pm.finalize_device(0, sort=True, owned=(own_lo, own_hi, g_lo, None if g_hi == n else g_hi)))
            assert sorted(parts) == want
    finally:
        pm.close()
    for packed in (False, True):
        pm = engine(c["pats"], name)
        try:
            if packed:
                bits = max(1, (len(c["table"]) - 1).bit_length())
                pm.init_packed(sat_amd.pack_codes(c["codes"], bits), bits, n, c["table"])
            else:
                pm.init(c["codes"], c["table"], window=1)               # (the smallest window the handle takes)
            check_route(c, name, pm.selected(), pm.describe())
            got = sat_amd.sorted_tuples(pm.find_all(chunk=1 << 26 if packed else 700))
            res = pm.residency()
        finally:
            pm.close()
        assert got == want, (name, packed, len(got), len(want))
        assert res["bits"] > 0 if packed else (0 < res["window"] < n and res["loads"] > 1), res


# ---- 5. caps and refusals ----------------------------------------------------------------------------------------------
def test_caps_and_refusals(monkeypatch):
    c = parity_case(0)
    rng = np.random.default_rng(4400)
    pats, codes, table = c["pats"], c["codes"], c["table"]
    members, nclass, nrest = class_counts(c, "K2")
    # five N's in one field pair: more than 256 keys, stays in the residue while its neighbours join the class
    five = list(c["ents"][0][100:120])
    for i in (4, 5, 6, 8, 9):
        five[i] = "N"
    five = "".join(five)
    assert not in_class(five, 2, False) and variants(five) > 16
    want = oracle_hits(codes, table, pats + [five], "K2")
    assert any(pid == len(pats) + 1 for _, pid, _ in want)
    selected, d, got = run(pats + [five], "K2", codes, table)
    assert "pm_wild_sub_scan for %d patterns" % nclass in d and "for %d patterns the seed plan does not take" % (nrest + 1) in d, d
    assert got == want

    def both(name, plist, codes=codes, table=table, **kw):
        """describe() and hits with the bit set, and with the knob off as well: (equal descriptions, text, hits)"""
        monkeypatch.delenv("PM_WILD_CLASS", raising=False)
        _, d_on, got_on = run(plist, name, codes, table, **kw)
        monkeypatch.setenv("PM_WILD_CLASS", "off")
        _, d_off, got_off = run(plist, name, codes, table, **kw)
        monkeypatch.delenv("PM_WILD_CLASS")
        assert got_on == got_off
        return d_on == d_off, d_on, got_on

    # more than 24,000 run entries in a field pair: 100 primers with 256 keys in every pair beside the list
    heavy = []
    for _ in range(100):
        p = list(rand_seq(rng, 20))
        for f in range(4):
            p[4 + 4 * f], p[4 + 4 * f + 2] = "N", "N"
        heavy.append("".join(p))
    same, d, got = both("K2", pats + heavy)
    assert same and "pm_wild_sub_scan" not in d, d
    assert got == oracle_hits(codes, table, pats + heavy, "K2")
    # option sets and lists the class does not apply to
    same, d, got = both("K2", pats, indels=True)                     # -k 2
    assert same and "pm_wild_sub_scan" not in d, d
    assert got == oracle_hits(codes, table, pats, "K2", indels=True)
    same, d, got = both("K2", pats, kernel=sat_amd.KERNEL_BITPAR)    # the bit-parallel kernels by name: a handle on them
    assert same and d.startswith("kernel=pm_bitpar_scan<2,false>"), d
    assert got == oracle_hits(codes, table, pats, "K2")
    # exact_halves with wildcards: a handle on the bit-parallel kernels.  Selector 14 on both sides: exact_halves over shift_and,
    # the form the reference picks under -w and the one whose half seeds honour the letters (select.cc:258-260; 11..13 look the
    # halves up in a keyword tree, letter by letter, and report fewer hits on this list: 167 against 211)
    same, d, got = both("K2", pats, semantics=14)
    assert same and d.startswith("kernel=pm_bitpar_scan"), d
    want_h = oracle_hits(codes, table, pats, "K2", engine=14)
    assert got == want_h, (len(got), len(want_h), sorted(set(got) - set(want_h))[:8], sorted(set(want_h) - set(got))[:8])
    for off in (False, True):                                        # the seed kernels by name refuse wildcards, as before: an error, no handle
        if off:
            monkeypatch.setenv("PM_WILD_CLASS", "off")
        with pytest.raises(sat_amd.PmError) as ei:
            run(pats, "K2", codes, table, kernel=sat_amd.KERNEL_SEED)
        assert ei.value.code == -2 and "seed engine: IUPAC wildcards run on the bit-parallel family" in str(ei.value), str(ei.value)
    monkeypatch.delenv("PM_WILD_CLASS")
    # a stream with an R in it; -W on a stream with N
    ents_r = c["ents"] + ["ACGTRACGT" + rand_seq(rng, 30)]
    table_r = synth.table_for(ents_r)
    codes_r = synth.normalize(synth.stream(ents_r), table_r)
    same, d, got = both("K2", pats, codes=codes_r, table=table_r)
    assert same and "pm_wild_sub_scan" not in d, d
    assert got == oracle_hits(codes_r, table_r, pats, "K2")
    cn = parity_case(1)
    same, d, got = both("K2", cn["pats"], codes=cn["codes"], table=cn["table"], text_n=True)
    assert same and "pm_wild_sub_scan" not in d, d
    assert got == oracle_hits(cn["codes"], cn["table"], cn["pats"], "K2", text_n=True)
    # an X primer (accepts no base) keeps the list on the route it had
    xp = add_letters(rng, rand_seq(rng, 24), 4)
    xp = xp[:3] + "X" + xp[4:]
    same, d, got = both("K2", pats + [xp])
    assert same, d
    assert got == oracle_hits(codes, table, pats + [xp], "K2")
    # an N primer on an N stream under filter_bitvec stays in the residue
    npr = add_letters(rng, cn["ents"][0][50:74].replace("N", "A"), 3, alphabet="BDHV")
    npr = npr[:10] + "N" + npr[11:]
    _, ncl, nre = class_counts(cn, "K2")
    extra = [npr]
    selected, d, got = run(cn["pats"] + extra, "K2", cn["codes"], cn["table"])
    assert "pm_wild_sub_scan for %d patterns" % ncl in d and "for %d patterns the seed plan does not take" % (nre + 1) in d, d
    assert got == oracle_hits(cn["codes"], cn["table"], cn["pats"] + extra, "K2")


# ---- 6. a class-only list ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k0", "K2"])
def test_class_only_list(name):
    c = parity_case(4)
    members, _, _ = class_counts(c, name)
    pats = [p for p, m in zip(c["pats"], members) if m][:40]
    assert len(pats) == 40
    want = oracle_hits(c["codes"], c["table"], pats, name)
    assert len(want) >= 10
    for chunk in (1 << 26, 193):
        selected, d, got = run(pats, name, c["codes"], c["table"], chunk=chunk)
        assert selected[1] == sat_amd.KERNEL_SEED and d.startswith("kernel=pm_wild_sub_scan+pm_wild_sub_verify for 40 patterns") and "does not take" not in d, d
        assert got == want, (name, chunk, len(got), len(want))


# ---- 7. zones ----------------------------------------------------------------------------------------------------------
def test_zones():
    """-5 / -3 style exact zones on class primers under -K 2 (a class-only list: beside other primers with letters a zoned
    list keeps the bit-parallel family, as before): a substitution inside a zone still chains and is never the hit"""
    rng = np.random.default_rng(4500)
    ents = synth.make_entries(rng, 2, 3000)
    codes = synth.normalize(synth.stream(ents), TABLE)
    pats, zones = [], []
    for i in range(60):
        e = ents[i % 2]
        a = int(rng.integers(0, len(e) - 24))
        t = e[a:a + 24]
        p = add_letters(rng, t, 4, alphabet="BDHVN")
        # a substitution at a place of its own: inside the 5' zone, inside the 3' zone, outside both, none
        where = [1, 22, 12, None][i % 4]
        if where is not None and p[where] in BASES:
            p = p[:where] + BASES[(BASES.index(p[where]) + 1) % 4] + p[where + 1:]
        pats.append(p)
        zones.append([(6, 0), (0, 6), (4, 4)][i % 3])
    pats = [p for p in pats if in_class(p, 2, False)]
    zones = zones[:len(pats)]
    want = oracle_hits(codes, TABLE, pats, "K2", zones=zones)
    plain = oracle_hits(codes, TABLE, pats, "K2")
    assert want != plain and len(want) >= 20                         # a violation changes the outcome somewhere, and hits remain
    selected, d, got = run(pats, "K2", codes, TABLE, zones=zones)
    assert d.startswith("kernel=pm_wild_sub_scan+pm_wild_sub_verify for %d patterns" % len(pats)), d
    assert got == want, (len(got), len(want))


# ---- 8. behind the scan --------------------------------------------------------------------------------------------------
def test_counts_and_device_alignment():
    c = parity_case(3)
    want = parity_want(3, "K2")
    members, _, _ = class_counts(c, "K2")
    text = O.Text(c["codes"], c["table"])
    eds = [O.cli_align(text, c["pats"][pid - 1], end, 2, False, wildcards=True)[3] for end, pid, _ in want]
    pm = engine(c["pats"], "K2")
    try:
        pm.init(c["codes"], c["table"])
        check_route(c, "K2", pm.selected(), pm.describe())
        for M in (0, 2):
            wc, wcap, winfo = count_rule.tally(want, lambda i: eds[i], len(c["pats"]), 2, M)
            pm.reset()
            counts, capped, info = pm.count_all(max_count=M)
            assert counts.tolist() == wc and capped.tolist() == wcap
            for f in ("tallied", "skipped", "bogus"):
                assert info[f] == winfo[f], (f, info[f], winfo[f])
        pm.reset()
        hits = pm.find_all()
        own = hits[np.array([members[pid - 1] for pid in hits["pid"].tolist()], dtype=bool)]
        assert own.size >= 20
        dev = pm.align_hits_device_numpy(own)
        host = pm.align_hits(own)
        for f in ("start", "end", "editdist", "value"):
            assert dev[f].tolist() == host[f].tolist(), f
    finally:
        pm.close()


def test_pcr_pair_round_over_degenerate_primers():
    """pm_pcr_scan + pm_pcr_pair over three pairs of class primers (both strands in the list, as pm_pcr_match adds them): the
    amplicons, their re-alignments and strings equal the host loop's (tests/pcr_rule.py) on the hits find_all reports"""
    import pcr_rule as R
    from test_gpu_pcr_pairs import STRIDE, check_round, realign

    class W:
        pass
    rng = np.random.default_rng(4600)
    ents = [rand_seq(rng, 2500), rand_seq(rng, 2500)]
    w = W()
    w.raw = synth.stream(ents)
    w.n = len(w.raw)
    w.starts = [1, 2 + len(ents[0])]
    s = w.raw.decode()
    sites = [(w.starts[0] + 300, w.starts[0] + 600), (w.starts[0] + 1500, w.starts[0] + 1850), (w.starts[1] + 700, w.starts[1] + 1000)]
    prim = []
    for a, b in sites:                                               # both primers as they stand on the stream (ids 2j - 1, 2j: tests/pcr_rule.py)
        prim += [wild20(rng, s[a:a + 20], with_n=False), wild20(rng, s[b:b + 20], with_n=False)]
    assert all(in_class(p, 2, False) for p in prim)
    pats = prim + [synth.revcomp_iupac(p) for p in prim]
    codes = synth.normalize(w.raw, TABLE)
    pm = engine(pats, "K2")
    try:
        pm.init(codes, TABLE)
        pm.pcr_setup(amplicon_max=420, entry_starts=w.starts)
        found = pm.find_all()
        d = pm.describe()
        assert d.startswith("kernel=pm_wild_sub_scan+pm_wild_sub_verify for 12 patterns"), d
        hits = sorted(zip(found["end"].tolist(), found["pid"].tolist(), found["k"].tolist()))
        assert len(hits) >= 6                                        # every site
        res = realign(pm, found, 2)
        rule = R.Rule(len(prim), [0] + [len(p) for p in pats], 2, False, False, False, 0, 420, -1, None)
        pm.reset()
        got = 0
        for begin in range(0, w.n, 1000):
            got += pm.pcr_scan(begin, min(w.n, begin + 1000))
        assert got == len(hits)
        want, carried = check_round(pm, w, rule, res, hits, w.n, False)
        assert carried == [] and {x[5] for x in want} >= {1, 2, 3}
    finally:
        pm.close()


def test_suspect_list_grows_and_the_range_is_scanned_again():
    """a homopolymer of 500,000 bases under a class primer whose last 16 characters accept it in every field pair and whose
    first eight do not: six suspects per window, 3 * 10^6 in all, against the 2^21 the suspect list holds at first (the
    range / 128 + 2^20 16-byte slots of wild_scan, two 8-byte suspects each).  The scan counts past the list's end without
    writing there, the list grows, the range is scanned again -- and the hits are the oracle's"""
    rng = np.random.default_rng(4700)
    p = "CCCCCCCC" + "ANAAADAAAVAAAHAA"
    assert in_class(p, 2, False)
    site = "CCCCCCCC" + "AGAAATAAACAAATAA"
    ents = [rand_seq(rng, 50) + site + rand_seq(rng, 50), "G" + "A" * 500000 + "G", rand_seq(rng, 30) + site[:5] + "G" + site[6:] + rand_seq(rng, 30)]
    codes = synth.normalize(synth.stream(ents), TABLE)
    want = oracle_hits(codes, TABLE, [p], "K2")
    assert len(want) >= 2
    pm = engine([p], "K2")
    try:
        pm.init(codes, TABLE)
        got = sat_amd.sorted_tuples(pm.find_all())
        st = pm.scan_stats()
        d = pm.describe()
    finally:
        pm.close()
    assert d.startswith("kernel=pm_wild_sub_scan+pm_wild_sub_verify for 1 patterns"), d
    assert st["internal_rescans"] >= 1 and st["between_stages"] > 1 << 21, st
    assert got == want, (got, want)
