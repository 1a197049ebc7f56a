"""GPU: degenerate -w primers of 33..64 characters on the wild class (pm_wild_sub_verify_wide, csrc/pm_short.hip).

With wild_class=True and wild_long=True (bits 5 and 7 of pm_config.long_patterns) a -w primer of 33..64 characters with
three or more ambiguity letters joins the class of pm_wild_sub_scan: its keys are its last 16 characters', the exact stage
reads rows of 64 class nibbles.  Here: parity with the oracle through the C ABI on seven kinds of list (k = 0 on shift_and
and keyword_tree, -K 1 / -K 2 on filter_bitvec; whole and in ranges of 997 and 193) on table-coded and raw ASCII streams
with and without N, the routing and the bit clear (describe() texts recorded from the commit before the bit existed:
tests/golden/wild_long_parent.txt, written by tests/golden/make_wild_long_parent.py), every placement of up to two
substitutions, the stream's edges and the handle forms, zones, the refusals, the stages behind the scan and the growth of
the suspect list.  Expected values come from the oracle."""
import hashlib
import itertools
import os

import numpy as np
import pytest

import count_rule
import sat_amd
import synth
from oracle import pmoracle as O
from test_gpu_wild_class import BASES, CLASS, LETTERS, OPTS, TABLE, TABLE_N, add_letters, oracle_hits, pair_keys, rand_seq, variants

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wild_long_parent.txt")
FLAGS = ("long_patterns", "long_exact", "long_edits", "long_halves", "long_align", "wild_class", "edit_pair", "wild_long")
NO_N = "RYKMSWBDHV"
LONG_TEXT = "of them of 33..64 characters: pm_wild_sub_verify_wide"
# the option sets of tests/test_gpu_wild_class.py and k = 0 under keyword_tree.  The oracle restates no keyword tree with
# wildcards; at k = 0 its records are shift_and's -- every occurrence by class -- so that is the expected value there.
ALL_OPTS = dict(OPTS, k0kt=(0, True, sat_amd.SEM_KEYWORD_TREE, 4))
ORACLE_NAME = {"k0": "k0", "k0kt": "k0", "K1": "K1", "K2": "K2"}


def engine(pats, name, bits=160, zones=None, **kw):
    k, indels, sem, _ = ALL_OPTS[name]
    args = dict(k=k, indels=indels, semantics=sem, wildcards=True)
    args.update({f: bool((bits >> i) & 1) for i, f in enumerate(FLAGS)})
    args.update(kw)
    pm = sat_amd.PatternMatch(**args)
    assert pm.long_patterns_bits == bits
    for i, p in enumerate(pats):
        z = zones[i] if zones else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    return pm


def run(pats, name, codes, table, chunk=1 << 26, **kw):
    pm = engine(pats, name, **kw)
    try:
        pm.init(codes, table)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        return pm.selected(), pm.describe(), got                      # (the description holds the last scan's geometry)
    finally:
        pm.close()


def in_class(p, k, stream_has_n, maxlen=64):
    """the routing rule restated: 16..64 characters, more than 16 concrete variants, at most 256 keys in every field pair
    of the plan (of the last 16 characters), and under filter_bitvec no N primer on a stream with N"""
    pairs = list(itertools.combinations(range(4), 2)) if k == 2 else [(0, 1), (2, 3)]
    if not 16 <= len(p) <= maxlen or variants(p) <= 16 or any(pair_keys(p, a, b) > 256 for a, b in pairs):
        return False
    return not (k > 0 and "N" in p and stream_has_n)


def degenerate(rng, window, nletters, nsub=0, alphabet=LETTERS):
    """a class primer cut from the text: `nsub` substitutions, then `nletters` ambiguity letters that accept what they replace"""
    for _ in range(200):
        p = add_letters(rng, synth.mutate(rng, window, nsub=nsub), nletters, alphabet=alphabet)
        if in_class(p, 2, False) and in_class(p, 1, False):
            return p
    raise AssertionError("no class primer from " + window)


# ---- the streams and the lists -------------------------------------------------------------------------------------------
_CASE = {}
STREAMS = ("table", "table_n", "ascii", "ascii_n")


def case():
    """Entries: two of uniform text and one tandem repeat (a unit of 37 bases, 14 copies); the same with N runs.  Lists (a)-(g)
    of the primers cut from them, mutated by 0..2 substitutions (the last list: primers of exactly 33 and 64)."""
    if _CASE:
        return _CASE
    rng = np.random.default_rng(7100)
    unit = rand_seq(rng, 37)
    ents = synth.make_entries(rng, 2, 2600) + [rand_seq(rng, 40) + unit * 14 + rand_seq(rng, 40)]
    with_n = [list(e) for e in ents]
    for e in with_n:
        for _ in range(4):
            a = int(rng.integers(0, len(e) - 8))
            for i in range(a, a + int(rng.integers(1, 6))):
                e[i] = "N"
    with_n = ["".join(e) for e in with_n]

    def cut(L, e=None):
        e = ents[int(rng.integers(0, 3)) if e is None else e]
        a = int(rng.integers(0, len(e) - L))
        return e[a:a + L]

    def longs(n, L, alphabet=LETTERS):
        out = []
        for i in range(n):
            Li = L if isinstance(L, int) else int(rng.integers(L[0], L[1] + 1))
            out.append(degenerate(rng, cut(Li, 2 if i % 5 == 4 else None), 3 + i % 3, nsub=i % 3, alphabet=alphabet if i % 2 else NO_N))
        return out

    ten = longs(10, 52)
    plain20 = [synth.mutate(rng, cut(20), nsub=i % 3) for i in range(200)]
    plain12 = [cut(12) for _ in range(60)]
    short_class = [degenerate(rng, cut(int(rng.integers(16, 33))), 3 + i % 3, nsub=i % 3) for i in range(10)]
    lists = {
        "a": ten,
        "b": ten + plain20,
        "c": ten + plain12,
        "d": ten + short_class + plain20[:40],
        "e": ten + [cut(70), cut(40)] + plain20[:40],
        "f": longs(12, (33, 64)),
        "g": longs(4, 33) + longs(4, 64) + plain20[:30],
    }
    for name in lists:
        lists[name] = lists[name] + [synth.revcomp_iupac(p) for p in lists[name]]
    _CASE["lists"] = lists
    _CASE["ents"] = ents
    raw, raw_n = synth.stream(ents), synth.stream(with_n)
    _CASE["streams"] = {
        "table": (synth.normalize(raw, TABLE), TABLE, False),
        "table_n": (synth.normalize(raw_n, TABLE_N), TABLE_N, True),
        "ascii": (np.frombuffer(raw, dtype=np.uint8), None, False),
        "ascii_n": (np.frombuffer(raw_n, dtype=np.uint8), None, True),
    }
    _CASE["want"] = {}
    return _CASE


def want_of(lst, name, stream):
    c = case()
    key = (lst, ORACLE_NAME[name], stream)
    if key not in c["want"]:
        codes, table, _ = c["streams"][stream]
        c["want"][key] = oracle_hits(codes, table, c["lists"][lst], ORACLE_NAME[name])
    return c["want"][key]


def counts(pats, name, has_n, bits=160):
    """(class primers, of them long, residue primers) the routing must give for this list"""
    k = ALL_OPTS[name][0]
    maxlen = 64 if bits & 128 else 32
    members = [bool(bits & 32) and in_class(p, k, has_n, maxlen) for p in pats]
    nlong = sum(1 for p, m in zip(pats, members) if m and len(p) > 32)
    longest = 32
    if (k == 0 and bits & 2) or (k > 0 and bits & 1):
        longest = 64
    rest = 0
    for p, m in zip(pats, members):
        if m:
            continue
        quirk = k > 0 and "N" in p and has_n
        if variants(p) > 16 or quirk or len(p) > longest:
            rest += 1
    return sum(members), nlong, rest


def check_route(pats, name, has_n, selected, d, bits=160):
    nclass, nlong, nrest = counts(pats, name, has_n, bits)
    assert selected[1] == sat_amd.KERNEL_SEED, d
    assert "for %d patterns with more than 16 concrete variants" % nclass in d, (nclass, d)
    assert ", %d %s" % (nlong, LONG_TEXT) in d, (nlong, d)
    if nrest:
        assert "for %d patterns the seed plan does not take" % nrest in d, (nrest, d)
    else:
        assert "does not take" not in d, d


# ---- 1. parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OPTS))
@pytest.mark.parametrize("lst", list("abcdefg"))
def test_parity_condition(lst, name):
    """the inputs: on the plain table-coded stream the oracle reports hits of the long class primers that were cut from it
    with at most k substitutions (a third of them each with 0, 1 and 2: at least 4, 6 and 8 primers of every list), and --
    under -K 2 -- hits at distance 1 and 2 among them"""
    c = case()
    pats = c["lists"][lst]
    k = OPTS[name][0]
    long_ids = {i + 1 for i, p in enumerate(pats) if len(p) > 32 and in_class(p, k, False)}
    own = [(pid, dist) for _, pid, dist in want_of(lst, name, "table") if pid in long_ids]
    assert len({pid for pid, _ in own}) >= (4, 6, 8)[k], (lst, name, len(own))
    if k == 2:
        assert {dist for _, dist in own} >= {0, 1, 2}


@pytest.mark.parametrize("name", list(ALL_OPTS))
@pytest.mark.parametrize("lst", list("abcdefg"))
def test_parity(lst, name):
    """every list under shift_and and keyword_tree at k = 0 and filter_bitvec at -K 1 / -K 2, on the four stream forms, whole
    and in pm_scan ranges of 997 and 193"""
    c = case()
    pats = c["lists"][lst]
    for stream in STREAMS:
        codes, table, has_n = c["streams"][stream]
        want = want_of(lst, name, stream)
        for chunk in (1 << 26, 997, 193):
            selected, d, got = run(pats, name, codes, table, chunk=chunk)
            check_route(pats, name, has_n, selected, d)
            assert name != "k0kt" or selected[0] == sat_amd.SEM_KEYWORD_TREE, selected
            assert got == want, (lst, name, stream, chunk, len(got), len(want))


@pytest.mark.parametrize("lst", ["b", "e", "f"])
def test_parity_with_the_long_tiles_beside_the_class(lst):
    """keyword_tree at k = 0 reports what the same handle reports without any bit; and every option set with bits 0 / 1 on
    as well (the plain 40-mer of list (e) is then a main-class primer, the class primers are where they were)"""
    c = case()
    pats = c["lists"][lst]
    codes, table, has_n = c["streams"]["table"]
    assert run(pats, "k0kt", codes, table, bits=0)[2] == run(pats, "k0kt", codes, table)[2] == want_of(lst, "k0kt", "table")
    for name in ALL_OPTS:
        for stream in ("table", "ascii_n"):
            codes, table, has_n = c["streams"][stream]
            for chunk in (1 << 26, 193):
                selected, d, got = run(pats, name, codes, table, chunk=chunk, bits=163)
                check_route(pats, name, has_n, selected, d, bits=163)
                assert got == want_of(lst, name, stream), (lst, name, stream, chunk)
    if lst == "e":
        codes, table, _ = c["streams"]["table"]
        _, d, _ = run(pats, "K2", codes, table, bits=163)
        assert "with 2 patterns of 33..64 characters (pm_pair_verify_wide" in d and "for 2 patterns the seed plan does not take" in d, d


# ---- 2. routing ----------------------------------------------------------------------------------------------------------
def digest(hits):
    return hashlib.sha256(repr(hits).encode()).hexdigest()[:16]


def golden():
    """key -> hits, digest, describe: one tab-separated line per handle"""
    gold = {}
    with open(GOLDEN) as f:
        for line in f:
            key, hits, dig, text = line.rstrip("\n").split("\t")
            gold[key] = {"hits": int(hits), "digest": dig, "describe": text}
    return gold


def golden_cases():
    """(key, list, option set, bits) of the handles whose describe() text the golden file records from the parent commit"""
    return [("%s/%s/%d" % (lst, name, bits), lst, name, bits) for lst in "abcdefg" for name in OPTS for bits in (32, 127)]


def test_the_class_holds_the_long_primers():
    """bits 5 and 7: describe() names the long primers in the class and no residue for them"""
    c = case()
    codes, table, _ = c["streams"]["table"]
    _, d, _ = run(c["lists"]["a"], "K2", codes, table)
    assert d.startswith("kernel=pm_wild_sub_scan+pm_wild_sub_verify for 20 patterns with more than 16 concrete variants") and (", 20 " + LONG_TEXT) in d and "does not take" not in d, d
    _, d, _ = run(c["lists"]["b"], "K2", codes, table)
    assert d.startswith("kernel=pm_pair_scan") and "+ pm_wild_sub_scan for 20 patterns" in d and (", 20 " + LONG_TEXT) in d and "does not take" not in d, d
    _, d, _ = run(c["lists"]["c"], "k0", codes, table)
    assert d.startswith("kernel=pm_seed_scan") and "+ pm_wild_sub_scan for 20 patterns" in d and (", 20 " + LONG_TEXT) in d and "does not take" not in d, d


@pytest.mark.parametrize("name", list(OPTS))
def test_bit_seven_clear_is_the_parents_handle(name, monkeypatch):
    """values 32 and 127, bit 7 without bit 5 (128 behaves as 0, 223 as 95), and PM_WILD_LONG=off with both bits: the text the
    parent commit's build gives for the same handle, and its hits"""
    gold = golden()
    c = case()
    codes, table, _ = c["streams"]["table"]
    monkeypatch.delenv("PM_WILD_LONG", raising=False)
    for key, lst, nm, bits in golden_cases():
        if nm != name:
            continue
        pats = c["lists"][lst]
        want = want_of(lst, name, "table")
        assert gold[key]["hits"] == len(want) and gold[key]["digest"] == digest(want), key
        _, d, got = run(pats, name, codes, table, bits=bits)
        assert d == gold[key]["describe"] and got == want, (key, d)
        assert LONG_TEXT not in d
    for lst in "abef":
        pats = c["lists"][lst]
        want = want_of(lst, name, "table")
        zero = run(pats, name, codes, table, bits=0)
        assert run(pats, name, codes, table, bits=128) == zero and zero[2] == want
        assert run(pats, name, codes, table, bits=223)[1:] == run(pats, name, codes, table, bits=95)[1:]
        monkeypatch.setenv("PM_WILD_LONG", "off")
        _, d, got = run(pats, name, codes, table, bits=160)
        assert d == gold["%s/%s/32" % (lst, name)]["describe"] and got == want, d
        _, d, got = run(pats, name, codes, table, bits=255)
        assert d == gold["%s/%s/127" % (lst, name)]["describe"] and got == want, d
        monkeypatch.delenv("PM_WILD_LONG")


def test_the_golden_texts_keep_the_long_primers_in_the_residue():
    gold = golden()
    assert sorted(gold) == sorted(key for key, _, _, _ in golden_cases())
    assert all("does not take" in g["describe"] or g["describe"].startswith("kernel=pm_bitpar_scan") for g in gold.values())
    assert gold["d/K2/32"]["describe"].count("pm_wild_sub_scan for 20 patterns") == 1      # (the class of 16..32 stays a class)


# ---- 3. every placement --------------------------------------------------------------------------------------------------
_PLACE = {}


def placement_case():
    """a 40-mer and a 64-mer with one ambiguity letter in each field of the tail; per placement of <= 2 substitutions to a
    base outside the class at that position one text on a random concrete variant: every position pair of the 40-mer; of
    the 64-mer the clean text, every single position and a fixed sample of 2,000 position pairs; and 300 texts with three substitutions; texts are entries of their own"""
    if not _PLACE:
        rng = np.random.default_rng(7200)
        prim, texts, far, subs, owner = [], [], [], [], []
        for L, four in ((40, "RYKN"), (64, "BDMS")):
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
                combos = list(itertools.combinations(free, r))
                if len(p) == 64 and r == 2:
                    combos = [combos[i] for i in sorted(rng.choice(len(combos), size=2000, replace=False).tolist())]
                for where in combos:
                    texts.append(text_of(p, where))
                    subs.append(r)
        for _ in range(300):
            o = int(rng.integers(0, 2))
            p = prim[o]
            free = [i for i, ch in enumerate(p) if ch != "N"]
            far.append(text_of(p, rng.choice(free, size=3, replace=False).tolist()))
            owner.append(o + 1)
        decoys = [rand_seq(rng, int(rng.integers(20, 29))) for _ in range(100)]
        ents = texts + far
        bounds, at = [], 1
        for e in ents:
            bounds.append((at, at + len(e)))
            at += len(e) + 1
        _PLACE.update(pats=prim + decoys, codes=synth.normalize(synth.stream(ents), TABLE), subs=subs, owner=owner, far_bounds=bounds[len(texts):])
    return _PLACE


@pytest.mark.parametrize("name", ["K2", "K1", "k0"])
def test_every_placement(name):
    c = placement_case()
    want = oracle_hits(c["codes"], TABLE, c["pats"], name)
    selected, d, got = run(c["pats"], name, c["codes"], TABLE)
    assert selected[1] == sat_amd.KERNEL_SEED and "pm_wild_sub_scan for 2 patterns" in d and (", 2 " + LONG_TEXT) in d and "does not take" not in d, d
    assert got == want, (name, len(got), len(want))
    K = OPTS[name][0]
    own = [(end, pid) for end, pid, _ in got if pid <= 2]
    assert len(own) >= sum(1 for r in c["subs"] if r <= K), (name, len(own))   # a hit per text built within K substitutions, at least
    starts = np.array([a for a, _ in c["far_bounds"]])
    for end, pid in own:                                             # no text with three substitutions holds a hit of its own primer
        j = int(np.searchsorted(starts, end, side="right")) - 1
        if j >= 0:
            a, b = c["far_bounds"][j]
            assert not (a < end <= b) or c["owner"][j] != pid, (name, end, pid, j)


# ---- 4. edges ------------------------------------------------------------------------------------------------------------
def wild_tail(rng, t, with_n=True):
    """a class primer that matches t: four letters, one in each field of the tail"""
    p = list(t)
    for f, n in zip(range(4), rng.permutation(4).tolist()):
        i = len(t) - 16 + 4 * f + int(rng.integers(0, 4))
        p[i] = "N" if n == 0 and with_n else str(rng.choice([c for c in "BDHV" if t[i] in CLASS[c]]))
    return "".join(p)


@pytest.mark.parametrize("name", list(OPTS))
def test_tiny_streams_and_stream_ends(name):
    """streams of L - 1, L and L + 1 bases for L = 33, 52 and 64, a hit that starts at the first byte and one that ends at the
    last base, in whole scans and in ranges of 3"""
    rng = np.random.default_rng(7300)
    t = rand_seq(rng, 64)
    pats = [wild_tail(rng, t), wild_tail(rng, t[:52]), wild_tail(rng, t[:33]), wild_tail(rng, t[12:]), wild_tail(rng, rand_seq(rng, 45)), rand_seq(rng, 22)]
    assert all(in_class(p, 2, False) for p in pats[:5])
    streams = [t[:32], t[:33], t[:34], t[:51], t[:52], t[:53], t[:63], t, t + "G", "G" + t + rand_seq(rng, 10), t + "\n" + rand_seq(rng, 40) + t, "\n" + t]
    for raw in streams:
        codes = synth.normalize(raw.encode(), TABLE)
        want = oracle_hits(codes, TABLE, pats, name)
        for chunk in (1 << 26, 3):
            selected, d, got = run(pats, name, codes, TABLE, chunk=chunk)
            assert selected[1] == sat_amd.KERNEL_SEED and "pm_wild_sub_scan for 5 patterns" in d and (", 5 " + LONG_TEXT) in d, d
            assert got == want, (name, raw, chunk, got, want)
    want = oracle_hits(synth.normalize(streams[10].encode(), TABLE), TABLE, pats, name)
    assert {pid for _, pid, _ in want} >= {1, 2, 3, 4}               # hits that start at byte 0 and hits that end at the last byte


@pytest.mark.parametrize("name", list(OPTS))
def test_eos_and_n_inside_the_window(name):
    """an end-of-sequence character at every index of the window of a 64-mer (never a hit), a text N at every index (a mismatch)"""
    rng = np.random.default_rng(7301)
    t = rand_seq(rng, 64)
    pats = [wild_tail(rng, t, with_n=False)] + [rand_seq(rng, 21) for _ in range(5)]   # (filter_bitvec keeps an N primer on an N stream in the residue)
    parts = []
    for i in range(64):
        parts += [rand_seq(rng, 7) + t[:i] + "\n" + t[i + 1:] + rand_seq(rng, 9), rand_seq(rng, 5) + t[:i] + "N" + t[i + 1:] + rand_seq(rng, 11)]
    raw = ("\n".join(parts) + "\n" + t).encode()
    k = OPTS[name][0]
    for codes, table in ((synth.normalize(raw, TABLE_N), TABLE_N), (np.frombuffer(raw, dtype=np.uint8), None)):
        want = oracle_hits(codes, table, pats, name)
        selected, d, got = run(pats, name, codes, table)
        assert "pm_wild_sub_scan for 1 patterns" in d and (", 1 " + LONG_TEXT) in d and "does not take" not in d, d
        assert got == want, (name, got, want)
        own = [x for x in want if x[1] == 1]
        assert len(own) == (1 if k == 0 else 65), own                # the clean copy; under -K also the 64 with one N


@pytest.mark.parametrize("name", ["k0", "K2"])
def test_scan_ranges_and_handle_forms(name):
    """pm_scan in ranges of 1..5 positions across the hits, a windowed handle with the smallest window it takes (four times its
    halo), a packed handle, and two position shards with a long class primer's hit straddling the cut"""
    c = case()
    pats = c["lists"]["d"]
    codes, table, has_n = c["streams"]["table"]
    want = want_of("d", name, "table")
    n = codes.size
    k = OPTS[name][0]
    pm = engine(pats, name)
    try:
        pm.init(codes, table)
        got, pos, step = [], 0, 1
        while pos < n:                                                # ranges of 1, 2, .. 5, 1, .. positions
            e = min(n, pos + step)
            v = pm.scan_view(pos, e)
            got += list(zip(v["end"].tolist(), v["pid"].tolist(), v["k"].tolist()))
            pos, step = e, step % 5 + 1
        assert sorted(got) == want, (name, len(got), len(want))
        if name == "K2":                                             # shards: the cut 30 characters inside a long class primer's hit
            seam = next(end for end, pid, _ in want if len(pats[pid - 1]) > 32 and in_class(pats[pid - 1], k, has_n) and end > 300) - 30
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
        pm = engine(pats, name)
        try:
            if packed:
                bits = max(1, (len(table) - 1).bit_length())
                pm.init_packed(sat_amd.pack_codes(codes, bits), bits, n, table)
            else:
                pm.init(codes, table, window=1)                       # (the smallest window the handle takes)
            check_route(pats, name, has_n, pm.selected(), pm.describe())
            got = sat_amd.sorted_tuples(pm.find_all(chunk=1 << 26 if packed else 700))
            res = pm.residency()
        finally:
            pm.close()
        assert got == want, (name, packed, len(got), len(want))
        assert res["bits"] > 0 if packed else (0 < res["window"] < n and res["loads"] > 1), res


# ---- 5. zones ------------------------------------------------------------------------------------------------------------
def test_zones():
    """-5 6 and -3 40 on 52-mer class primers under -K 2 (a class-only list): a substitution inside a zone still chains and is
    never the hit; the 3' zone of 40 reaches from character 12 to the end, past character 32"""
    rng = np.random.default_rng(7400)
    ents = synth.make_entries(rng, 2, 3000)
    codes = synth.normalize(synth.stream(ents), TABLE)
    pats, zones = [], []
    for i in range(60):
        e = ents[i % 2]
        a = int(rng.integers(0, len(e) - 52))
        p = add_letters(rng, e[a:a + 52], 4, alphabet="BDHVN")
        where = [2, 20, 45, 8, None][i % 5]                            # a substitution inside the 5' zone, inside the 3' zone (before and behind character 32), outside both, none
        if where is not None and p[where] in BASES:
            p = p[:where] + BASES[(BASES.index(p[where]) + 1) % 4] + p[where + 1:]
        if in_class(p, 2, False):
            pats.append(p)
            zones.append([(6, 0), (0, 40), (6, 40)][i % 3])
    want = oracle_hits(codes, TABLE, pats, "K2", zones=zones)
    plain = oracle_hits(codes, TABLE, pats, "K2")
    assert want != plain and len(want) >= 15                         # a violation changes the outcome somewhere, and hits remain
    selected, d, got = run(pats, "K2", codes, TABLE, zones=zones)
    assert d.startswith("kernel=pm_wild_sub_scan+pm_wild_sub_verify for %d patterns" % len(pats)) and (", %d %s" % (len(pats), LONG_TEXT)) in d, d
    assert got == want, (len(got), len(want))


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals():
    c = case()
    rng = np.random.default_rng(7500)
    pats = c["lists"]["b"]
    codes, table, _ = c["streams"]["table"]
    nclass, nlong, nrest = counts(pats, "K2", False)
    assert (nclass, nlong, nrest) == (20, 20, 0)
    e0 = c["ents"][0]
    # a 65-mer with letters stays in the residue; so does a 52-mer with five N's in one field pair (more than 256 keys)
    p65 = add_letters(rng, e0[200:265], 4, alphabet=NO_N)
    five = list(e0[400:452])
    for i in (36, 37, 38, 40, 41):
        five[i] = "N"
    five = "".join(five)
    assert not in_class(p65, 2, False) and not in_class(five, 2, False) and variants(five) > 16
    extra = pats + [p65, five]
    want = oracle_hits(codes, table, extra, "K2")
    assert {len(pats) + 1, len(pats) + 2} <= {pid for _, pid, _ in want}
    _, d, got = run(extra, "K2", codes, table)
    assert "pm_wild_sub_scan for 20 patterns" in d and (", 20 " + LONG_TEXT) in d and "for 2 patterns the seed plan does not take" in d, d
    assert got == want
    # a class over the entry cap: 100 52-mers with 256 keys in every pair beside the list leave every primer where it was
    heavy = []
    for _ in range(100):
        p = list(rand_seq(rng, 52))
        for f in range(4):
            p[36 + 4 * f], p[36 + 4 * f + 2] = "N", "N"
        heavy.append("".join(p))
    _, d, got = run(pats + heavy, "K2", codes, table)
    _, d32, got32 = run(pats + heavy, "K2", codes, table, bits=32)
    assert "pm_wild_sub_scan" not in d and d == d32 and got == got32 == oracle_hits(codes, table, pats + heavy, "K2"), d
    # indels on; the bit-parallel kernels by name; the seed kernels by name (an error, as before)
    _, d, got = run(pats, "K2", codes, table, indels=True)
    assert "pm_wild_sub_scan" not in d and got == oracle_hits(codes, table, pats, "K2", indels=True), d
    _, d, got = run(pats, "K2", codes, table, kernel=sat_amd.KERNEL_BITPAR)
    assert d.startswith("kernel=pm_bitpar_scan<2,false>") and got == want_of("b", "K2", "table"), d
    with pytest.raises(sat_amd.PmError) as ei:
        run(pats, "K2", codes, table, kernel=sat_amd.KERNEL_SEED)
    assert ei.value.code == -2 and "seed engine: IUPAC wildcards run on the bit-parallel family" in str(ei.value), str(ei.value)


# ---- 7. behind the scan --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(OPTS))
def test_counts_and_device_alignment(name):
    c = case()
    pats = c["lists"]["b"]
    codes, table, has_n = c["streams"]["table"]
    want = want_of("b", name, "table")
    k, indels = OPTS[name][0], OPTS[name][1]
    text = O.Text(codes, table)
    eds = [O.cli_align(text, pats[pid - 1], end, k, indels, wildcards=True)[3] for end, pid, _ in want]
    pm = engine(pats, name)
    try:
        pm.init(codes, table)
        check_route(pats, name, has_n, pm.selected(), pm.describe())
        for M in (0, 2):
            wc, wcap, winfo = count_rule.tally(want, lambda i: eds[i], len(pats), k, M)
            pm.reset()
            cnt, capped, info = pm.count_all(max_count=M)
            assert cnt.tolist() == wc and capped.tolist() == wcap
            for f in ("tallied", "skipped", "bogus"):
                assert info[f] == winfo[f], (f, info[f], winfo[f])
        pm.reset()
        hits = pm.find_all()
        own = hits[np.array([len(pats[pid - 1]) > 32 for pid in hits["pid"].tolist()], dtype=bool)]
        assert own.size >= 8
        dev = pm.align_hits_device_numpy(own)
        host = pm.align_hits(own)
        for f in ("start", "end", "editdist", "value"):
            assert dev[f].tolist() == host[f].tolist(), f
    finally:
        pm.close()


@pytest.mark.parametrize("lengths,text", [((45, 52, 60), True), ((45, 52, 64), False)], ids=["text-60", "records-64"])
def test_pcr_pair_round_over_long_degenerate_primers(lengths, text):
    """pm_pcr_scan + pm_pcr_pair over three pairs of long class primers (both strands in the list, as pm_pcr_match adds them):
    the amplicons, their re-alignments and -- with text -- strings equal the host loop's (tests/pcr_rule.py) on the hits
    find_all reports.  check_round's byte accounting takes text rows of 64 characters, which hold L + k up to 64: the round with
    text runs primers of up to 60 characters, the round with a 64-mer compares the records and re-alignments"""
    import pcr_rule as R
    from test_gpu_pcr_pairs import check_round, realign

    class W:
        pass
    rng = np.random.default_rng(7600)
    ents = [rand_seq(rng, 2500), rand_seq(rng, 2500)]
    w = W()
    w.raw = synth.stream(ents)
    w.n = len(w.raw)
    w.starts = [1, 2 + len(ents[0])]
    s = w.raw.decode()
    sites = [(w.starts[0] + 300, w.starts[0] + 600), (w.starts[0] + 1500, w.starts[0] + 1850), (w.starts[1] + 700, w.starts[1] + 1000)]
    prim = []
    for j, (a, b) in enumerate(sites):                               # both primers as they stand on the stream (ids 2j - 1, 2j: tests/pcr_rule.py)
        L = lengths[j]
        prim += [wild_tail(rng, s[a:a + L], with_n=False), wild_tail(rng, s[b:b + L], with_n=False)]
    assert all(in_class(p, 2, False) for p in prim)
    pats = prim + [synth.revcomp_iupac(p) for p in prim]
    codes = synth.normalize(w.raw, TABLE)
    pm = engine(pats, "K2")
    try:
        pm.init(codes, TABLE)
        pm.pcr_setup(amplicon_max=480, entry_starts=w.starts)
        found = pm.find_all()
        d = pm.describe()
        assert d.startswith("kernel=pm_wild_sub_scan+pm_wild_sub_verify for 12 patterns") and (", 12 " + LONG_TEXT) in d, d
        hits = sorted(zip(found["end"].tolist(), found["pid"].tolist(), found["k"].tolist()))
        assert len(hits) >= 6                                        # every site
        res = realign(pm, found, 2)
        rule = R.Rule(len(prim), [0] + [len(p) for p in pats], 2, False, False, False, 0, 480, -1, None)
        pm.reset()
        got = 0
        for begin in range(0, w.n, 1000):
            got += pm.pcr_scan(begin, min(w.n, begin + 1000))
        assert got == len(hits)
        want, carried = check_round(pm, w, rule, res, hits, w.n, False, text=text)
        assert carried == [] and {x[5] for x in want} >= {1, 2, 3}
    finally:
        pm.close()


def test_suspect_list_grows_and_the_range_is_scanned_again():
    """the homopolymer construction of tests/test_gpu_wild_class.py with one 40-mer class primer: 500,000 A's under a primer
    whose last 16 characters accept them in every field pair and whose first 24 do not -- six suspects per window.  The list
    holds 2 * (n / 128 + 2^20) suspects at first, so it overflows from 350,438 windows on: 355,000 A's give 2.13 * 10^6
    suspects against 2.10 * 10^6 (the construction's 500,000 are not needed).  The scan counts past the list's end without
    writing there, the list grows, the range is scanned again, and the hits are the oracle's"""
    rng = np.random.default_rng(7700)
    head = "CCCCCCCCGTGTCCCCGTGTCCCC"
    p = head + "ANAAADAAAVAAAHAA"
    assert len(p) == 40 and in_class(p, 2, False)
    site = head + "AGAAATAAACAAATAA"
    ents = [rand_seq(rng, 50) + site + rand_seq(rng, 50), "G" + "A" * 355000 + "G", rand_seq(rng, 30) + site[:5] + "G" + site[6:] + rand_seq(rng, 30)]
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
    assert d.startswith("kernel=pm_wild_sub_scan+pm_wild_sub_verify for 1 patterns") and (", 1 " + LONG_TEXT) in d, d
    assert st["internal_rescans"] >= 1 and st["between_stages"] > 1 << 21, st
    assert got == want, (got, want)
