"""GPU: windows on keys beyond their row's slots, now that the row's overflow marker holds those keys' patterns.

A row of the pair plan's slot table (32 keys) has `stride` slots (PM_PAIR_ROW; 12 by default); the keys ranked
stride - 1 or later share the last one, the overflow marker.  pair_build (csrc/pm_pair.hip) writes their patterns into
it, so pm_pair_scan / pm_pair_edit_scan dismiss a window on such a key whose other ten bases are far from all of them,
as they do for every other key; with PM_SEED_DEBUG bit 6 the markers are the empty flagged ones of earlier versions and
every such window is a suspect for pm_pair_verify.

The patterns are families of row mates (equal in one key field and in the low five bits of the other): 12, 13 (two
patterns per key), 14 and 16 keys in a row for the default stride, 2..5 for strides 2 and 3 -- markers with one, two,
three patterns and flagged ones.  For every (pattern on an overflow key, field pair whose row overflows) the text holds
the key with the other ten bases at distance 0, 1, 2 and 3 from the pattern, and 48 times with other bases that are
further than 2 from every pattern of the row (400 times at the default stride, where few rows overflow).  Checked per
case (-K 1 and -K 2 at strides 2, 3 and the default; -k 2, whose tables hold two patterns per slot, at stride 3):
  * the hits are the oracle's (shift_and_inexact.cc:249-352) and, sorted, equal to those of a handle created with the
    debug bit;
  * -K: the handle with the debug bit passes at least ten times as many suspects between its kernels as there are hits,
    the shipped one strictly fewer than that handle.  (-k 2: pm_scan_stats counts the seed records BEHIND
    pm_pair_edit_resolve there, which walks every suspect's run in full: they must be equal.)
"""
import numpy as np
import pytest

import synth
import sat_amd
from oracle import pmoracle as O

pytestmark = pytest.mark.gpu

TABLE = b"ACGT\n"
PAIRS = {1: [(0, 1), (2, 3)], 2: [(a, b) for a in range(4) for b in range(a + 1, 4)]}
FAR = {2: 48, 3: 48, 12: 400}                                      # dismissable windows per (overflow pattern, field pair), by stride


def field(w, j):
    return (w >> (10 * j)) & 0x3FF


def word_to_str(w):
    return "".join("ACGT"[(w >> (2 * i)) & 3] for i in range(20))


def family_words(rng):
    """Row mates of field pair (a, b) agree in field a and in the low 5 bits of field b: a family fixes a word but for the
    high 5 bits of field b (one value per key) and one other field, `vary` (random per pattern)."""
    words = []
    fams = [(1, 2, 16, 1), (2, 3, 13, 2), (3, 0, 12, 1), (3, 1, 14, 1), (1, 3, 3, 2), (2, 0, 4, 0)]
    fams += [(b, vary, m, 1) for b, vary in ((1, 2), (2, 3), (3, 0), (3, 1)) for m in (2, 3, 4, 5)]
    for b, vary, m, per_key in fams:                                 # per_key 0: the keys' patterns agree outside field b
        f = [int(x) for x in rng.integers(0, 1 << 10, size=4)]
        for hi in rng.choice(32, size=m, replace=False):
            f[b] = (f[b] & 31) | (int(hi) << 5)
            for _ in range(max(per_key, 1)):
                if per_key:
                    f[vary] = int(rng.integers(0, 1 << 10))
                words.append(sum(x << (10 * j) for j, x in enumerate(f)))
    return words


def hamming10(x, y):
    """bases that differ between two 20-bit words (ten bases of 2 bits)"""
    z = x ^ y
    z = (z | (z >> 1)) & 0x55555
    return bin(z).count("1")


def make_case(stride, k):
    """patterns and text for tables of `stride` slots per row with the field pairs of -K k"""
    rng = np.random.default_rng(9100 + 10 * stride + k)
    words = family_words(rng)
    kmax = stride - 1
    sites = []
    groups = 0
    for a, b in PAIRS[k]:
        c, d = [j for j in range(4) if j not in (a, b)]
        other = lambda w: field(w, c) | (field(w, d) << 10)
        rows = {}
        for w in words:
            key = field(w, a) | (field(w, b) << 10)
            rows.setdefault(key & 0x7FFF, {}).setdefault(key >> 15, []).append(w)
        for row, keys in rows.items():
            row_others = [other(w) for ws in keys.values() for w in ws]
            for rank, bit in enumerate(sorted(keys)):
                if rank < kmax:
                    continue
                for w in keys[bit]:                                  # a pattern on an overflow key of this field pair
                    groups += 1
                    put = lambda o: (w & ~((0x3FF << (10 * c)) | (0x3FF << (10 * d)))) | ((o & 0x3FF) << (10 * c)) | ((o >> 10) << (10 * d))
                    for dist in range(4):
                        o = other(w)
                        for pos in rng.choice(10, size=dist, replace=False):
                            o ^= int(rng.integers(1, 4)) << (2 * int(pos))
                        assert hamming10(o, other(w)) == dist
                        sites.append(word_to_str(put(o)))
                    n = 0
                    while n < FAR[stride]:
                        o = int(rng.integers(0, 1 << 20))
                        if min(hamming10(o, x) for x in row_others) > 2:
                            sites.append(word_to_str(put(o)))
                            n += 1
    rnd = lambda n: "".join(rng.choice(list("ACGT"), size=n).tolist())
    pats = [word_to_str(w) for w in words]
    pats += [rnd(int(rng.integers(1, 12))) + p for p in pats[:12]]   # longer ones (the plan looks at the last 20 bases)
    order = rng.permutation(len(sites))
    raw = ("\n" + "".join(rnd(int(rng.integers(3, 20))) + sites[i] for i in order) + rnd(50) + "\n").encode()
    return pats + [synth.revcomp(p) for p in pats], synth.normalize(raw, TABLE), groups


def run(allp, codes, k, indels, monkeypatch, debug):
    if debug:
        monkeypatch.setenv("PM_SEED_DEBUG", "64")
    else:
        monkeypatch.delenv("PM_SEED_DEBUG", raising=False)
    pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sat_amd.SEM_SHIFT_AND_INEXACT, kernel=sat_amd.KERNEL_SEED)
    for i, p in enumerate(allp):
        pm.add_pattern(p, i + 1)
    pm.init(codes, TABLE)
    desc = pm.describe()
    got = sat_amd.sorted_tuples(pm.find_all(chunk=1 << 26))
    between = pm.scan_stats()["between_stages"]
    pm.close()
    return got, between, desc


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("row_slots", [2, 3, None])
def test_overflow_keys_are_settled_by_their_marker(row_slots, k, monkeypatch):
    if row_slots is not None:
        monkeypatch.setenv("PM_PAIR_ROW", str(row_slots))
    monkeypatch.setenv("PM_SEED_CHUNK", "16384")
    allp, codes, groups = make_case(row_slots or 12, k)
    assert groups >= 8 and codes.size < 600000, (groups, codes.size)
    want = O.sorted_tuples(O.find_all(O.Text(codes, TABLE), allp, engine=100, k=k, indels=False))
    got, between, desc = run(allp, codes, k, False, monkeypatch, False)
    assert "pm_pair_scan" in desc and (row_slots is None or "row_slots=%d" % row_slots in desc), desc
    old, between_old, _ = run(allp, codes, k, False, monkeypatch, True)
    print("row_slots %s -K %d: %d bases, %d overflow (pattern, pair) groups, %d hits, suspects %d, with empty markers %d"
          % (row_slots, k, codes.size, groups, len(want), between, between_old))
    assert got == want and len(want) >= groups, (row_slots, k, len(got), len(want), groups)
    assert old == got, (row_slots, k, len(old), len(got))
    assert between_old >= 10 * len(want), (row_slots, k, between_old, len(want))
    assert between < between_old, (row_slots, k, between, between_old)


def test_overflow_keys_of_the_edit_plan(monkeypatch):
    """-k 2: pm_pair_edit_scan on tables with two patterns per slot; pm_pair_edit_resolve walks a suspect's whole run"""
    monkeypatch.setenv("PM_PAIR_ROW", "3")
    monkeypatch.setenv("PM_SEED_CHUNK", "16384")
    allp, codes, groups = make_case(3, 2)
    want = O.sorted_tuples(O.find_all(O.Text(codes, TABLE), allp, engine=sat_amd.SEM_SHIFT_AND_INEXACT, k=2, indels=True))
    got, between, desc = run(allp, codes, 2, True, monkeypatch, False)
    assert "pm_pair_edit_scan" in desc, desc
    old, between_old, _ = run(allp, codes, 2, True, monkeypatch, True)
    print("-k 2 row_slots 3: %d bases, %d groups, %d hits, seed records %d, with empty markers %d" % (codes.size, groups, len(want), between, between_old))
    assert got == want and len(want) >= groups, (len(got), len(want), groups)
    assert old == got, (len(old), len(got))
    assert between == between_old, (between, between_old)
