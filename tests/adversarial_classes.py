"""tests/adversarial.py's small cases with every opt-in primer class in one list: each primer drawn from a length band of
its own -- 16..19 (the short classes), 20..32 (the main class), 33..64 (wide tiles, 4.9 .. 4.12), now
and then 12..15 and 65..70 (the bit-parallel residue) -- under -w with 0 .. 5 ambiguity letters per primer (plain, expanded
into the main class, or the degenerate class of pm_wild_sub_scan, 4.13), and `route`: the permission bits of
pm_config.long_patterns as keyword arguments of sat_amd.PatternMatch, all seven on three cases in four, a random subset on
the fourth.  Streams, zones, engines, k, knobs, record caps, modes as in adversarial.small_case.  Shared by
tests/test_gpu_adversarial_classes.py (fixed seeds) and scripts/fuzz_families.py --oracle --classes (open-ended)."""
import numpy as np

import adversarial as A
import sat_amd

BITS = ("long_patterns", "long_exact", "long_edits", "long_halves", "long_align", "wild_class", "edit_pair")
# (lo, hi, weight) of a primer's length band
BANDS = ((16, 19, 3.0), (20, 32, 3.0), (33, 64, 4.0), (12, 15, 0.5), (65, 70, 0.5))
R806 = "GGACTACNVGGGTWTCTAAT"                                       # 806R: 24 concrete variants
VARIANTS = {c: 1 for c in "ACGT"}
VARIANTS.update({c: 2 for c in "RYKMSW"})
VARIANTS.update({c: 3 for c in "BDHV"})
VARIANTS["N"] = 4


def variants(p):
    v = 1
    for ch in p:
        v *= VARIANTS[ch]
    return v


def kind(p):
    """plain / expanded (at most 16 concrete variants) / degenerate (more)"""
    v = variants(p)
    return "plain" if v == 1 else "expanded" if v <= 16 else "degenerate"


def class_case(seed):
    """One case of the shape of adversarial.small_case (its keys, so that describe / gpu_hits / oracle_hits take it) plus
    `route` and `lens`, the primers' lengths.  600 .. 8000 characters, 4 .. 80 primers x 2 strands."""
    rng = np.random.default_rng([seed, 0xC1A55])                      # (a stream of its own: no case shares its text with small_case(seed))
    style = int(rng.integers(0, 4))
    n = int(rng.integers(600, 8001))
    s = A.make_stream(rng, n, style)
    k = int(rng.integers(0, 3))
    indels = bool(rng.integers(0, 2)) and k > 0
    count = int(rng.integers(4, 81))
    # now and then a residue: five lists in eight have neither a primer of 12..15 nor one of 65..70 characters (exact_halves
    # keeps no residue, and one primer of 10..15 characters keeps a -K list off the pair plan: DESIGN.md 4.8, 4.9, 4.12), one has
    # the long ones only, one the short ones only, one has both
    residue = (0, 0, 0, 0, 0, 2, 1, 3)[int(rng.integers(0, 8))]
    w = np.array([b[2] for b in BANDS])
    w[3] *= residue & 1
    w[4] *= residue >> 1
    pats = []
    for b in rng.choice(len(BANDS), size=count, p=w / w.sum()):
        lo, hi, _ = BANDS[int(b)]
        pats += A.make_patterns(rng, s, 1, lo, hi, k)
    allp = pats + [sat_amd.reverse_comp(p) for p in pats]
    wild = bool(rng.integers(0, 3) == 0)                              # ambiguity codes in the primers (-w) on a third of the cases
    if wild:
        wp = []
        for p in allp:
            q = list(p)
            for _ in range(int(rng.integers(0, 6))):                  # 0 .. 5 ambiguity letters
                i = int(rng.integers(0, len(q)))
                if q[i] in A.IUPAC:
                    q[i] = A.IUPAC[q[i]][int(rng.integers(0, 7))]
            wp.append("".join(q))
        allp = wp
        if rng.integers(0, 3) == 0:                                   # 806R, forward and reversed: two primers of 24 concrete variants
            allp += [R806, R806[::-1]]
    sem, sname = A.SEMS[int(rng.integers(0, len(A.SEMS)))]
    zones = None
    if sem == sat_amd.SEM_EXACT_BASES or rng.integers(0, 3) == 0:    # exact zones on a third of the cases, always for exact_bases
        zones = []
        for p in allp:
            e, f_ = (int(rng.integers(0, 9)), 0) if rng.integers(0, 2) else (0, int(rng.integers(0, 9)))
            if rng.integers(0, 4) == 0:
                e, f_ = int(rng.integers(0, 7)), int(rng.integers(0, 7))
            if sem == sat_amd.SEM_EXACT_BASES and max(e, f_) < 6:
                e = 6 + int(rng.integers(0, 4))
            zones.append((min(e, len(p)), min(f_, len(p))))
    with_n = bool(rng.integers(0, 4) == 0)
    env = {}
    for name, val in A.KNOBS:
        v = val[int(rng.integers(0, len(val)))]
        if v is not None:
            env[name] = v
    cap = [1 << 10, 1 << 14, 1 << 20][int(rng.integers(0, 3))]
    mode = int(rng.integers(0, 4))
    raw = bool(rng.integers(0, 4) == 0)
    table = None if raw else (b"ACGT\nN" if with_n else A.TABLE)
    if with_n:
        s = s.copy()
        s[rng.integers(0, n, int(rng.integers(1, 40)))] = 5
    if not raw and rng.integers(0, 8) == 0:                           # the end-of-entry character first in the table (code 0)
        table = b"\nACGT" + (b"N" if with_n else b"")
        s = np.array([1, 2, 3, 4, 0, 5], dtype=np.uint8)[s]
    stream = np.frombuffer(b"ACGT\nN", dtype=np.uint8)[s].copy() if raw else s
    chunk = int(rng.integers(64, 3000))
    cut = int(rng.integers(n // 4, 3 * n // 4))
    host = bool(rng.integers(0, 3) == 0)
    if rng.integers(0, 4):                                            # all seven bits on three cases in four
        route = {b: True for b in BITS}
    else:                                                             # a random subset: a route beside another route's former path
        route = {b: bool(rng.integers(0, 2)) for b in BITS}
    lens = [len(p) for p in allp]
    return dict(seed=seed, style=style, n=n, k=k, indels=indels, lo=min(lens), hi=max(lens), patterns=allp, sem=sem, sname=sname, zones=zones,
                wild=wild, with_n=with_n, env=env, cap=cap, mode=mode, raw=raw, table=table, stream=stream, chunk=chunk, cut=cut, host=host,
                route=route, lens=lens)


def describe(c):
    return "class " + A.describe(c) + " bits " + "".join("1" if c["route"][b] else "0" for b in BITS)
