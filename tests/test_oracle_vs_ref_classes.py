"""CPU: the oracle against the real reference engines (oracle/_ref/ref_harness where it is built, its recorded runs where
it is not: tests/refrec.py) at the shapes of tests/adversarial_classes.py, which tests/test_oracle_vs_ref.py does not draw:
lists that mix primers of 16..19, 20..32, 33..64 and 65..70 characters, both strands, on tandem-repeat and skewed text
(tests/adversarial.make_stream: most windows are seed hits), and under -w primers with 0 .. 5 ambiguity letters, 806R and
mlCOIintF among them.  Engines as the reference selects them, filter_bitvec, exact_halves and bare shift_and_inexact.

No primer is left out of any option set: "Bogus hit returned to primer_match main()", with which the reference's primer_match
ends at k = 0 -w on 806R (tests/golden/make_cli_wild_golden.py), comes from that program's re-alignment of an engine's hit;
ref_harness prints the engines' hits as they are and ends with status 0 on every list here."""
import numpy as np
import pytest

import adversarial as A
import refrec
from oracle import pmoracle as O

TABLE = b"ACGT\n"
BANDS = ((16, 19), (20, 32), (33, 64), (65, 70))
NAMED = ["GGACTACNVGGGTWTCTAAT", "GGWACWGGWTGAACWGTWTAYCCYCC"]        # 806R, mlCOIintF
OPTIONS = [(0, False), (1, False), (2, False), (1, True), (2, True)]   # k = 0, -K 1, -K 2, -k 1, -k 2
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
CLASS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "K": "GT", "M": "AC", "S": "CG", "W": "AT", "B": "CGT", "D": "AGT", "H": "ACT",
         "V": "ACG", "N": "ACGT"}


def make_case(seed, wild):
    """a stream of 300 .. 1500 characters (tandem: even seeds, skewed: odd), 2 .. 4 primers per length band cut from it
    with 0 .. 3 edits, and their reverse complements; under -w 0 .. 5 ambiguity letters in every primer"""
    rng = np.random.default_rng([seed, 77, int(wild)])
    n = int(rng.integers(300, 1501))
    s = A.make_stream(rng, n, 3 if seed % 2 == 0 else 1)
    pats = []
    for lo, hi in BANDS:
        pats += A.make_patterns(rng, s, int(rng.integers(2, 5)), lo, hi, 2)
    allp = pats + ["".join(COMP[ch] for ch in reversed(p)) for p in pats]
    if wild:
        wp = []
        for p in allp:
            q = list(p)
            for _ in range(int(rng.integers(0, 6))):
                i = int(rng.integers(0, len(q)))
                if q[i] in A.IUPAC:
                    q[i] = A.IUPAC[q[i]][int(rng.integers(0, 7))]
            wp.append("".join(q))
        allp = wp
        at = int(rng.integers(0, n - 60))                             # a site of each named primer in the text, the first of its variants
        for p in NAMED:
            site = ["ACGT".index(CLASS[ch][0]) for ch in p]
            s[at:at + len(site)] = site
            at = (at + 31) % (n - 60)
        allp += NAMED
    return s, allp


def compare(seed, wild, s, allp, k, indels, sel):
    """one run of ref_harness against the oracle; returns the reference's hits"""
    cmd = ["-N", str(sel), "-n", "-i", "{d}/db", "-P", "{d}/pat.txt"] + (["-w"] if wild else [])
    if k:
        cmd += ["-k" if indels else "-K", str(k)]
    inputs = {"db.sqn": s.tobytes(), "db.tbl": TABLE, "pat.txt": ("\n".join(allp) + "\n").encode()}
    status, out, _ = refrec.run("ref_harness", cmd, inputs, timeout=300)
    assert status == 0, (seed, wild, k, indels, sel, status)
    ref = refrec.hits(out)
    got = O.sorted_tuples(O.find_all(O.Text(s, TABLE), allp, engine=sel, k=k, indels=indels, wildcards=wild))
    assert got == ref, (seed, wild, k, indels, sel, len(got), len(ref), sorted(set(ref) - set(got))[:4], sorted(set(got) - set(ref))[:4])
    return ref


def engines(k, wild):
    """0: as pick_pattern_index selects; filter_bitvec, exact_halves (over shift_and under -w), bare shift_and_inexact"""
    if k == 0:
        return [0, O.SHIFT_AND] if wild else [0]
    return [0, O.FILTER_BITVEC, O.EXACT_HALVES_SA if wild else O.EXACT_HALVES_KT, O.SHIFT_AND_INEXACT]


@pytest.mark.parametrize("seed", range(4))
def test_mixed_length_lists_against_reference(seed):
    s, allp = make_case(seed, False)
    bands = set()
    for k, indels in OPTIONS:
        for sel in engines(k, False):
            ref = compare(seed, False, s, allp, k, indels, sel)
            bands |= set(b for b, (lo, hi) in enumerate(BANDS) for h in ref if lo <= len(allp[h[1] - 1]) <= hi)
    assert bands == {0, 1, 2, 3}, (seed, bands)                        # hits of every length band


@pytest.mark.parametrize("seed", range(4))
def test_degenerate_lists_against_reference(seed):
    """-w with k = 0, -K 1, -K 2"""
    s, allp = make_case(seed, True)
    named = degenerate = 0
    for k, indels in OPTIONS[:3]:
        for sel in engines(k, True):
            ref = compare(seed, True, s, allp, k, indels, sel)
            named += sum(1 for h in ref if allp[h[1] - 1] in NAMED)
            degenerate += sum(1 for h in ref if sum(ch not in "ACGT" for ch in allp[h[1] - 1]) >= 3)
    assert named >= 6 and degenerate > named, (seed, named, degenerate)
