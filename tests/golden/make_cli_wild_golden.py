#!/usr/bin/env python3
"""Generate tests/golden/cli_wild.json from the REAL reference command lines (build container only).

A seeded FASTA database of about 40 kbp with planted sites and a primer file of 60 primers of 18..28 nt, twenty of them
with 3..6 IUPAC ambiguity letters -- 806R (GGACTACNVGGGTWTCTAAT) and mlCOIintF (GGWACWGGWTGAACWGTWTAYCCYCC) among them,
the primers that run on pm_wild_sub_scan where pm_config.long_patterns allows it -- go through
oracle/_ref/compress_seq and oracle/_ref/primer_match -w -r at k = 0, -K 1 and -K 2 (one run with -5 6) and one -c tally.
The -K 1 run and the run with -5 6 name the engine (-N 5, filter_bitvec): left to itself the reference picks exact_halves
at -K 1 and exact_bases with -5 6, which the class does not apply to (out of scope) and whose hits the
reference hands out in seed order, not in the (end, id) order of the GPU engine; those two runs are recorded as well
(K1_auto, K2_five_auto) and compared as sorted lines, like the other command-line fixtures of exact_halves.
Every recorded run must have at least 30 hit lines, at least 10 of them of the twenty degenerate primers: checked here.
At k = 0 the reference's own primer_match ends with "Bogus hit returned to primer_match main()" as soon as 806R or another
primer with an N next to a second ambiguity letter has a hit (its re-alignment disagrees with its search engine), so no
reference output exists for the whole list there: the k = 0 run carries the list without the primers for which the
reference fails alone (found here by running each primer on its own; their lines stay in the file as a placeholder
primer without a hit, so that the primer indices are the same in every run).
Stored: the inputs and the standard output per option set and database form.  Data only -- no reference source.  Re-run:
    make -C oracle ref && python tests/golden/make_cli_wild_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
ONE_LINE = "%i %r %s %e %d %p %q\\n"                                  # primer index, strand, start, end, distance, primer, site
CASES = [
    ("k0", ["-w", "-r", "-A", ONE_LINE]),
    ("K1", ["-w", "-r", "-K", "1", "-N", "5", "-A", ONE_LINE]),
    ("K2", ["-w", "-r", "-K", "2", "-A", ONE_LINE]),
    ("K2_five", ["-w", "-r", "-K", "2", "-5", "6", "-N", "5", "-A", ONE_LINE]),
    ("K2_counts", ["-w", "-r", "-K", "2", "-c"]),
    # the same two without -N: the reference picks exact_halves / exact_bases, engines the class does not apply to
    ("K1_auto", ["-w", "-r", "-K", "1", "-A", ONE_LINE]),
    ("K2_five_auto", ["-w", "-r", "-K", "2", "-5", "6", "-A", ONE_LINE]),
    # -5 6 on the list without the primers that carry a letter and are no class primers: the zoned list then stays on the seed
    # family and the zones go through pm_wild_sub_verify (primer file: zoned_primers_txt)
    ("K2_five_class", ["-w", "-r", "-K", "2", "-5", "6", "-N", "5", "-A", ONE_LINE]),
]
CLASS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "K": "GT", "M": "AC", "S": "CG", "W": "AT",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
NAMED = ["GGACTACNVGGGTWTCTAAT", "GGWACWGGWTGAACWGTWTAYCCYCC"]        # 806R, mlCOIintF


def class_primer(p):
    """the routing rule of DESIGN.md 4.13 at -K 2, restated: more than 16 concrete variants, at most 256 keys in every pair
    of the four fields of the last 16 characters"""
    n = 1
    for ch in p:
        n *= len(CLASS[ch])
    fields = [p[len(p) - 16 + 4 * f:len(p) - 12 + 4 * f] for f in range(4)]
    keys = [1, 1, 1, 1]
    for f in range(4):
        for ch in fields[f]:
            keys[f] *= len(CLASS[ch])
    return 16 <= len(p) <= 32 and n > 16 and all(keys[a] * keys[b] <= 256 for a in range(4) for b in range(a + 1, 4))


def concrete(rng, p):
    return "".join(str(rng.choice(list(CLASS[ch]))) for ch in p)


def build_inputs(seed):
    rng = np.random.default_rng(seed)
    ents = [list(s) for s in synth.make_entries(rng, 4, 10000)]
    degenerate, plain = list(NAMED), []
    while len(degenerate) < 20:                                        # windows of the database with 3..6 letters that hold the base
        L = int(rng.integers(18, 29))
        e = int(rng.integers(0, 4))
        a = int(rng.integers(0, len(ents[e]) - L))
        w = list("".join(ents[e][a:a + L]))
        for i in rng.choice(L, size=int(rng.integers(3, 7)), replace=False).tolist():
            w[i] = str(rng.choice([c for c in "RYKMSWBDHVN" if w[i] in CLASS[c]]))
        degenerate.append("".join(w))
    for n, p in enumerate(NAMED):                                      # planted sites of the two named primers: 0, 1 and 2 substitutions
        for r in range(6):
            site = synth.mutate(rng, concrete(rng, p), nsub=r % 3)
            if r % 2:
                site = synth.revcomp(site)
            e, a = (2 * n + r) % 4, 500 + 1500 * r + 700 * n
            ents[e][a:a + len(site)] = list(site)
    ents = ["".join(s) for s in ents]
    while len(plain) < 40:
        L = int(rng.integers(18, 29))
        e = int(rng.integers(0, 4))
        a = int(rng.integers(0, len(ents[e]) - L))
        w = synth.mutate(rng, ents[e][a:a + L], nsub=int(rng.integers(0, 5)) // 2)   # (two in five exact: hits at k = 0)
        plain.append(synth.revcomp(w) if int(rng.integers(0, 2)) else w)
    for i in range(0, 40, 8):                                          # a few with one or two letters: these stay in the main class
        w = list(plain[i])
        w[int(rng.integers(0, len(w)))] = "R" if w[0] in "AG" else "Y"
        plain[i] = "".join(w)
    pats = []
    for i in range(20):                                                # degenerate and plain primers interleaved
        pats += [degenerate[i], plain[2 * i], plain[2 * i + 1]]
    fasta = "".join(">entry%d synthetic len=%d\n%s" % (i + 1, len(s), "".join(s[j:j + 60] + "\n" for j in range(0, len(s), 60))) for i, s in enumerate(ents))
    return fasta, "\n".join(pats) + "\n", pats, [3 * i + 1 for i in range(20)]


def main():
    fasta, ptxt, pats, degenerate_ids = build_inputs(47)
    zoned = [p for p in pats if set(p) <= set("ACGT") or class_primer(p)]
    zoned_ids = [i + 1 for i, p in enumerate(zoned) if not set(p) <= set("ACGT")]
    out = {"fasta": fasta, "primers_txt": ptxt, "degenerate_ids": degenerate_ids, "zoned_primers_txt": "\n".join(zoned) + "\n",
           "zoned_degenerate_ids": zoned_ids, "cases": {}}
    with tempfile.TemporaryDirectory() as d:
        pf = os.path.join(d, "primers.P")
        with open(pf, "w") as f:
            f.write(ptxt)
        for variant, args in (("normalized", ["-n", "true"]), ("indexed", [])):
            os.mkdir(os.path.join(d, variant))
            fa = os.path.join(d, variant, "db.fa")
            with open(fa, "w") as f:
                f.write(fasta)
            r = subprocess.run([os.path.join(REF, "compress_seq"), "-i", fa] + args, capture_output=True)
            assert r.returncode == 0, r.stderr
            for cname, extra in CASES:
                use = pf
                if cname == "k0":                                      # the primers the reference cannot run at k = 0 (see above)
                    if "k0_primers_txt" not in out:
                        kept = []
                        for p in pats:
                            with open(os.path.join(d, "one.P"), "w") as f:
                                f.write(p + "\n")
                            r = subprocess.run([os.path.join(REF, "primer_match"), "-i", fa, "-P", os.path.join(d, "one.P")] + extra, capture_output=True)
                            kept.append(p if r.returncode == 0 else "ACGT" * 5)
                        out["k0_primers_txt"] = "\n".join(kept) + "\n"
                        out["k0_left_out"] = [p for p, q in zip(pats, kept) if p != q]
                    use = os.path.join(d, "k0.P")
                    with open(use, "w") as f:
                        f.write(out["k0_primers_txt"])
                if cname == "K2_five_class":
                    use = os.path.join(d, "zoned.P")
                    with open(use, "w") as f:
                        f.write(out["zoned_primers_txt"])
                r = subprocess.run([os.path.join(REF, "primer_match"), "-i", fa, "-P", use] + extra, capture_output=True)
                assert r.returncode == 0, (cname, r.stderr[-500:])
                text = r.stdout.decode("latin1")
                out["cases"].setdefault(cname, {"options": extra})[variant] = text
                if "-c" not in extra:                                  # the condition on every recorded run
                    ids = [int(ln.split()[0]) for ln in text.splitlines()]
                    own = sum(1 for i in ids if i in (zoned_ids if cname == "K2_five_class" else degenerate_ids))
                    assert len(ids) >= 30 and own >= 10, (cname, variant, len(ids), own)
    with open(os.path.join(HERE, "cli_wild.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("left out at k = 0:", out["k0_left_out"])
    print({k: len(v["normalized"].splitlines()) for k, v in out["cases"].items()}, sorted({len(p) for p in pats}))


if __name__ == "__main__":
    main()
