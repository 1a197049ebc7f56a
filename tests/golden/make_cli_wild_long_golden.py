#!/usr/bin/env python3
"""Generate tests/golden/cli_wild_long.json from the REAL reference command lines (build container only).

A seeded FASTA database of 120 kbp with planted sites and a primer file of 14 fusion primers of 45..60 nt -- a plain
adapter in front of a degenerate locus-specific part: 806R (GGACTACNVGGGTWTCTAAT), mlCOIintF
(GGWACWGGWTGAACWGTWTAYCCYCC), 515F-Y (GTGYCAGCMGCCGCGGTAA, two letters: no class primer) and eleven windows of the database
with 3..5 ambiguity letters in their last 20 characters -- beside eight plain primers of 20..24 nt, go through
oracle/_ref/compress_seq and oracle/_ref/primer_match -w -r at k = 0, -K 1 -N 5, -K 2 and -K 2 -c.  The long degenerate
primers are the ones that run on pm_wild_sub_scan + pm_wild_sub_verify_wide under PM_GPU_LONG=160.
At k = 0 the reference's own primer_match ends with "Bogus hit returned to primer_match main()" for some degenerate primers
(DESIGN.md 4.13): every primer is run alone there first, and one the reference fails on is replaced in the k = 0 primer
file by a placeholder without a hit (k0_left_out names them; the primer indices stay the same in every run).
Every recorded run must hold hits of at least eight of the long degenerate primers: checked here, and again by the test.
Stored: the inputs and the standard output per option set and database form ("indexed": null where the indexed form gives
the bytes of the normalized one: they are stored once).  Data only -- no reference source.  Re-run:
    make -C oracle ref && python tests/golden/make_cli_wild_long_golden.py
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
    ("K2_counts", ["-w", "-r", "-K", "2", "-c"]),
]
CLASS = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "K": "GT", "M": "AC", "S": "CG", "W": "AT",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
NAMED = ["GGACTACNVGGGTWTCTAAT", "GGWACWGGWTGAACWGTWTAYCCYCC", "GTGYCAGCMGCCGCGGTAA"]   # 806R, mlCOIintF, 515F-Y


def class_primer(p):
    """the routing rule of DESIGN.md 4.14 at -K 2, restated: 33..64 characters, more than 16 concrete variants, at most 256
    keys in every pair of the four fields of the last 16 characters"""
    n = 1
    for ch in p:
        n *= len(CLASS[ch])
    keys = [1, 1, 1, 1]
    for f in range(4):
        for ch in p[len(p) - 16 + 4 * f:len(p) - 12 + 4 * f]:
            keys[f] *= len(CLASS[ch])
    return 33 <= len(p) <= 64 and n > 16 and all(keys[a] * keys[b] <= 256 for a in range(4) for b in range(a + 1, 4))


def concrete(rng, p):
    return "".join(str(rng.choice(list(CLASS[ch]))) for ch in p)


def build_inputs(seed):
    rng = np.random.default_rng(seed)
    ents = [list(s) for s in synth.make_entries(rng, 4, 30000)]
    rand = lambda n: "".join(rng.choice(list("ACGT"), size=n).tolist())
    fusion = []
    for i, tail in enumerate(NAMED):                                   # adapter + published primer: 45..60 nt
        fusion.append(rand(52 - len(tail) + 4 * i) + tail)
    while len(fusion) < 14:                                            # windows of the database, 3..5 letters (no N) in the last 20 characters
        L = int(rng.integers(45, 61))
        e = int(rng.integers(0, 4))
        a = int(rng.integers(0, len(ents[e]) - L))
        w = list("".join(ents[e][a:a + L]))
        for i in rng.choice(20, size=int(rng.integers(3, 6)), replace=False).tolist():
            j = L - 20 + i
            w[j] = str(rng.choice([c for c in "RYKMSWBDHV" if w[j] in CLASS[c]]))
        if class_primer("".join(w)):
            fusion.append("".join(w))
    at = 700
    for n, p in enumerate(fusion):                                     # planted sites of every fusion primer: 0, 1 and 2 substitutions, both strands
        for r in range(6):
            site = synth.mutate(rng, concrete(rng, p), nsub=r % 3)
            if r % 2:
                site = synth.revcomp(site)
            e = (n + r) % 4
            ents[e][at:at + len(site)] = list(site)
            at = 700 + (at + 1000 - 700) % 28000
    ents = ["".join(s) for s in ents]
    plain = []
    while len(plain) < 8:
        L = int(rng.integers(20, 25))
        e = int(rng.integers(0, 4))
        a = int(rng.integers(0, len(ents[e]) - L))
        w = synth.mutate(rng, ents[e][a:a + L], nsub=int(rng.integers(0, 5)) // 2)
        plain.append(synth.revcomp(w) if int(rng.integers(0, 2)) else w)
    pats = []
    for i in range(14):
        pats.append(fusion[i])
        if i < 8:
            pats.append(plain[i])
    fasta = "".join(">entry%d synthetic len=%d\n%s" % (i + 1, len(s), "".join(s[j:j + 60] + "\n" for j in range(0, len(s), 60))) for i, s in enumerate(ents))
    return fasta, "\n".join(pats) + "\n", pats, [i + 1 for i, p in enumerate(pats) if class_primer(p)]


def main():
    fasta, ptxt, pats, class_ids = build_inputs(53)
    assert len(class_ids) >= 12, class_ids
    out = {"fasta": fasta, "primers_txt": ptxt, "class_ids": class_ids, "cases": {}}
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
                r = subprocess.run([os.path.join(REF, "primer_match"), "-i", fa, "-P", use] + extra, capture_output=True)
                assert r.returncode == 0, (cname, r.stderr[-500:])
                text = r.stdout.decode("latin1")
                out["cases"].setdefault(cname, {"options": extra})[variant] = text
                if "-c" not in extra:                                  # the condition on every recorded run
                    ids = {int(ln.split()[0]) for ln in text.splitlines()}
                    left = {i + 1 for i, p in enumerate(pats) if cname == "k0" and p in out["k0_left_out"]}
                    own = ids & (set(class_ids) - left)
                    assert len(own) >= 8, (cname, variant, sorted(own))
    for c in out["cases"].values():                                    # the same bytes on both database forms: stored once
        if c["indexed"] == c["normalized"]:
            c["indexed"] = None
    with open(os.path.join(HERE, "cli_wild_long.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("left out at k = 0:", out["k0_left_out"])
    print({k: (len(v["normalized"].splitlines()), v["indexed"] is None) for k, v in out["cases"].items()}, sorted({len(p) for p in pats}), class_ids)


if __name__ == "__main__":
    main()
