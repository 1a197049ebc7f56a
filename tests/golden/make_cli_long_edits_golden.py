#!/usr/bin/env python3
"""Generate tests/golden/cli_long_edits.json from the REAL reference command lines (build container only).

A seeded FASTA database, a primer file whose primers are 18..60 nt long -- most of them windows of the database with up
to three edits (substitutions, insertions, deletions), a third of them of 33 nt or more (the primers that run on the
edit plan's wide tiles where bit 2 of pm_config.long_patterns allows it), some of 18 and 19 nt -- and a
file of primer pairs with planted amplicons, one primer of every pair of 33 nt or more, go through
oracle/_ref/compress_seq, oracle/_ref/primer_match -k 2 -r, -k 1 -r and oracle/_ref/pcr_match -k 1.  The -k 1 lines
name the engine (-N 5, filter_bitvec): left to itself the reference takes exact_halves for -k 1 on primers of 12 nt or
more (select.cc:121-126), an option set the long route does not apply to.  Stored: the inputs and the standard output
per option set and database form.  Data only -- no reference source.  Re-run:
    make -C oracle ref && python tests/golden/make_cli_long_edits_golden.py
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
ONE_LINE = "%i %r %s %e %5 %3 %S %E %d %l %D %p %q %Q %t %T %U %A [%h|%H|%f] %| %^ %v %* %+ %%\\n"
PCR_LINE = "%i %r%R [%>s %>e %>S %>E %>d %>p %>q %>Q %>A] [%<s %<e %<S %<E %<d %<p %<q %<Q %<A] %l %>l %<l %%\\n"
CASES = [
    ("k2_default", ["-r", "-k", "2"]),
    ("k2_oneline", ["-r", "-k", "2", "-A", ONE_LINE]),
    ("k2_counts", ["-r", "-k", "2", "-c"]),
    ("k1_default", ["-r", "-k", "1", "-N", "5"]),
    ("k1_oneline", ["-r", "-k", "1", "-N", "5", "-A", ONE_LINE]),
]
PCR_CASES = [
    ("pcr_k1_default", ["-r", "-k", "1", "-N", "5"]),
    ("pcr_k1_oneline", ["-r", "-k", "1", "-N", "5", "-A", PCR_LINE]),
]


def build_inputs(seed):
    rng = np.random.default_rng(seed)
    ents = synth.make_entries(rng, 4, 900, n_runs=2, repeats=True, short=True)
    fasta = "".join(">entry%d synthetic len=%d\n%s" % (i + 1, len(s), "".join(s[j:j + 60] + "\n" for j in range(0, len(s), 60))) for i, s in enumerate(ents))
    pats = []
    while len(pats) < 30:
        L = (int(rng.integers(33, 61)), int(rng.integers(20, 33)), int(rng.integers(18, 20)))[len(pats) % 3]
        e = int(rng.integers(0, 4))
        a = int(rng.integers(0, len(ents[e]) - L))
        w = ents[e][a:a + L]
        if "N" in w:
            continue
        w = synth.mutate(rng, w, nsub=int(rng.integers(0, 2)), nins=int(rng.integers(0, 2)), ndel=int(rng.integers(0, 2)))   # up to three edits: some primers have no hit
        if not 18 <= len(w) <= 60:
            continue
        pats.append(synth.revcomp(w) if int(rng.integers(0, 2)) else w)
    pats.append(ents[0][:33])                                          # the first and the last bases of an entry
    pats.append(ents[1][-60:])
    pats.append(ents[2][:18])
    pats.append("".join(rng.choice(list("ACGT"), size=40).tolist()))  # no hit
    pats.append(pats[0])                                               # duplicate primer
    pats.append("AC" * 18)                                             # tandem repeat, 36 nt
    pairs = []
    while len(pairs) < 8:
        e = int(rng.integers(0, 4))
        Lf, Lr = (int(rng.integers(33, 61)), int(rng.integers(18, 33))) if len(pairs) % 2 == 0 else (int(rng.integers(18, 33)), int(rng.integers(33, 61)))
        amp = int(rng.integers(120, 500))
        a = int(rng.integers(0, len(ents[e]) - amp))
        fwd, rev_site = ents[e][a:a + Lf], ents[e][a + amp - Lr:a + amp]
        if "N" in fwd or "N" in rev_site:
            continue
        f = synth.mutate(rng, fwd, nsub=int(rng.integers(0, 2)))
        r = synth.mutate(rng, rev_site, nins=int(rng.integers(0, 2))) if len(pairs) % 2 else synth.mutate(rng, rev_site, ndel=int(rng.integers(0, 2)))
        if not (18 <= min(len(f), len(r)) < 33 <= max(len(f), len(r)) <= 60):
            continue
        pairs.append((synth.revcomp(r), f) if len(pairs) % 3 == 2 else (f, synth.revcomp(r)))   # (every third: the amplicon on the minus strand)
    return fasta, "\n".join(pats) + "\n", pats, "".join("%s %s\n" % p for p in pairs)


def main():
    fasta, ptxt, pats, pairs_txt = build_inputs(31)
    out = {"fasta": fasta, "primers_txt": ptxt, "pairs_txt": pairs_txt, "cases": {}, "pcr_cases": {}}
    with tempfile.TemporaryDirectory() as d:
        pf, qf = os.path.join(d, "primers.P"), os.path.join(d, "pairs.P")
        with open(pf, "w") as f:
            f.write(ptxt)
        with open(qf, "w") as f:
            f.write(pairs_txt)
        for variant, args in (("normalized", ["-n", "true"]), ("indexed", [])):
            os.mkdir(os.path.join(d, variant))
            fa = os.path.join(d, variant, "db.fa")
            with open(fa, "w") as f:
                f.write(fasta)
            r = subprocess.run([os.path.join(REF, "compress_seq"), "-i", fa] + args, capture_output=True)
            assert r.returncode == 0, r.stderr
            for cname, extra in CASES:
                r = subprocess.run([os.path.join(REF, "primer_match"), "-i", fa, "-P", pf] + extra, capture_output=True)
                assert r.returncode == 0, (cname, r.stderr[-500:])
                out["cases"].setdefault(cname, {"options": extra})[variant] = r.stdout.decode("latin1")
            if variant == "normalized":
                for cname, extra in PCR_CASES:
                    r = subprocess.run([os.path.join(REF, "pcr_match"), "-i", fa, "-P", qf] + extra, capture_output=True)
                    assert r.returncode == 0, (cname, r.stderr[-500:])
                    out["pcr_cases"][cname] = {"options": extra, "stdout": r.stdout.decode("latin1")}
    with open(os.path.join(HERE, "cli_long_edits.json"), "w") as f:
        json.dump(out, f, indent=1)
    print({k: len(v["normalized"].splitlines()) for k, v in out["cases"].items()}, {k: len(v["stdout"].splitlines()) for k, v in out["pcr_cases"].items()},
          sorted({len(p) for p in pats}))


if __name__ == "__main__":
    main()
