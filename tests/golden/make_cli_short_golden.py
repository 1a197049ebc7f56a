#!/usr/bin/env python3
"""Generate tests/golden/cli_short.json from the REAL reference command lines (build container only).

A seeded FASTA database and a primer file whose primers are 16..24 nt long -- most of them windows of the database with
up to two edits, half of them shorter than 20 nt (the class pm_short_edit_scan takes) -- go through
oracle/_ref/compress_seq and oracle/_ref/primer_match -k 2 -r.  Stored: the inputs and primer_match's standard output per
option set and database form.  Data only -- no reference source.  Re-run:
    make -C oracle ref && python tests/golden/make_cli_short_golden.py
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
CASES = [
    ("k2_default", ["-r", "-k", "2"]),
    ("k2_oneline", ["-r", "-k", "2", "-A", ONE_LINE]),
    ("k2_counts", ["-r", "-k", "2", "-c"]),
]


def build_inputs(seed):
    rng = np.random.default_rng(seed)
    ents = synth.make_entries(rng, 4, 900, n_runs=2, repeats=True, short=True)
    fasta = "".join(">entry%d synthetic len=%d\n%s" % (i + 1, len(s), "".join(s[j:j + 60] + "\n" for j in range(0, len(s), 60))) for i, s in enumerate(ents))
    pats = []
    while len(pats) < 28:
        L = int(rng.integers(16, 20)) if len(pats) % 2 == 0 else int(rng.integers(20, 25))
        e = int(rng.integers(0, 4))
        a = int(rng.integers(0, len(ents[e]) - L))
        w = ents[e][a:a + L]
        if "N" in w:
            continue
        kind = int(rng.integers(0, 7))
        w = synth.mutate(rng, w, nsub=(kind == 1) + 2 * (kind == 2), nins=int(kind in (3, 5)), ndel=int(kind in (4, 5)))
        if kind == 6:                                                 # an edit at either end
            w = w[1:] if int(rng.integers(0, 2)) else w[:-1] + "ACGT"[("ACGT".index(w[-1]) + 1) % 4]
        if not 16 <= len(w) <= 24:
            continue
        pats.append(synth.revcomp(w) if int(rng.integers(0, 2)) else w)
    pats.append(ents[0][:17])                                          # the first and the last bases of an entry
    pats.append(ents[1][-18:])
    pats.append("".join(rng.choice(list("ACGT"), size=18).tolist()))  # no hit
    pats.append(pats[0])                                               # duplicate primer
    pats.append("ACACACACACACACACAC")                                   # tandem repeat, 18 nt
    return fasta, "\n".join(pats) + "\n", pats


def main():
    fasta, ptxt, pats = build_inputs(21)
    out = {"fasta": fasta, "primers_txt": ptxt, "cases": {}}
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
                r = subprocess.run([os.path.join(REF, "primer_match"), "-i", fa, "-P", pf] + extra, capture_output=True)
                assert r.returncode == 0, (cname, r.stderr[-500:])
                out["cases"].setdefault(cname, {"options": extra})[variant] = r.stdout.decode("latin1")
    with open(os.path.join(HERE, "cli_short.json"), "w") as f:
        json.dump(out, f, indent=1)
    print({k: len(v["normalized"].splitlines()) for k, v in out["cases"].items()}, sorted({len(p) for p in pats}))


if __name__ == "__main__":
    main()
