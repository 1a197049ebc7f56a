#!/usr/bin/env python3
"""Generate tests/golden/pcr_dense.json from the REAL reference pcr_match (build container only).

Hit-dense input for the pairing stage: a tandem-repeat entry (100 copies of a 25 nt unit, one copy broken by an N run)
with a primer pair cut from the unit -- the two sites overlap each other and every copy is a hit of both primers, so one
pair has hundreds of hits and every hit several partners -- and a second pair with overlapping sites in a random entry.
Run through oracle/_ref/compress_seq -n true and oracle/_ref/pcr_match with -R 1, -R 50 and the default, -k 1 and -K 2,
-a and -b; inputs and standard output are stored.  Data only -- no reference source.  Re-run:
    make -C oracle ref && python tests/golden/make_pcr_dense_golden.py
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
FMT = "%i %r %>s %<e %>d %<d %l %N\\n"

CASES = [
    ("dense_k1_R1", ["-r", "-k", "1", "-M", "60", "-R", "1", "-A", FMT]),
    ("dense_K2_R50", ["-r", "-K", "2", "-M", "60", "-R", "50", "-A", FMT]),
    ("dense_k1_allorient", ["-r", "-a", "-k", "1", "-M", "60", "-A", FMT]),
    ("dense_K2_between_R50", ["-r", "-b", "-K", "2", "-m", "5", "-M", "40", "-R", "50", "-A", FMT]),
    ("dense_k1_between_allorient_R1", ["-r", "-a", "-b", "-k", "1", "-M", "20", "-R", "1", "-A", FMT]),
]


def build_inputs(seed):
    rng = np.random.default_rng(seed)
    rnd = lambda n: "".join(rng.choice(list("ACGT"), size=n).tolist())
    unit = rnd(25)
    copies = [unit] * 100
    copies[57] = unit[:11] + "NNNN" + unit[15:]
    e1 = rnd(60) + "".join(copies) + rnd(60)
    e2 = rnd(600)
    entries = [e1, e2]
    pairs = [(unit[0:18], synth.revcomp(unit[10:25] + unit[0:3])),       # the two sites share 8 bases
             (e2[100:120], synth.revcomp(e2[112:132]))]
    fasta = "".join(">rep%d entry %d\n%s" % (i + 1, i + 1, "".join(s[j:j + 70] + "\n" for j in range(0, len(s), 70)))
                    for i, s in enumerate(entries))
    return fasta, "".join("%s %s\n" % p for p in pairs)


def main():
    fasta, ptxt = build_inputs(31)
    out = {"fasta": fasta, "primers": {"P": ptxt}, "cases": {}}
    with tempfile.TemporaryDirectory() as d:
        fa = os.path.join(d, "db.fa")
        with open(fa, "w") as f:
            f.write(fasta)
        r = subprocess.run([os.path.join(REF, "compress_seq"), "-i", fa, "-n", "true"], capture_output=True)
        assert r.returncode == 0, r.stderr
        with open(os.path.join(d, "primers.P"), "w") as f:
            f.write(ptxt)
        for cname, extra in CASES:
            r = subprocess.run([os.path.join(REF, "pcr_match"), "-i", fa, "-P", os.path.join(d, "primers.P")] + extra, capture_output=True)
            assert r.returncode == 0, (cname, r.stderr[-500:])
            out["cases"][cname] = {"primers": "P", "options": extra, "stdout": r.stdout.decode("latin1")}
    with open(os.path.join(HERE, "pcr_dense.json"), "w") as f:
        json.dump(out, f, indent=1)
    print({k: len(v["stdout"].splitlines()) for k, v in out["cases"].items()})


if __name__ == "__main__":
    main()
