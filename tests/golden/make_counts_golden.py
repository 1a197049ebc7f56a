#!/usr/bin/env python3
"""Generate tests/golden/cli_counts_*.json from the REAL reference primer_match (build container only).

Hit-dense databases -- words of a small vocabulary, tandem repeats, an N run, primers cut from the text with 0 .. 2
edits, a duplicate primer, (AC) x 10 -- so that many primers have more hits than -M lets through.  Per option set the
file holds primer_match's standard output for -c, -c -a and -c -C fmt with and without -M, and the hit list the same
binary prints with -A '%i %r %E %d' (tests/test_counts_abi.py rebuilds the tallies from it with tests/count_rule.py).
Data only -- no reference source.  Re-run:
    make -C oracle ref && python tests/golden/make_counts_golden.py
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
TALLY_FMT = "%i %r %c [%C] %+\\n"
OPTSETS = [("k0", []), ("K1", ["-K", "1"]), ("K2", ["-K", "2"]), ("k1", ["-k", "1"]), ("k2", ["-k", "2"]), ("k2_5prime6", ["-k", "2", "-5", "6"]),
           ("k1_3prime4", ["-k", "1", "-3", "4"])]
CAPS = (0, 1, 3, 7)
FORMS = [("c", ["-c"]), ("ca", ["-c", "-a"]), ("C", ["-C", TALLY_FMT, "-c"])]


def build_inputs(seed):
    rng = np.random.default_rng(seed)
    letters = list("ACGT")
    words = ["".join(rng.choice(letters, size=12).tolist()) for _ in range(6)]
    ents = []
    for e in range(2):
        parts = []
        while sum(map(len, parts)) < 1200:
            r = rng.random()
            if r < 0.5:
                w = words[int(rng.integers(0, len(words)))]
                parts.append(synth.mutate(rng, w, nsub=1) if rng.random() < 0.3 else w)
            elif r < 0.7:
                parts.append("".join(rng.choice(letters, size=int(rng.integers(1, 7))).tolist()) * int(rng.integers(5, 30)))
            else:
                parts.append("".join(rng.choice(letters, size=int(rng.integers(5, 60))).tolist()))
        s = "".join(parts)
        if e == 1:
            s = s[:200] + "NNN" + s[203:]
        ents.append(s)
    pats = []
    for _ in range(24):
        L = int(rng.integers(20, 27))
        s = ents[int(rng.integers(0, len(ents)))]
        a = int(rng.integers(0, len(s) - L))
        w = s[a:a + L].replace("N", "A")
        kind = int(rng.integers(0, 5))
        w = synth.mutate(rng, w, nsub=int(kind == 1), nins=int(kind == 2), ndel=int(kind == 3))
        if kind == 4:
            w = synth.mutate(rng, w, nsub=2)
        pats.append(w)
    pats.append("ACACACACACACACACACAC")
    pats.append(pats[0])
    fasta = "".join(">e%d dense entry\n%s" % (i, "".join(s[j:j + 60] + "\n" for j in range(0, len(s), 60))) for i, s in enumerate(ents))
    sts = "".join("STS%d\t%s\t%s\t%d\tACC%d\t%d\tALT%d\tHomo sapiens\n" % (i, pats[i], pats[i + 1], 100 + i, i, i % 23 + 1, i) for i in range(0, len(pats) - 1, 2))
    widen = {"A": "RMWN", "C": "YMSN", "G": "RKSN", "T": "YKWN"}
    wpats = []
    for p in pats[:12]:
        w = list(p)
        for _ in range(int(rng.integers(1, 3))):
            i = int(rng.integers(0, len(w)))
            w[i] = str(rng.choice(list(widen.get(w[i], w[i]))))
        wpats.append("".join(w))
    wpats.append(ents[1][190:210])                                   # a site over the N run: matches only with -W
    return fasta, "\n".join(pats) + "\n", sts, "\n".join(wpats) + "\n"


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, check=False)
    assert r.returncode == 0, (cmd, r.stderr[-500:])
    return r.stdout.decode("latin1")


def main():
    for name, seed in (("cli_counts_a", 0), ("cli_counts_b", 1)):
        fasta, ptxt, psts, wtxt = build_inputs(seed)
        out = {"fasta": fasta, "primers_txt": ptxt, "primers_sts": psts, "primers_iupac": wtxt, "tally_format": TALLY_FMT, "cases": {}, "hits": {}}
        with tempfile.TemporaryDirectory() as d:
            dbs = {}
            for variant, args in (("normalized", ["-n", "true"]), ("indexed", []), ("compressed", ["-z", "true"])):
                os.mkdir(os.path.join(d, variant))
                dbs[variant] = os.path.join(d, variant, "db.fa")
                with open(dbs[variant], "w") as f:
                    f.write(fasta)
                run([os.path.join(REF, "compress_seq"), "-i", dbs[variant]] + args)
            for src, text in (("P", ptxt), ("S", psts), ("W", wtxt)):
                with open(os.path.join(d, "primers." + src), "w") as f:
                    f.write(text)
            pm = os.path.join(REF, "primer_match")

            def case(cname, src, options):
                """the same bytes on every database form, or the golden is not one"""
                parg = ["-" + ("P" if src == "W" else src), os.path.join(d, "primers." + src)]
                outs = [run([pm, "-i", dbs[v]] + parg + options) for v in ("normalized", "indexed", "compressed")]
                assert outs[0] == outs[1] == outs[2], cname
                out["cases"][cname] = {"primers": src, "options": options, "stdout": outs[0]}

            for oname, opts in OPTSETS:
                lines = run([pm, "-i", dbs["normalized"], "-P", os.path.join(d, "primers.P"), "-r", "-A", "%i %r %E %d\\n"] + opts)
                out["hits"][oname] = {"options": ["-r"] + opts, "k": int(opts[1]) if opts else 0,
                                      "records": [[int(i), r, int(e), int(dd)] for i, r, e, dd in (ln.split() for ln in lines.splitlines())]}
                for M in CAPS:
                    for fname, form in FORMS:
                        case("%s_M%d_%s" % (oname, M, fname), "P", ["-r"] + opts + form + (["-M", str(M)] if M else []))
            for M in (0, 3):
                cap = ["-M", str(M)] if M else []
                case("k1_sts_M%d" % M, "S", ["-k", "1", "-C", "%I %L %i %r %c\\n", "-c"] + cap)
                case("k0_W_M%d" % M, "W", ["-r", "-W", "-c"] + cap)
                case("K1_W_M%d" % M, "W", ["-r", "-W", "-K", "1", "-c", "-C", TALLY_FMT] + cap)
        with open(os.path.join(HERE, name + ".json"), "w") as f:
            json.dump(out, f, separators=(",", ":"))
        print(name, len(out["cases"]), "cases;", {k: len(v["records"]) for k, v in out["hits"].items()}, os.path.getsize(os.path.join(HERE, name + ".json")), "bytes")


if __name__ == "__main__":
    main()
