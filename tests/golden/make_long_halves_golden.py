#!/usr/bin/env python3
"""Generate tests/golden/long_halves_ref.json.gz and tests/golden/cli_long_halves.json from the REAL reference (build
container only).  Data only -- no reference source.

long_halves_ref.json.gz (gzip: tests/test_oracle_golden.py, test_gpu_parity.py and test_gpu_windowed.py take every plain
*.json here that is no cli_ or pcr_ file as a case of their own format), from oracle/_ref/ref_harness (the engines at the find_patterns boundary): the hits of a 33-, a 40-
and a 64-mer on the stream of all their one-edit texts under `-k 1` (automatic choice: exact_halves, select.cc:121-126),
and of a mixed list of 20..64 nt primers on a 4,000-base stream under `-k 2 -N 11` (exact_halves asked for by name).
tests/test_long_halves_ref.py pins the oracle to these before anything is compared with it at these lengths.

cli_long_halves.json, from the real command lines: a seeded FASTA database, a primer file whose primers are 20..60 nt
long -- most of them windows of the database with up to two edits, a third of them of 33 nt or more (the primers that stay
on the halves plan where bit 3 of pm_config.long_patterns allows it) -- and a file of primer pairs with
planted amplicons, one primer of every pair of 33 nt or more, go through oracle/_ref/compress_seq,
oracle/_ref/primer_match -k 1 -r and oracle/_ref/pcr_match -k 1, engine left to the automatic choice: exact_halves.
Stored: the inputs and the standard output per option set and database form.  Re-run:
    make -C oracle ref && python tests/golden/make_long_halves_golden.py
"""
import gzip
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
TABLE = b"ACGT\n"
ONE_LINE = "%i %r %s %e %5 %3 %S %E %d %l %D %p %q %Q %t %T %U %A [%h|%H|%f] %| %^ %v %* %+ %%\\n"
PCR_LINE = "%i %r%R [%>s %>e %>S %>E %>d %>p %>q %>Q %>A] [%<s %<e %<S %<E %<d %<p %<q %<Q %<A] %l %>l %<l %%\\n"
CASES = [
    ("k1_default", ["-r", "-k", "1"]),
    ("k1_oneline", ["-r", "-k", "1", "-A", ONE_LINE]),
    ("k1_counts", ["-r", "-k", "1", "-c"]),
]
PCR_CASES = [
    ("pcr_k1_default", ["-r", "-k", "1"]),
    ("pcr_k1_oneline", ["-r", "-k", "1", "-A", PCR_LINE]),
]


def one_edit(w):
    out = set()
    for i in range(len(w)):
        out.add(w[:i] + w[i + 1:])
        for c in "ACGT":
            if c != w[i]:
                out.add(w[:i] + c + w[i + 1:])
    for i in range(len(w) + 1):
        for c in "ACGT":
            out.add(w[:i] + c + w[i:])
    return out


def harness(codes, table, pats, args):
    """(end, id, value) triples of oracle/_ref/ref_harness on a normalized stream, sorted"""
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "db.sqn"), "wb") as f:
            f.write(bytes(codes))
        with open(os.path.join(d, "db.tbl"), "wb") as f:
            f.write(bytes(table))
        with open(os.path.join(d, "pat.txt"), "w") as f:
            f.write("\n".join(pats) + "\n")
        r = subprocess.run([os.path.join(REF, "ref_harness"), "-m", "1000", "-n", "-i", os.path.join(d, "db"), "-P", os.path.join(d, "pat.txt")] + args,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-500:]
        return sorted([int(x) for x in ln.split()] for ln in r.stdout.splitlines() if ln.strip() and not ln.startswith("#"))


def engine_level():
    rng = np.random.default_rng(41)
    out = {"table": TABLE.decode(), "one_edit": [], "mixed": None}
    for L in (33, 40, 64):
        p = "".join(rng.choice(list("ACGT"), size=L).tolist())
        parts = ["".join(rng.choice(list("ACGT"), size=3).tolist()) + v + "".join(rng.choice(list("ACGT"), size=2).tolist()) for v in sorted(one_edit(p))]
        raw = synth.stream(parts)
        hits = harness(synth.normalize(raw, TABLE), TABLE, [p], ["-k", "1"])
        out["one_edit"].append({"pattern": p, "texts": len(parts), "stream": raw.decode(), "args": ["-k", "1"], "hits": hits})
    ents = synth.make_entries(rng, 2, 2000)
    pats = []
    for L in (20, 24, 28, 31, 32, 33, 34, 40, 47, 53, 63, 64) * 3:
        e = ents[int(rng.integers(0, 2))]
        a = int(rng.integers(0, len(e) - L - 2))
        w = "".join(synth.mutate(rng, e[a:a + L + 2], nsub=int(rng.integers(0, 2)), nins=int(rng.integers(0, 2)), ndel=int(rng.integers(0, 2))))[:L]
        if len(w) == L:
            pats.append(w)
    raw = synth.stream(ents)
    assert 4000 <= len(raw) <= 4100
    hits = harness(synth.normalize(raw, TABLE), TABLE, pats, ["-k", "2", "-N", "11"])
    out["mixed"] = {"patterns": pats, "stream": raw.decode(), "args": ["-k", "2", "-N", "11"], "hits": hits}
    with gzip.GzipFile(os.path.join(HERE, "long_halves_ref.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print([(len(c["pattern"]), c["texts"], len(c["hits"])) for c in out["one_edit"]], len(pats), len(hits))


def build_inputs(seed):
    rng = np.random.default_rng(seed)
    ents = synth.make_entries(rng, 4, 900, n_runs=2, repeats=True, short=True)
    fasta = "".join(">entry%d synthetic len=%d\n%s" % (i + 1, len(s), "".join(s[j:j + 60] + "\n" for j in range(0, len(s), 60))) for i, s in enumerate(ents))
    pats = []
    while len(pats) < 30:
        L = (int(rng.integers(33, 61)), int(rng.integers(20, 33)), int(rng.integers(20, 33)))[len(pats) % 3]
        e = int(rng.integers(0, 4))
        a = int(rng.integers(0, len(ents[e]) - L))
        w = ents[e][a:a + L]
        if "N" in w:
            continue
        w = synth.mutate(rng, w, nsub=int(rng.integers(0, 2)), nins=int(rng.integers(0, 2) and len(pats) % 2), ndel=int(rng.integers(0, 2) and not len(pats) % 2))   # up to two edits: some primers have no hit
        if not 20 <= len(w) <= 60:
            continue
        pats.append(synth.revcomp(w) if int(rng.integers(0, 2)) else w)
    pats.append(ents[0][:33])                                          # the first and the last bases of an entry
    pats.append(ents[1][-60:])
    pats.append(ents[2][:20])
    pats.append("".join(rng.choice(list("ACGT"), size=40).tolist()))  # no hit
    pats.append(pats[0])                                               # duplicate primer
    pats.append("AC" * 18)                                             # tandem repeat, 36 nt
    pairs = []
    while len(pairs) < 8:
        e = int(rng.integers(0, 4))
        Lf, Lr = (int(rng.integers(33, 61)), int(rng.integers(20, 33))) if len(pairs) % 2 == 0 else (int(rng.integers(20, 33)), int(rng.integers(33, 61)))
        amp = int(rng.integers(120, 500))
        a = int(rng.integers(0, len(ents[e]) - amp))
        fwd, rev_site = ents[e][a:a + Lf], ents[e][a + amp - Lr:a + amp]
        if "N" in fwd or "N" in rev_site:
            continue
        f = synth.mutate(rng, fwd, nsub=int(rng.integers(0, 2)))
        r = synth.mutate(rng, rev_site, nins=int(rng.integers(0, 2))) if len(pairs) % 2 else synth.mutate(rng, rev_site, ndel=int(rng.integers(0, 2)))
        if not (20 <= min(len(f), len(r)) < 33 <= max(len(f), len(r)) <= 60):
            continue
        pairs.append((synth.revcomp(r), f) if len(pairs) % 3 == 2 else (f, synth.revcomp(r)))   # (every third: the amplicon on the minus strand)
    return fasta, "\n".join(pats) + "\n", pats, "".join("%s %s\n" % p for p in pairs)


def cli_level():
    fasta, ptxt, pats, pairs_txt = build_inputs(37)
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
    with open(os.path.join(HERE, "cli_long_halves.json"), "w") as f:
        json.dump(out, f, indent=1)
    print({k: len(v["normalized"].splitlines()) for k, v in out["cases"].items()}, {k: len(v["stdout"].splitlines()) for k, v in out["pcr_cases"].items()},
          sorted({len(p) for p in pats}))


if __name__ == "__main__":
    engine_level()
    cli_level()
