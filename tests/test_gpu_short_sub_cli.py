"""GPU: pm_primer_match -K 2 -r and pm_pcr_match -K 2 with primers of 16..24 nt -- half of them shorter than 20 nt, the
class that runs on pm_short_sub_scan beside the pair plan -- against the standard output of the real
reference primer_match and pcr_match on the same database and primer files (tests/golden/cli_short_K.json, recorded by
tests/golden/make_cli_short_K_golden.py)."""
import json
import os
import subprocess
import tempfile

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")
PM = os.path.join(HOST, "pm_primer_match")
PCR = os.path.join(HOST, "pm_pcr_match")
CS = os.path.join(HOST, "pm_compress_seq")


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "cli_short_K.json")) as f:
        return json.load(f)


def test_primer_match_output_equals_the_reference():
    """default output, one-line -A and -c, on a normalized and an indexed database; compared as sorted lines (the order of
    hits that end at one position -- a primer and its duplicate -- is engine specific)"""
    assert os.path.exists(PM) and os.path.exists(CS), "run __graft_entry__.build()"
    g = golden()
    lens = sorted(len(p) for p in g["primers_txt"].split())
    assert lens[0] == 16 and lens[-1] == 24 and sum(n < 20 for n in lens) >= 10 and sum(n >= 20 for n in lens) >= 10
    with tempfile.TemporaryDirectory() as d:
        pf = os.path.join(d, "primers.P")
        with open(pf, "w") as f:
            f.write(g["primers_txt"])
        for variant, args in (("normalized", ["-n", "true"]), ("indexed", [])):
            os.mkdir(os.path.join(d, variant))
            fa = os.path.join(d, variant, "db.fa")
            with open(fa, "w") as f:
                f.write(g["fasta"])
            r = subprocess.run([CS, "-i", fa] + args, capture_output=True)
            assert r.returncode == 0, r.stderr
            for case, c in g["cases"].items():
                r = subprocess.run([PM, "-i", fa, "-P", pf] + c["options"], capture_output=True, timeout=300)
                assert r.returncode == 0, (case, variant, r.stderr[-500:])
                got, want = r.stdout.decode("latin1"), c[variant]
                assert want.strip(), (case, variant)
                assert sorted(got.splitlines()) == sorted(want.splitlines()), (case, variant)
                assert len(got) == len(want), (case, variant)


def test_pcr_match_output_equals_the_reference():
    """primer pairs with one primer shorter than 20 nt each; compared as sorted lines (the order of hits that end at one
    position is engine specific)"""
    assert os.path.exists(PCR) and os.path.exists(CS), "run __graft_entry__.build()"
    g = golden()
    pairs = [ln.split() for ln in g["pairs_txt"].splitlines()]
    assert all(min(len(a), len(b)) < 20 <= max(len(a), len(b)) for a, b in pairs)
    with tempfile.TemporaryDirectory() as d:
        fa, qf = os.path.join(d, "db.fa"), os.path.join(d, "pairs.P")
        with open(fa, "w") as f:
            f.write(g["fasta"])
        with open(qf, "w") as f:
            f.write(g["pairs_txt"])
        r = subprocess.run([CS, "-i", fa, "-n", "true"], capture_output=True)
        assert r.returncode == 0, r.stderr
        for case, c in g["pcr_cases"].items():
            r = subprocess.run([PCR, "-i", fa, "-P", qf] + c["options"], capture_output=True, timeout=300)
            assert r.returncode == 0, (case, r.stderr[-500:])
            got = r.stdout.decode("latin1")
            assert c["stdout"].strip(), case
            assert sorted(got.splitlines()) == sorted(c["stdout"].splitlines()), case
            assert len(got) == len(c["stdout"])
