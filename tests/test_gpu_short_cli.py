"""GPU: pm_primer_match -k 2 -r with primers of 16..24 nt -- half of them shorter than 20 nt, the class that runs on
pm_short_edit_scan -- against the standard output of the real reference primer_match on the same database
and primer file (tests/golden/cli_short.json, recorded by tests/golden/make_cli_short_golden.py).  Byte for byte."""
import json
import os
import subprocess
import tempfile

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")
PM = os.path.join(HOST, "pm_primer_match")
CS = os.path.join(HOST, "pm_compress_seq")


def test_short_primers_output_equals_the_reference():
    assert os.path.exists(PM) and os.path.exists(CS), "run __graft_entry__.build()"
    with open(os.path.join(ROOT, "tests", "golden", "cli_short.json")) as f:
        g = json.load(f)
    lens = sorted(len(p) for p in g["primers_txt"].split())
    assert lens[0] == 16 and lens[-1] == 24 and sum(n < 20 for n in lens) >= 10
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
                assert sorted(got.splitlines()) == sorted(want.splitlines()), (case, variant)   # (the same lines ...)
                assert got == want, (case, variant)                                               # (... in the same order)
