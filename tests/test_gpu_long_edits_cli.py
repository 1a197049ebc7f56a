"""GPU: pm_primer_match -k 2 -r, -k 1 -r and pm_pcr_match -k 1 with PM_GPU_LONG=4 and primers of 18..60 nt -- a third of them
of 33 nt or more, the primers that run on the edit plan's wide tiles under that permission -- against
the standard output of the real reference primer_match and pcr_match on the same database and primer files
(tests/golden/cli_long_edits.json, recorded by tests/golden/make_cli_long_edits_golden.py).  The -k 1 lines name the
engine (-N 5, filter_bitvec), in the reference's run and here: left to itself the choice for -k 1 on primers of 12 nt or
more is exact_halves, an option set the route does not apply to."""
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
ROUTE = b"[pm] long route:"                                         # PM_DEBUG: the handle took long primers onto the edit plan


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "cli_long_edits.json")) as f:
        return json.load(f)


def environment(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("PM_GPU_LONG", "PM_LONG_EDITS", "PM_DEBUG")}
    env.update(kw)
    return env


def test_primer_match_output_equals_the_reference():
    """default output, one-line -A and -c, on a normalized and an indexed database; compared as sorted lines (the order of
    hits that end at one position -- a primer and its duplicate -- is engine specific).  PM_DEBUG shows the route: taken
    with PM_GPU_LONG=4, not taken without it and not with PM_LONG_EDITS=off beside it; the output is the same on all three"""
    assert os.path.exists(PM) and os.path.exists(CS), "run __graft_entry__.build()"
    g = golden()
    lens = sorted(len(p) for p in g["primers_txt"].split())
    assert lens[0] == 18 and lens[-1] == 60 and sum(n >= 33 for n in lens) >= 10 and sum(20 <= n <= 32 for n in lens) >= 10 and sum(n < 20 for n in lens) >= 10
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
                want = c[variant]
                assert want.strip(), (case, variant)
                routes = [(environment(PM_GPU_LONG="4", PM_DEBUG="1"), True)]
                if case in ("k2_default", "k1_default"):
                    routes += [(environment(PM_DEBUG="1"), False), (environment(PM_GPU_LONG="4", PM_LONG_EDITS="off", PM_DEBUG="1"), False)]
                for env, taken in routes:
                    r = subprocess.run([PM, "-i", fa, "-P", pf] + c["options"], capture_output=True, timeout=300, env=env)
                    assert r.returncode == 0, (case, variant, r.stderr[-500:])
                    assert (ROUTE in r.stderr) == taken, (case, variant, taken, r.stderr[-1500:])
                    got = r.stdout.decode("latin1")
                    assert sorted(got.splitlines()) == sorted(want.splitlines()), (case, variant, taken)
                    assert len(got) == len(want), (case, variant)


def test_pcr_match_output_equals_the_reference():
    """primer pairs with one primer of 33 nt or more each; compared as sorted lines (the order of hits that end at one
    position is engine specific)"""
    assert os.path.exists(PCR) and os.path.exists(CS), "run __graft_entry__.build()"
    g = golden()
    pairs = [ln.split() for ln in g["pairs_txt"].splitlines()]
    assert all(min(len(a), len(b)) < 33 <= max(len(a), len(b)) <= 60 for a, b in pairs)
    with tempfile.TemporaryDirectory() as d:
        fa, qf = os.path.join(d, "db.fa"), os.path.join(d, "pairs.P")
        with open(fa, "w") as f:
            f.write(g["fasta"])
        with open(qf, "w") as f:
            f.write(g["pairs_txt"])
        r = subprocess.run([CS, "-i", fa, "-n", "true"], capture_output=True)
        assert r.returncode == 0, r.stderr
        for case, c in g["pcr_cases"].items():
            routes = [(environment(PM_GPU_LONG="4", PM_DEBUG="1"), True)]
            if case == "pcr_k1_default":
                routes += [(environment(PM_DEBUG="1"), False), (environment(PM_GPU_LONG="4", PM_LONG_EDITS="off", PM_DEBUG="1"), False)]
            for env, taken in routes:
                r = subprocess.run([PCR, "-i", fa, "-P", qf] + c["options"], capture_output=True, timeout=300, env=env)
                assert r.returncode == 0, (case, r.stderr[-500:])
                assert (ROUTE in r.stderr) == taken, (case, taken, r.stderr[-1500:])
                got = r.stdout.decode("latin1")
                assert c["stdout"].strip(), case
                assert sorted(got.splitlines()) == sorted(c["stdout"].splitlines()), (case, taken)
                assert len(got) == len(c["stdout"])
