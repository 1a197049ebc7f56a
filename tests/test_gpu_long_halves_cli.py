"""GPU: pm_primer_match -k 1 -r and pm_pcr_match -k 1 with PM_GPU_LONG=8 and primers of 20..60 nt -- a third of them of 33 nt
or more, the primers that keep the list on the halves plan under that permission -- against the standard
output of the real reference primer_match and pcr_match on the same database and primer files
(tests/golden/cli_long_halves.json, recorded by tests/golden/make_long_halves_golden.py).  No engine is named, in the
reference's run or here: for -k 1 on primers of 12 nt or more the automatic choice is exact_halves."""
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
ROUTE = b"[pm] long route:"                                         # PM_DEBUG: the handle kept long primers on the halves plan
PLAN = b"on the halves plan"


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "cli_long_halves.json")) as f:
        return json.load(f)


def environment(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("PM_GPU_LONG", "PM_LONG_HALVES", "PM_HALF_SCAN", "PM_DEBUG")}
    env.update(kw)
    return env


def routes(first):
    """the route is taken with PM_GPU_LONG=8 (and in a sum), not taken without the variable, with the other three bits and
    with PM_LONG_HALVES=off beside it"""
    r = [(environment(PM_GPU_LONG="8", PM_DEBUG="1"), True)]
    if first:
        r += [(environment(PM_DEBUG="1"), False), (environment(PM_GPU_LONG="8", PM_LONG_HALVES="off", PM_DEBUG="1"), False),
              (environment(PM_GPU_LONG="7", PM_DEBUG="1"), False), (environment(PM_GPU_LONG="15", PM_DEBUG="1"), True)]
    return r


def test_primer_match_output_equals_the_reference():
    """default output, one-line -A and -c, on a normalized and an indexed database; compared as sorted lines (the order of
    hits that end at one position -- a primer and its duplicate -- is engine specific); the output is the same on every
    route"""
    assert os.path.exists(PM) and os.path.exists(CS), "run __graft_entry__.build()"
    g = golden()
    lens = sorted(len(p) for p in g["primers_txt"].split())
    assert lens[0] == 20 and lens[-1] == 60 and sum(n >= 33 for n in lens) >= 12 and sum(20 <= n <= 32 for n in lens) >= 12
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
                for env, taken in routes(case == "k1_default"):
                    r = subprocess.run([PM, "-i", fa, "-P", pf] + c["options"], capture_output=True, timeout=300, env=env)
                    assert r.returncode == 0, (case, variant, r.stderr[-500:])
                    assert (ROUTE in r.stderr) == taken and (PLAN in r.stderr) == taken, (case, variant, taken, r.stderr[-1500:])
                    got = r.stdout.decode("latin1")
                    assert sorted(got.splitlines()) == sorted(want.splitlines()), (case, variant, taken)
                    assert len(got) == len(want), (case, variant)


def test_pcr_match_output_equals_the_reference():
    """primer pairs with one primer of 33 nt or more each; compared as sorted lines (the order of hits that end at one
    position is engine specific)"""
    assert os.path.exists(PCR) and os.path.exists(CS), "run __graft_entry__.build()"
    g = golden()
    pairs = [ln.split() for ln in g["pairs_txt"].splitlines()]
    assert all(20 <= min(len(a), len(b)) < 33 <= max(len(a), len(b)) <= 60 for a, b in pairs)
    with tempfile.TemporaryDirectory() as d:
        fa, qf = os.path.join(d, "db.fa"), os.path.join(d, "pairs.P")
        with open(fa, "w") as f:
            f.write(g["fasta"])
        with open(qf, "w") as f:
            f.write(g["pairs_txt"])
        r = subprocess.run([CS, "-i", fa, "-n", "true"], capture_output=True)
        assert r.returncode == 0, r.stderr
        for case, c in g["pcr_cases"].items():
            for env, taken in routes(case == "pcr_k1_default"):
                r = subprocess.run([PCR, "-i", fa, "-P", qf] + c["options"], capture_output=True, timeout=300, env=env)
                assert r.returncode == 0, (case, r.stderr[-500:])
                assert (ROUTE in r.stderr) == taken and (PLAN in r.stderr) == taken, (case, taken, r.stderr[-1500:])
                got = r.stdout.decode("latin1")
                assert c["stdout"].strip(), case
                assert sorted(got.splitlines()) == sorted(c["stdout"].splitlines()), (case, taken)
                assert len(got) == len(c["stdout"])
