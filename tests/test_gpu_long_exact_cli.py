"""GPU: pm_primer_match -r and pm_pcr_match -r (no -k / -K: the exact engines) with PM_GPU_LONG=2 and primers of 12..60
nt -- a third of them of 33 nt or more, the primers that run on the seed plan's wide tiles under that permission
 -- against the standard output of the real reference primer_match and pcr_match on the same database
and primer files (tests/golden/cli_long_exact.json, recorded by tests/golden/make_cli_long_exact_golden.py)."""
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
ROUTE = b"[pm] long route:"                                         # PM_DEBUG: the handle took long primers into its main class


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "cli_long_exact.json")) as f:
        return json.load(f)


def environment(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("PM_GPU_LONG", "PM_LONG_EXACT", "PM_LONG_SUB", "PM_DEBUG")}
    env.update(kw)
    return env


# the three routes: the permission given, not given, and given with the knob that overrides it; VALUES: PM_GPU_LONG as
# bit 1 beside bit 0, and bit 0 alone ("1" keeps its meaning)
ROUTES = [(dict(PM_GPU_LONG="2"), True), (dict(), False), (dict(PM_GPU_LONG="2", PM_LONG_EXACT="off"), False)]
VALUES = [(dict(PM_GPU_LONG="3"), True), (dict(PM_GPU_LONG="1"), False)]


@pytest.mark.parametrize("variant,args", [("normalized", ["-n", "true"]), ("indexed", [])], ids=["normalized", "indexed"])
@pytest.mark.parametrize("case", ["k0_default", "k0_oneline", "k0_counts"])
def test_primer_match_output_equals_the_reference(case, variant, args):
    """default output, one-line -A and -c, on a normalized and an indexed database; compared as sorted lines (the order of
    hits that end at one position -- a primer and its duplicate -- is engine specific).  PM_DEBUG shows the route; the
    output is the same on all of them"""
    assert os.path.exists(PM) and os.path.exists(CS), "run __graft_entry__.build()"
    g = golden()
    lens = sorted(len(p) for p in g["primers_txt"].split())
    assert lens[0] == 12 and lens[-1] == 60 and sum(n >= 33 for n in lens) * 3 >= len(lens) and sum(20 <= n <= 32 for n in lens) >= 10 and sum(n < 20 for n in lens) >= 10
    c = g["cases"][case]
    want = c[variant]
    assert want.strip(), (case, variant)
    with tempfile.TemporaryDirectory() as d:
        pf, fa = os.path.join(d, "primers.P"), os.path.join(d, "db.fa")
        with open(pf, "w") as f:
            f.write(g["primers_txt"])
        with open(fa, "w") as f:
            f.write(g["fasta"])
        r = subprocess.run([CS, "-i", fa] + args, capture_output=True)
        assert r.returncode == 0, r.stderr
        for extra, taken in ROUTES + (VALUES if (case, variant) == ("k0_default", "normalized") else []):
            r = subprocess.run([PM, "-i", fa, "-P", pf] + c["options"], capture_output=True, timeout=300, env=environment(PM_DEBUG="1", **extra))
            assert r.returncode == 0, (case, variant, r.stderr[-500:])
            assert (ROUTE in r.stderr) == taken, (case, variant, extra, r.stderr[-1500:])
            got = r.stdout.decode("latin1")
            assert sorted(got.splitlines()) == sorted(want.splitlines()), (case, variant, extra)
            assert len(got) == len(want), (case, variant)


def test_pcr_match_output_equals_the_reference():
    """primer pairs with one primer of 33 nt or more each; compared as sorted lines (the order of hits that end at one
    position is engine specific); the same output with the permission, without it and with PM_LONG_EXACT=off beside it"""
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
            assert c["stdout"].strip(), case
            for extra, taken in ROUTES:
                r = subprocess.run([PCR, "-i", fa, "-P", qf] + c["options"], capture_output=True, timeout=300, env=environment(PM_DEBUG="1", **extra))
                assert r.returncode == 0, (case, r.stderr[-500:])
                assert (ROUTE in r.stderr) == taken, (case, extra, r.stderr[-1500:])
                got = r.stdout.decode("latin1")
                assert sorted(got.splitlines()) == sorted(c["stdout"].splitlines()), (case, extra)
                assert len(got) == len(c["stdout"])
