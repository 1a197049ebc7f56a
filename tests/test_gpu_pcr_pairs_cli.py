"""GPU: pm_pcr_match with the pairing stage on the device (PM_GPU_PCR=1) against the recorded output of
the reference's pcr_match (tests/golden/pcr_a.json, pcr_b.json and the hit-dense pcr_dense.json of
tests/golden/make_pcr_dense_golden.py; compared as tests/test_gpu_pcr_match_cli.py compares) and, byte for byte, against
the host loop's output of the same command line.  With --ranks 2 or PM_GPU_WINDOW next to PM_GPU_PCR=1 the host loop runs
and the output does not change."""
import json
import os
import subprocess
import tempfile

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")
PCR = os.path.join(HOST, "pm_pcr_match")
CS = os.path.join(HOST, "pm_compress_seq")
FLAG = {"S": "-S", "P": "-P", "Q": "-P", "F": "-F"}
ON_GPU = b"pairing on the GPU"
FIXTURES = ["pcr_a", "pcr_b", "pcr_dense"]


def load(fixture):
    with open(os.path.join(ROOT, "tests", "golden", fixture + ".json")) as f:
        return json.load(f)


CASES = [(fx, case) for fx in FIXTURES for case in load(fx)["cases"]]


def run(cmd, env_more=None):
    env = dict(os.environ)
    for k in ("PM_GPU_PCR", "PM_GPU_WINDOW", "PM_RANKS"):
        env.pop(k, None)
    env.update(env_more or {})
    r = subprocess.run(cmd, capture_output=True, timeout=300, env=env)
    assert r.returncode == 0, (cmd, r.stderr[-800:])
    return r.stdout.decode("latin1"), r.stderr


@pytest.fixture(scope="module")
def databases():
    """every fixture's database and primer files, written once"""
    assert os.path.exists(PCR) and os.path.exists(CS), "run __graft_entry__.build()"
    with tempfile.TemporaryDirectory() as top:
        out = {}
        for fx in FIXTURES:
            g = load(fx)
            d = os.path.join(top, fx)
            os.mkdir(d)
            fa = os.path.join(d, "db.fa")
            with open(fa, "w") as f:
                f.write(g["fasta"])
            run([CS, "-i", fa, "-n", "true"])
            for k, text in g["primers"].items():
                with open(os.path.join(d, "primers." + k), "w") as f:
                    f.write(text)
            out[fx] = (g, d, fa)
        yield out


def command(databases, fixture, case):
    g, d, fa = databases[fixture]
    c = g["cases"][case]
    return c, [PCR, "-i", fa, FLAG[c["primers"]], os.path.join(d, "primers." + c["primers"])] + c["options"] + ["-v"]


@pytest.mark.parametrize("fixture,case", CASES)
def test_device_route_equals_reference_and_host_route(databases, fixture, case):
    c, cmd = command(databases, fixture, case)
    host, err_host = run(cmd)
    got, err = run(cmd, {"PM_GPU_PCR": "1"})
    assert ON_GPU in err and ON_GPU not in err_host
    assert got == host                                               # byte for byte, the order of the lines included
    assert sorted(got.splitlines()) == sorted(c["stdout"].splitlines())
    assert len(got) == len(c["stdout"])


def test_dense_fixture_is_dense(databases):
    """what pcr_dense.json is for: hundreds of hits of one pair, many rounds (-R 1), several partners per hit"""
    _, cmd = command(databases, "pcr_dense", "dense_k1_R1")
    _, err = run(cmd, {"PM_GPU_PCR": "1"})
    line = [x for x in err.decode().splitlines() if "pairing on the GPU" in x][0]
    words = line.replace(",", " ").replace(";", " ").split()
    hits, amplicons, cands = int(words[words.index("primer") - 1]), int(words[words.index("amplicons") - 1]), int(words[words.index("candidate") - 1])
    assert hits > 190 and amplicons > 190 and cands >= amplicons


@pytest.mark.parametrize("fixture,case", [("pcr_a", "sts_k1_default"), ("pcr_a", "pairs_r_k1_allorient"), ("pcr_dense", "dense_k1_allorient")])
def test_ranks_and_windows_keep_the_host_route(databases, fixture, case):
    _, cmd = command(databases, fixture, case)
    host, _ = run(cmd)
    for more, env in ((["--ranks", "2"], {"PM_GPU_PCR": "1"}), ([], {"PM_GPU_PCR": "1", "PM_GPU_WINDOW": "4096"}), ([], {"PM_GPU_PCR": "0"})):
        got, err = run(cmd + more, env)
        assert ON_GPU not in err, (more, env)
        assert got == host, (more, env)
