"""GPU: pm_init_windowed -- the stream stays in host memory and HBM holds a ring of windows of it.  Every test checks
that the windowed path ran (pm_stream_residency: a window size, more than one window load) and that the hits are
those of the resident form (pm_init), the committed reference outputs or the oracle."""
import glob
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import adversarial as A
import synth
import sat_amd
from oracle import pmoracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")
CASES = sorted(p for p in glob.glob(os.path.join(GOLD, "*.json")) if "config1" not in p and not os.path.basename(p).startswith(("cli_", "pcr_")))
SEL2SEM = {0: sat_amd.SEM_AUTO, 1: sat_amd.SEM_KEYWORD_TREE, 2: sat_amd.SEM_KEYWORD_TREE, 4: sat_amd.SEM_SHIFT_AND,
           5: sat_amd.SEM_FILTER_BITVEC, 12: sat_amd.SEM_EXACT_HALVES, 14: sat_amd.SEM_EXACT_HALVES,
           100: sat_amd.SEM_SHIFT_AND_INEXACT}
TABLE = b"ACGT\n"
# the documented bound of the HBM a windowed handle holds for the stream: two slots of
# window + 2 guard margins, 1.25 bytes per base (text + 2-bit words); a guard margin is the halo plus at most 4 MiB + 17 KiB
GUARD_MAX = (4 << 20) + (17 << 10) + 4096


def residency_bound(window):
    return int(2 * 1.25 * (window + 2 * GUARD_MAX)) + 1024


def engine(pats, k, indels, sem=sat_amd.SEM_AUTO, kernel=sat_amd.KERNEL_AUTO, zones=None, wildcards=False, text_n=False):
    pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sem, kernel=kernel, wildcards=wildcards, text_n=text_n)
    for i, p in enumerate(pats):
        z = zones[i] if zones else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    return pm


def run(pats, codes, table, k, indels, window, chunk=1 << 26, **kw):
    """(hits of find_all on a windowed handle, its residency figures)"""
    pm = engine(pats, k, indels, **kw)
    pm.init(codes, table, window=window)
    got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
    res = pm.residency()
    pm.close()
    return got, res


def resident(pats, codes, table, k, indels, chunk=1 << 26, **kw):
    pm = engine(pats, k, indels, **kw)
    pm.init(codes, table)
    got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
    pm.close()
    return got


def min_window(pats, k, indels, **kw):
    pm = engine(pats, k, indels, **kw)
    pm.init(np.zeros(64, dtype=np.uint8), TABLE, window=1)
    w = pm.residency()["window"]
    pm.close()
    return w


def ran_windowed(res, n):
    assert res["window"] > 0 and res["loads"] >= 1 and res["uploaded"] >= n, res
    if n > 2 * res["window"]:
        assert res["loads"] > 1, res


def load(path):
    with open(path) as f:
        c = json.load(f)
    table = c["table"].encode("latin1")
    codes = synth.normalize(synth.stream(c["entries"]), table)
    pats = c["patterns"]
    return c, codes, table, pats + [sat_amd.reverse_comp(p) for p in pats]


def test_residency_of_a_resident_handle():
    codes = np.array([0, 1, 2, 3] * 1000, dtype=np.uint8)
    pm = engine(["ACGTACGTACGT"], 0, False)
    pm.init(codes, TABLE)
    r = pm.residency()
    assert r["window"] == 0 and r["uploaded"] == codes.size and r["loads"] == 1 and r["held"] >= codes.size
    pm.close()


@pytest.mark.parametrize("kernel", [sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_SEED, sat_amd.KERNEL_AUTO])
@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-5] for p in CASES])
def test_golden_engine_hits_windowed(path, kernel):
    c, codes, table, allp = load(path)
    ran = 0
    for name, e in c["engine"].items():
        sem = SEL2SEM[e["sel"]]
        try:
            base = resident(allp, codes, table, e["k"], e["indels"], sem=sem, kernel=kernel)
        except sat_amd.PmError as err:
            assert kernel == sat_amd.KERNEL_SEED and err.code == -2, (c["name"], name, err)
            continue
        want = [tuple(h) for h in e["hits"]]
        assert base == want
        w0 = min_window(allp, e["k"], e["indels"], sem=sem, kernel=kernel)
        # the minimum window with ranges smaller than it, three times the minimum with ranges much larger
        for window, chunk in ((w0, 997), (3 * w0, 1 << 26)):
            got, res = run(allp, codes, table, e["k"], e["indels"], window, chunk=chunk, sem=sem, kernel=kernel)
            assert res["window"] == window, res
            ran_windowed(res, codes.size)
            assert got == want, (c["name"], name, kernel, window, chunk)
        ran += 1
    assert ran >= 7


@pytest.mark.parametrize("seed", range(60))
def test_adversarial_windowed_vs_oracle(seed):
    c = A.small_case(seed * 7919 + 11)
    want = A.oracle_hits(c)
    if want is None:
        return                                                        # the reference rejects this option set (select.cc:87-90)
    with A.knobs(c["env"]):
        pm = engine(c["patterns"], c["k"], c["indels"], sem=c["sem"], zones=c["zones"], wildcards=c["wild"])
    w0 = 0
    try:
        pm.init(c["stream"], c["table"], window=1)
        w0 = pm.residency()["window"]
        pm.close()
        with A.knobs(c["env"]):
            pm = engine(c["patterns"], c["k"], c["indels"], sem=c["sem"], zones=c["zones"], wildcards=c["wild"])
        window = w0 + 64 * (seed % 5)
        pm.init(c["stream"], c["table"], window=window)
        chunk = c["chunk"] if c["chunk"] % window else c["chunk"] + 1  # ranges that do not divide the window
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        res = pm.residency()
    finally:
        pm.close()
    ran_windowed(res, c["n"])
    assert got == want, A.describe(c)


def tandem_case(seed, total):
    rng = np.random.default_rng(seed)
    unit = "CA" if seed % 2 else "ACGTA"
    rep = (unit * (total // len(unit) + 1))[:total]
    pre = "".join("ACGT"[x] for x in rng.integers(0, 4, 3000))
    post = "".join("ACGT"[x] for x in rng.integers(0, 4, 3000))
    s = pre + rep + post
    lut = np.zeros(256, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = i
    codes = lut[np.frombuffer(s.encode(), dtype=np.uint8)]
    pats = [rep[3:23], rep[10:32], pre[100:121], post[500:522]]
    return codes, pats + [sat_amd.reverse_comp(p) for p in pats]


@pytest.mark.parametrize("indels", [False, True])
@pytest.mark.parametrize("seed", [0, 1])
def test_long_tandem_chain_spans_windows(seed, indels):
    """a same-pattern chain of candidates (gaps <= 2k+1) over a tandem repeat longer than three windows: what the device
    cluster DP of the last piece reads reaches back over all of them (carry_reach)"""
    k = 2
    w0 = min_window(["A" * 22], k, indels)
    codes, allp = tandem_case(seed, 4 * w0 + 500)
    text = O.Text(codes, TABLE)
    want = O.sorted_tuples(O.find_all(text, allp, engine=O.pick_engine(text, allp, k, indels), k=k, indels=indels))
    got, res = run(allp, codes, TABLE, k, indels, w0, chunk=w0 // 3)
    ran_windowed(res, codes.size)
    assert len(want) > 0 and got == want
    got2, _ = run(allp, codes, TABLE, k, indels, w0, chunk=1 << 26)
    assert got2 == want


def test_stream_edges():
    rng = np.random.default_rng(3)
    ents = synth.make_entries(rng, 3, 4000, n_runs=2, repeats=True, short=True)
    pats = synth.make_patterns(rng, ents, 60, length=22, planted=0.5)
    allp = pats + [synth.revcomp(p) for p in pats]
    codes = synth.normalize(synth.stream(ents), TABLE)
    for k, indels in ((0, False), (2, False), (2, True)):
        w0 = min_window(allp, k, indels)
        # a stream shorter than one window
        short = codes[:w0 // 2].copy()
        got, res = run(allp, short, TABLE, k, indels, w0)
        assert res["window"] == w0 and res["loads"] == 1
        assert got == resident(allp, short, TABLE, k, indels)
        want = resident(allp, codes, TABLE, k, indels)
        for tail in (1, 2, 3, 4):                                     # the last range (and window) holds 1 .. 4 positions
            pm = engine(allp, k, indels)
            pm.init(codes, TABLE, window=w0)
            n = codes.size
            cuts = [5] + list(range(w0, n - tail, w0)) + [n - tail, n]   # a first range shorter than the longest pattern
            parts, pos = [], 0
            for e in cuts:
                parts.append(pm.scan_view(pos, e).copy())
                pos = e
            h = np.concatenate(parts)
            assert sat_amd.sorted_tuples(h) == want, (k, indels, tail)
            loads = pm.residency()["loads"]
            assert loads > 1
            assert sat_amd.sorted_tuples(pm.find_all(chunk=w0 // 2 + 3)) == want    # pm_reset, then a second pass
            assert pm.residency()["loads"] > loads
            pm.close()


@pytest.mark.parametrize("text_n", [False, True])
def test_wildcards_on_a_raw_stream(text_n):
    """-w / -W on a raw stream: the census of the letters the stream holds is taken from the host copy"""
    rng = np.random.default_rng(9 + text_n)
    n = 20000
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    s[rng.integers(0, n, 60)] = ord("N")
    s[rng.integers(0, n, 30)] = ord("\n")
    s[rng.integers(0, n, 10)] = ord("R")
    pats = []
    for _ in range(20):
        a = int(rng.integers(0, n - 25))
        q = list(s[a:a + 20].tobytes().decode().replace("\n", "A"))
        q[int(rng.integers(0, 20))] = "NRYKM"[int(rng.integers(0, 5))]
        pats.append("".join(q))
    for k, indels in ((0, False), (1, True)):
        w0 = min_window(pats, k, indels, wildcards=True, text_n=text_n)
        got, res = run(pats, s, None, k, indels, w0, chunk=1500, wildcards=True, text_n=text_n)
        ran_windowed(res, n)
        text = O.Text(s)
        want = O.sorted_tuples(O.find_all(text, pats, k=k, indels=indels, wildcards=True, text_n=text_n))
        assert got == want, (k, indels, text_n)


def random_db(n, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda", generator=g)
    t[0] = 4
    t[-1] = 4
    t[n // 3] = 4
    return t.cpu().numpy()


def sampled_primers(host, rng, count, L=20):
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    while len(out) < count:
        a = int(rng.integers(1, min(host.size, 1 << 24) - L - 1))
        w = host[a:a + L]
        if (w > 3).any():
            continue
        out.append(lut[w].tobytes().decode())
    return out


def test_bounded_memory_64mbp():
    n, window = 64 << 20, 1 << 20
    host = random_db(n, 5)
    rng = np.random.default_rng(5)
    pats = sampled_primers(host, rng, 500) + ["".join("ACGT"[x] for x in rng.integers(0, 4, 20)) for _ in range(500)]
    allp = pats + [sat_amd.reverse_comp(p) for p in pats]
    pm = engine(allp, 1, False)
    pm.init(host, TABLE, window=window)
    got = pm.find_all(chunk=1 << 30)
    res = pm.residency()
    pm.close()
    assert res["window"] == window and res["loads"] > 1 and res["uploaded"] >= n, res
    assert res["peak"] <= residency_bound(window), res
    assert res["peak"] < n, res
    pm = engine(allp, 1, False)
    pm.init(host, TABLE)
    want = pm.find_all(chunk=1 << 30)
    pm.close()
    assert want.size > 500 and sat_amd.sorted_tuples(got) == sat_amd.sorted_tuples(want)


def test_full_size_3gbp():
    """100k 20-mers (50k and their reverse complements) over 3 Gbp at -K 2 in 256 MiB windows: the hits of the resident form"""
    n, window = 3 * 10 ** 9, 256 << 20
    host = random_db(n, 7)
    rng = np.random.default_rng(7)
    pats = sampled_primers(host, rng, 2000) + ["".join("ACGT"[x] for x in rng.integers(0, 4, 20)) for _ in range(48000)]
    allp = pats + [sat_amd.reverse_comp(p) for p in pats]
    out = {}
    for mode in ("resident", "windowed"):
        pm = engine(allp, 2, False)
        pm.init(host, TABLE, window=window if mode == "windowed" else None)
        out[mode] = pm.find_all(chunk=1 << 30)
        res = pm.residency()
        pm.close()
        if mode == "windowed":
            assert res["window"] == window and res["loads"] >= n // window and res["uploaded"] >= n, res
            assert res["peak"] <= residency_bound(window), res
    a, b = out["resident"], out["windowed"]
    assert a.size > 2000 and a.size == b.size
    assert (a["end"] == b["end"]).all() and (a["pid"] == b["pid"]).all() and (a["k"] == b["k"]).all()


def test_command_lines_in_windows():
    """pm_primer_match / pm_pcr_match with PM_GPU_WINDOW set (a window far smaller than the databases): the committed
    reference outputs, and -v names the windowed mode"""
    from test_gpu_primer_match_cli import load as cli_load, prepare, PM, CS
    env = dict(os.environ, PM_GPU_WINDOW="4096")
    for fixture in ("cli_a", "cli_b"):
        g = cli_load(fixture)
        with tempfile.TemporaryDirectory() as d:
            prepare(g, d)
            for case, c in g["cases"].items():
                fa = os.path.join(d, "normalized", "db.fa")
                if c["primers"] == "p":
                    parg = ["-p", " ".join(g["primers_txt"].split()[:5])]
                else:
                    parg = ["-" + ("P" if c["primers"] == "W" else c["primers"]), os.path.join(d, "primers." + c["primers"])]
                got = subprocess.run([PM, "-i", fa] + parg + c["options"] + ["-v"], capture_output=True, timeout=300, env=env)
                assert got.returncode == 0, (case, got.stderr[-500:])
                assert b"stream: windowed, window" in got.stderr, got.stderr[-500:]
                want = c["normalized"]
                out = got.stdout.decode("latin1")
                assert sorted(out.splitlines()) == sorted(want.splitlines()) and len(out) == len(want), (fixture, case)
    PCR = os.path.join(HOST, "pm_pcr_match")
    FLAG = {"S": "-S", "P": "-P", "Q": "-P", "F": "-F"}
    for fixture in ("pcr_a", "pcr_b"):
        with open(os.path.join(GOLD, fixture + ".json")) as f:
            g = json.load(f)
        with tempfile.TemporaryDirectory() as d:
            fa = os.path.join(d, "db.fa")
            with open(fa, "w") as f:
                f.write(g["fasta"])
            assert subprocess.run([CS, "-i", fa, "-n", "true"], capture_output=True).returncode == 0
            for k, text in g["primers"].items():
                with open(os.path.join(d, "primers." + k), "w") as f:
                    f.write(text)
            for case, c in g["cases"].items():
                cmd = [PCR, "-i", fa, FLAG[c["primers"]], os.path.join(d, "primers." + c["primers"])] + c["options"]
                got = subprocess.run(cmd + ["-v"], capture_output=True, timeout=300, env=env)
                assert got.returncode == 0 and b"stream: windowed, window" in got.stderr, (case, got.stderr[-500:])
                out = got.stdout.decode("latin1")
                assert sorted(out.splitlines()) == sorted(c["stdout"].splitlines()) and len(out) == len(c["stdout"]), (fixture, case)
