"""GPU: a bit-packed stream (<db>.sqz: char_io.t:18-214) crosses PCIe packed and is unpacked in HBM.  The unpack kernel
alone against numpy; pm_init_packed handles, resident and windowed, against the committed reference outputs and the
oracle; the stream's edges; one full-size stream; the command lines on a .sqz database."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import adversarial as A
import sat_amd
from oracle import pmoracle as O
from test_gpu_windowed import CASES, GUARD_MAX, SEL2SEM, TABLE, engine, load, min_window, random_db, sampled_primers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")
# adversarial.small_case(seed): the 40 lowest seeds from 1000 on whose case has a table (a packed stream needs one)
SEEDS = [1001, 1004, 1008, 1011, 1012, 1013, 1014, 1016, 1017, 1018, 1020, 1021, 1022, 1024, 1025, 1029, 1030, 1031, 1032, 1033,
         1037, 1039, 1041, 1043, 1044, 1046, 1049, 1050, 1051, 1053, 1054, 1055, 1056, 1057, 1059, 1061, 1063, 1064, 1065, 1066]


def bits_for(table):
    return max(1, (len(table) - 1).bit_length())


def packed_bound(window, bits):
    """the documented bound of the HBM a windowed packed handle holds for the stream (pm_gpu.h)"""
    return int(2 * (1.25 + bits / 8) * (window + 2 * GUARD_MAX)) + 2048


def np_words(codes):
    """the seed family's 2-bit words: dword i = bases 16i .. 16i+15, base j in bits 2j, value code & 3, zero past the end"""
    nw = (codes.size + 15) // 16
    c = np.zeros(nw * 16, dtype=np.uint32)
    c[:codes.size] = codes & 3
    return (c.reshape(nw, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint64).astype(np.uint32)


# ---- the kernel alone -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", range(1, 9))
def test_unpack_kernel_against_numpy(bits):
    rng = np.random.default_rng(100 + bits)
    for n in (1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, (1 << 20) + 3):
        codes = rng.integers(0, 1 << bits, n, dtype=np.uint8)
        packed = sat_amd.pack_codes(codes, bits)
        d_packed = torch.from_numpy(packed).cuda()
        for first in sorted({0, 64, 64 * 3, 64 * (n // 128)}):
            if first >= n:
                continue
            m = n - first
            pad, nw = (m + 15) // 16 * 16, (m + 15) // 16
            d_text = torch.full((pad + 256,), 0xAB, dtype=torch.uint8, device="cuda")
            d_words = torch.full((nw + 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            off = first * bits // 8
            for with_words in (True, False):
                d_text.fill_(0xAB)
                sat_amd.unpack_device(d_packed.data_ptr() + off, packed.size - off, bits, m, d_text.data_ptr(), d_words.data_ptr() if with_words else 0)
                torch.cuda.synchronize()
                text = d_text.cpu().numpy()
                assert (text[:m] == codes[first:]).all(), (bits, n, first)
                assert not text[m:pad].any(), (bits, n, first, "bytes past n up to the next multiple of 16 are zero")
                assert (text[pad:] == 0xAB).all(), (bits, n, first, "canary behind the text")
            words = d_words.cpu().numpy().view(np.uint32)
            assert (words[:nw] == np_words(codes[first:])).all(), (bits, n, first)
            assert (words[nw:] == 0x5A5A5A5A).all(), (bits, n, first, "canary behind the words")


def test_unpack_device_refuses_bad_arguments():
    t = torch.zeros(256, dtype=torch.uint8, device="cuda")
    p = t.data_ptr()
    for args in ((p, 24, 0, 64, p), (p, 24, 9, 2, p), (p, 24, 3, 65, p), (p + 4, 24, 3, 8, p), (p, 24, 3, 8, p + 8), (p, -1, 3, 0, p), (p, 24, 3, -1, p)):
        with pytest.raises(sat_amd.PmError):
            sat_amd.unpack_device(*args)


# ---- handles ------------------------------------------------------------------------------------------------------------
def run_packed(pats, codes, table, k, indels, window=None, chunk=1 << 26, bits=None, **kw):
    """(hits of find_all on a pm_init_packed handle, its residency figures)"""
    bits = bits or bits_for(table)
    pm = engine(pats, k, indels, **kw)
    try:
        pm.init_packed(sat_amd.pack_codes(codes, bits), bits, codes.size, table, window=window)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        res = pm.residency()
    finally:
        pm.close()
    assert res["bits"] == bits, res
    return got, res


def run_unpacked(pats, codes, table, k, indels, window=None, chunk=1 << 26, **kw):
    pm = engine(pats, k, indels, **kw)
    try:
        pm.init(codes, table, window=window)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        res = pm.residency()
    finally:
        pm.close()
    assert res["bits"] == 0, res
    return got, res


def check_resident(res, n, bits):
    assert res["window"] == 0 and res["loads"] == 1, res
    assert 0 < res["uploaded"] <= (n * bits + 7) // 8, res
    assert n <= res["held"] <= res["peak"], res


def check_windowed(res, base, n, window, bits):
    """res: the packed handle's figures, base: those of a pm_init_windowed handle on the unpacked codes after the same calls"""
    assert res["window"] == window == base["window"], (res, base)
    assert res["loads"] == base["loads"] >= 1, (res, base)
    if n > 2 * window:
        assert res["loads"] > 1, res
    assert res["uploaded"] <= base["uploaded"] * bits / 8 + 64 * res["loads"], (res, base)
    assert res["peak"] <= packed_bound(window, bits), res


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-5] for p in CASES])
def test_golden_engine_hits_packed(path):
    c, codes, table, allp = load(path)
    bits = bits_for(table)
    assert bits == 3
    assert len(c["engine"]) >= 7
    for name, e in c["engine"].items():
        sem = SEL2SEM[e["sel"]]
        want = [tuple(h) for h in e["hits"]]
        got, res = run_packed(allp, codes, table, e["k"], e["indels"], sem=sem)
        check_resident(res, codes.size, bits)
        assert got == want, (c["name"], name, "resident")
        w0 = min_window(allp, e["k"], e["indels"], sem=sem)
        for window, chunk in ((w0, 997), (3 * w0, 1 << 26)):
            got, res = run_packed(allp, codes, table, e["k"], e["indels"], window=window, chunk=chunk, sem=sem)
            _, base = run_unpacked(allp, codes, table, e["k"], e["indels"], window=window, chunk=chunk, sem=sem)
            check_windowed(res, base, codes.size, window, bits)
            assert got == want, (c["name"], name, window, chunk)


@pytest.mark.parametrize("size", [17, 200])
def test_wider_codes(size):
    """small_mixed with its table extended by symbols the stream does not use: 5 and 8 bits per code.  Expected hits: the
    committed reference outputs where the option set names its engine, and in every case pm_init's on the same codes
    and table (the automatic choice looks at the alphabet size, select.cc:117-126)."""
    path = [p for p in CASES if os.path.basename(p) == "small_mixed.json"][0]
    c, codes, table, allp = load(path)
    extra = bytes(b for b in range(1, 256) if b not in table and chr(b).upper() not in "ACGTUNRYKMSWBDHVX")
    wide = table + extra[:size - len(table)]
    bits = bits_for(wide)
    assert len(wide) == size and bits == (5 if size == 17 else 8)
    for name, e in c["engine"].items():
        sem = SEL2SEM[e["sel"]]
        want, _ = run_unpacked(allp, codes, wide, e["k"], e["indels"], sem=sem)
        if sem != sat_amd.SEM_AUTO:
            assert want == [tuple(h) for h in e["hits"]], (name, size)
        got, res = run_packed(allp, codes, wide, e["k"], e["indels"], sem=sem, bits=bits)
        check_resident(res, codes.size, bits)
        assert got == want, (name, size, "resident")
        w0 = min_window(allp, e["k"], e["indels"], sem=sem)
        got, res = run_packed(allp, codes, wide, e["k"], e["indels"], window=w0, chunk=1499, sem=sem, bits=bits)
        assert res["window"] == w0 and res["peak"] <= packed_bound(w0, bits), res
        assert got == want, (name, size, "windowed")


def adversarial_engine(c):
    with A.knobs(c["env"]):
        return engine(c["patterns"], c["k"], c["indels"], sem=c["sem"], zones=c["zones"], wildcards=c["wild"])


@pytest.mark.parametrize("seed", SEEDS)
def test_adversarial_packed_vs_oracle(seed):
    """the host-stage verifies (-k, exact zones, primers with ambiguity letters, N in the stream) on a handle with no host
    text: find_all whole and in the case's ranges"""
    c = A.small_case(seed)
    assert c["table"] is not None, "the seed list holds cases with a table only"
    want = A.oracle_hits(c)
    assert want is not None, A.describe(c)
    bits = bits_for(c["table"])
    packed = sat_amd.pack_codes(c["stream"], bits)
    pm = adversarial_engine(c)
    try:
        pm.init_packed(packed, bits, c["n"], c["table"])
        whole = sat_amd.sorted_tuples(pm.find_all())
        parts = sat_amd.sorted_tuples(pm.find_all(chunk=c["chunk"]))
        res = pm.residency()
    finally:
        pm.close()
    assert res["bits"] == bits
    check_resident(res, c["n"], bits)
    assert whole == want, A.describe(c)
    assert parts == want, A.describe(c)


@pytest.mark.parametrize("seed", SEEDS[:20])
def test_adversarial_packed_windowed_vs_oracle(seed):
    c = A.small_case(seed)
    want = A.oracle_hits(c)
    assert c["table"] is not None and want is not None, A.describe(c)
    bits = bits_for(c["table"])
    packed = sat_amd.pack_codes(c["stream"], bits)
    pm = adversarial_engine(c)
    try:
        pm.init(c["stream"], c["table"], window=1)
        w0 = pm.residency()["window"]
    finally:
        pm.close()
    for window, chunk in ((w0, c["chunk"] if c["chunk"] % w0 else c["chunk"] + 1), (3 * w0, 1 << 26)):
        out = []
        for form in ("packed", "unpacked"):
            pm = adversarial_engine(c)
            try:
                if form == "packed":
                    pm.init_packed(packed, bits, c["n"], c["table"], window=window)
                else:
                    pm.init(c["stream"], c["table"], window=window)
                out.append((sat_amd.sorted_tuples(pm.find_all(chunk=chunk)), pm.residency()))
            finally:
                pm.close()
        assert out[0][1]["bits"] == bits and out[1][1]["bits"] == 0
        check_windowed(out[0][1], out[1][1], c["n"], window, bits)
        assert out[0][0] == want, (A.describe(c), window, chunk)


# ---- the end of the stream --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0, 37])
@pytest.mark.parametrize("k,indels", [(2, False), (2, True)])
def test_hits_at_the_end_of_the_stream(k, indels, fill):
    """primers cut so that their sites end at n, n - 1, ... n - 17 of a stream whose length is no multiple of 16 (the DPs
    of -K 2 / -k 2 read past the hit: beyond n they must see what load16_edge hands out), and the same stream followed by
    end-of-sequence codes, as compress_seq fills the last buffer of a .sqz"""
    rng = np.random.default_rng(77)
    n0 = 9000 + 11
    body = rng.integers(0, 4, n0).astype(np.uint8)
    body[0] = 4
    body[n0 // 2] = 4
    codes = np.concatenate([body, np.full(fill, 4, dtype=np.uint8)])
    assert codes.size % 16 and n0 % 16
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    pats = [lut[body[e - 20:e]].tobytes().decode() for e in range(n0 - 17, n0 + 1)]
    pats += [lut[body[e - 22:e]].tobytes().decode() for e in (n0 - 3, n0 - 1, n0)]
    allp = pats + [sat_amd.reverse_comp(p) for p in pats]
    text = O.Text(codes, TABLE)
    want = O.sorted_tuples(O.find_all(text, allp, engine=O.pick_engine(text, allp, k, indels), k=k, indels=indels))
    ends = {h[0] for h in want}
    assert len(want) >= 18 and all(any(abs(e - x) <= 2 * k + 1 for x in ends) for e in range(n0 - 17, n0 + 1))
    got, res = run_packed(allp, codes, TABLE, k, indels)
    check_resident(res, codes.size, 3)
    assert got == want, "resident"
    w0 = min_window(allp, k, indels)
    for chunk in (w0 // 3 + 1, 1 << 26):
        got, res = run_packed(allp, codes, TABLE, k, indels, window=w0, chunk=chunk)
        assert res["window"] == w0 and res["loads"] > 1, res
        assert got == want, ("windowed", chunk)


# ---- size ----------------------------------------------------------------------------------------------------------------
def test_one_gbp_packed():
    """100k 20-mers (50k and their reverse complements) over 1 Gbp at 3 bits per code, -K 2: resident and in 256 MiB
    windows, the hit list of pm_init on the unpacked codes"""
    n, window, bits = 10 ** 9, 256 << 20, 3
    host = random_db(n, 17)
    rng = np.random.default_rng(17)
    pats = sampled_primers(host, rng, 2000) + ["".join("ACGT"[x] for x in rng.integers(0, 4, 20)) for _ in range(48000)]
    allp = pats + [sat_amd.reverse_comp(p) for p in pats]
    packed = np.zeros((n * bits + 7) // 8, dtype=np.uint8)
    step = 1 << 27                                                     # (a multiple of 8 codes: slices end on whole bytes)
    for a in range(0, n, step):
        packed[a // 8 * bits:(min(n, a + step) * bits + 7) // 8] = sat_amd.pack_codes(host[a:a + step], bits)
    assert (sat_amd.unpack_codes(packed, bits, n - 1000, 1000) == host[-1000:]).all()
    pm = engine(allp, 2, False)
    pm.init(host, TABLE)
    want = pm.find_all(chunk=1 << 30)
    pm.close()
    assert want.size > 2000
    for mode in ("resident", "windowed"):
        pm = engine(allp, 2, False)
        pm.init_packed(packed, bits, n, TABLE, window=window if mode == "windowed" else None)
        got = pm.find_all(chunk=1 << 30)
        res = pm.residency()
        pm.close()
        assert res["bits"] == bits
        if mode == "windowed":
            assert res["window"] == window and res["loads"] >= n // window, res
            assert res["uploaded"] <= (n + 2 * window) * bits // 8 + 64 * res["loads"], res
            assert res["peak"] <= packed_bound(window, bits), res
        else:
            check_resident(res, n, bits)
        assert got.size == want.size, mode
        assert (got["end"] == want["end"]).all() and (got["pid"] == want["pid"]).all() and (got["k"] == want["k"]).all(), mode


# ---- command lines -----------------------------------------------------------------------------------------------------
def routes():
    """(name, environment, what -v must say) of the three routes a .sqz database can take"""
    base = {k: v for k, v in os.environ.items() if k not in ("PM_GPU_PACKED", "PM_GPU_WINDOW")}
    return (("packed", base, b"stream: packed, 3 bits per code, resident"),
            ("unpacked on the host", dict(base, PM_GPU_PACKED="0"), b"stream: resident"),
            ("packed windows", dict(base, PM_GPU_WINDOW="4096"), b"stream: packed, 3 bits per code, windowed"))


def uploaded_fewer_bytes_than_bases(stderr):
    line = [x for x in stderr.decode("latin1").splitlines() if x.startswith("stream: packed") and "resident" in x][0]
    w = line.split()
    up, n = int(w[w.index("bytes") - 1]), int(w[w.index("positions") - 1])
    return 0 < up < n and up <= (3 * n + 7) // 8


@pytest.mark.parametrize("fixture", ["cli_a", "cli_b"])
def test_primer_match_on_a_compressed_database(fixture):
    from test_gpu_primer_match_cli import load as cli_load, prepare, PM, CS
    g = cli_load(fixture)
    with tempfile.TemporaryDirectory() as d:
        prepare(g, d)
        os.mkdir(os.path.join(d, "compressed"))
        fa = os.path.join(d, "compressed", "db.fa")
        with open(fa, "w") as f:
            f.write(g["fasta"])
        assert subprocess.run([CS, "-i", fa, "-z", "true"], capture_output=True).returncode == 0
        assert os.path.exists(fa + ".sqz") and not os.path.exists(fa + ".sqn")
        for case, c in g["cases"].items():
            if c["primers"] == "p":
                parg = ["-p", " ".join(g["primers_txt"].split()[:5])]
            else:
                parg = ["-" + ("P" if c["primers"] == "W" else c["primers"]), os.path.join(d, "primers." + c["primers"])]
            want = c["compressed"]
            for name, env, says in routes():
                r = subprocess.run([PM, "-i", fa] + parg + c["options"] + ["-v"], capture_output=True, timeout=300, env=env)
                assert r.returncode == 0, (case, name, r.stderr[-500:])
                assert says in r.stderr, (case, name, r.stderr[-500:])
                if name == "packed":
                    assert uploaded_fewer_bytes_than_bases(r.stderr), r.stderr[-500:]
                out = r.stdout.decode("latin1")
                assert sorted(out.splitlines()) == sorted(want.splitlines()) and len(out) == len(want), (fixture, case, name)


@pytest.mark.parametrize("fixture", ["pcr_a"])
def test_pcr_match_on_a_compressed_database(fixture):
    """the .sqz stream is the .sqn one plus end-of-sequence codes at the end: the same lines as the normalized run"""
    from test_gpu_primer_match_cli import CS
    PCR = os.path.join(HOST, "pm_pcr_match")
    FLAG = {"S": "-S", "P": "-P", "Q": "-P", "F": "-F"}
    with open(os.path.join(GOLD, fixture + ".json")) as f:
        g = json.load(f)
    with tempfile.TemporaryDirectory() as d:
        fas = {}
        for variant, args in (("normalized", ["-n", "true"]), ("compressed", ["-z", "true"])):
            os.mkdir(os.path.join(d, variant))
            fas[variant] = os.path.join(d, variant, "db.fa")
            with open(fas[variant], "w") as f:
                f.write(g["fasta"])
            assert subprocess.run([CS, "-i", fas[variant]] + args, capture_output=True).returncode == 0
        assert os.path.exists(fas["compressed"] + ".sqz") and not os.path.exists(fas["compressed"] + ".sqn")
        for k, text in g["primers"].items():
            with open(os.path.join(d, "primers." + k), "w") as f:
                f.write(text)
        for case, c in g["cases"].items():
            args = [FLAG[c["primers"]], os.path.join(d, "primers." + c["primers"])] + c["options"]
            ref = subprocess.run([PCR, "-i", fas["normalized"]] + args, capture_output=True, timeout=300)
            assert ref.returncode == 0, (case, ref.stderr[-500:])
            want = ref.stdout.decode("latin1")
            assert sorted(want.splitlines()) == sorted(c["stdout"].splitlines())
            for name, env, says in routes():
                r = subprocess.run([PCR, "-i", fas["compressed"]] + args + ["-v"], capture_output=True, timeout=300, env=env)
                assert r.returncode == 0 and says in r.stderr, (case, name, r.stderr[-500:])
                out = r.stdout.decode("latin1")
                assert sorted(out.splitlines()) == sorted(want.splitlines()) and len(out) == len(want), (fixture, case, name)
