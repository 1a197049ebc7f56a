"""GPU: the re-alignment with indels of primers of 33..64 characters on the device (bit 4 of pm_config.long_patterns,
long_align=True; csrc/pm_align_wide.h, csrc/pm_align.hip pm_align_hits_wide_kernel).

The narrow kernel compacts the records of patterns beyond its 32 characters into a list; with the bit set the wide kernel
reads that list on the device and writes the results where the narrow kernel would have, and only what it cannot take
either (65 characters and more) crosses to the host.  Here: records at planted occurrences of primers of 33, 40, 63 and
64 characters (exact, one substitution, one inserted base, one deleted base, a two-base indel run, an edit inside the
exact zone, k + 1 edits, across an end-of-sequence character) and at made-up ends, against the host's re-alignment and
the oracle's; the same in calls of 1, 63, 64, 65 and about 300 records with the long ones first, last and interleaved;
IUPAC letters under -w; count_all on three handles against the count rule on the oracle's hits; a pairing round of
40-mer primer pairs; pm_primer_match -c.  Everywhere the counters say who aligned what."""
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import count_rule
import pcr_cases as PC
import sat_amd
import synth
from oracle import pmoracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")
TABLE = b"ACGT\n"
BASES = "ACGT"
NONE = 2**31 - 1
LONG_LENS = [33, 40, 63, 64] * 3
ZONES3 = [(8, 0), (0, 8), (0, 0)]
SHORT_LENS = [20, 25, 32, 28]
OVER_LENS = [65, 70]


def rand_seq(rng, n):
    return "".join(rng.choice(list(BASES), size=n).tolist())


def other(rng, *avoid):
    return str(rng.choice([c for c in BASES if c not in avoid]))


def sub_at(rng, p, i):
    return p[:i] + other(rng, p[i]) + p[i + 1:]


# ---- the stream, the primers and the records ---------------------------------------------------------------------------
_W = {}


def world():
    """raw stream over ACGT and the end-of-sequence character with every form of every primer planted, and the records"""
    if _W:
        return _W
    rng = np.random.default_rng(6416)
    longp = [rand_seq(rng, L) for L in LONG_LENS]
    shortp = [rand_seq(rng, L) for L in SHORT_LENS]
    overp = [rand_seq(rng, L) for L in OVER_LENS]
    pats = longp + shortp + overp
    zones = [ZONES3[i % 3] for i in range(len(longp))] + [(0, 0)] * (len(shortp) + len(overp))
    raw, sites, planted = ["\n"], [], [0]

    def plant(pid, text, form):
        raw.append(rand_seq(rng, int(rng.integers(25, 41))))
        raw.append(text)
        sites.append((sum(len(x) for x in raw), pid, form))
        planted[0] += 1
        if planted[0] % 9 == 0:
            raw.append(rand_seq(rng, 12) + "\n")

    for i, p in enumerate(longp):
        L, mid, pid = len(p), len(p) // 2, i + 1
        plant(pid, p, "exact")
        plant(pid, sub_at(rng, p, mid), "sub")
        plant(pid, p[:mid] + other(rng, p[mid], p[mid - 1]) + p[mid:], "ins")
        plant(pid, p[:mid] + p[mid + 1:], "del")
        plant(pid, p[:mid] + other(rng, p[mid], p[mid - 1]) * 2 + p[mid:] if i % 2 == 0 else p[:mid] + p[mid + 2:], "run2")
        plant(pid, sub_at(rng, p, L - 3 if zones[i] == (0, 8) else 2), "zone")
        for ne in (2, 3, 4):                                          # k + 1 substitutions for k = 1, 2, 3, outside the zones
            w = p
            for e in range(ne):
                w = sub_at(rng, w, 10 + e * ((L - 20) // ne))
            plant(pid, w, "subs%d" % ne)
        plant(pid, p[:mid] + "\n" + p[mid:], "eos")
    for j, p in enumerate(shortp + overp):
        pid = len(longp) + j + 1
        plant(pid, p, "exact")
        plant(pid, sub_at(rng, p, len(p) // 2), "sub")
    raw.append(rand_seq(rng, 30) + "\n")
    raw = "".join(raw)
    n = len(raw)
    recs = set()
    for end, pid, _ in sites:
        # (the 65- and the 70-mer: only records that have an alignment under every k -- the host call that aligns them writes
        # no strings for a record without one and fails, with the wide kernel as without it)
        recs |= {(end - 1, pid), (end, pid), (end + 1, pid)} if pid <= len(longp) + len(shortp) else {(end, pid)}
    for pid in (1, 2, 3, 4, 13, 15):                                  # made-up records: ends in front of the pattern's length and behind n
        L = len(pats[pid - 1])
        recs |= {(e, pid) for e in (1, 5, L - 2, L, L + 1, L + 3, n, n + 1, n + 2, n + 3)}
    _W.update(raw=raw, n=n, codes=synth.normalize(raw.encode(), TABLE), pats=pats, zones=zones, sites=sites, recs=sorted(recs),
              nlong=len(longp), nshort=len(shortp), want={})
    return _W


def hit_array(pairs):
    h = np.zeros(len(pairs), dtype=sat_amd.HIT_DTYPE)
    if pairs:
        a = np.array(pairs, dtype=np.int64)
        h["end"], h["pid"] = a[:, 0], a[:, 1]
    return h


def handle(w, k, long_align, pats=None, zones=None, wildcards=False, sem=sat_amd.SEM_AUTO, bits=0):
    pm = sat_amd.PatternMatch(k=k, indels=True, semantics=sem, wildcards=wildcards, long_align=long_align, long_edits=bool(bits & 4),
                              long_halves=bool(bits & 8))
    pats = w["pats"] if pats is None else pats
    zones = w["zones"] if zones is None else zones
    for i, p in enumerate(pats):
        pm.add_pattern(p, i + 1, zones[i][0], zones[i][1])
    pm.init(w["codes"], TABLE)
    return pm


def check_against_host(pm, hits, al, ops, txt, what):
    """tests/test_gpu_align_device.py check_against_host: all four fields against pm_align_hits; the strings against
    pm_align_hits_text for every record that has an alignment, two empty strings for the others"""
    host = pm.align_hits(hits)
    for f in ("start", "end", "editdist", "value"):
        bad = np.nonzero(host[f] != al[f])[0]
        assert bad.size == 0, (what, f, hits[bad[0]], host[bad[0]], al[bad[0]])
    has = ~((host["editdist"] == NONE) & (host["start"] == 0) & (host["value"] == 0))
    idx = np.nonzero(has)[0]
    _, hops, htxt = pm.align_hits_text(hits[idx])
    for j, i in enumerate(idx.tolist()):
        assert (ops[i], txt[i]) == (hops[j], htxt[j]), (what, hits[i], al[i], ops[i], hops[j], txt[i], htxt[j])
    for i in np.nonzero(~has)[0].tolist():
        assert (ops[i], txt[i]) == ("", ""), (what, hits[i])
    return int(idx.size)


def info_of(pm):
    return pm.counts()[2]


def lengths_of(w, hits, pats=None):
    pats = w["pats"] if pats is None else pats
    return np.array([len(pats[int(p) - 1]) for p in hits["pid"]])


# ---- 1. records against host and oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_records_against_host_and_oracle(k):
    w = world()
    hits = hit_array(w["recs"])
    lens = lengths_of(w, hits)
    n_over, n_wide = int((lens > 64).sum()), int(((lens > 32) & (lens <= 64)).sum())
    assert n_over == 4 and n_wide >= 300 and int((lens <= 32).sum()) >= 20
    pm = handle(w, k, True)
    try:
        al, ops, txt = pm.align_hits_device_numpy(hits, text=True)
        info = info_of(pm)
        print("k=%d: %d records, %d of 33..64, %d beyond; %s" % (k, hits.size, n_wide, n_over, info))
        assert info["aligned_host"] == n_over                        # (without the wide kernel: n_over + n_wide)
        assert info["aligned_device"] == hits.size - n_over
        assert info["record_bytes_to_host"] == n_over * 16
        check_against_host(pm, hits, al, ops, txt, "k=%d" % k)
    finally:
        pm.close()
    text = O.Text(w["codes"], TABLE)
    kinds = dict(longer=0, shorter=0, none=0, within=0)
    for i, (end, pid) in enumerate(w["recs"]):
        z = w["zones"][pid - 1]
        _, st, en, ed, _ = O.cli_align(text, w["pats"][pid - 1], end, k, True, esb=z[0], eeb=z[1])
        assert (int(al["start"][i]), int(al["end"][i]), int(al["editdist"][i])) == (st, en, ed), (k, end, pid, al[i], (st, en, ed))
        if 32 < lens[i] <= 64:
            kinds["none"] += ed > k
            kinds["within"] += ed <= k
            kinds["longer"] += ed <= k and en - st > lens[i]
            kinds["shorter"] += ed <= k and en - st < lens[i]
    print(kinds)
    for name, cnt in kinds.items():
        assert cnt > 0, (name, kinds)
    # every planted form of a long primer within k re-aligns at its end; k + 1 substitutions and the end-of-sequence form do not
    by = {(e, p): i for i, (e, p) in enumerate(w["recs"])}
    cost = dict(exact=0, sub=1, ins=1, zone=1, run2=2, subs2=2, subs3=3, subs4=4)
    for end, pid, form in w["sites"]:
        if pid > w["nlong"] or form in ("eos", "del"):
            continue
        ed = int(al["editdist"][by[(end, pid)]])
        if form == "zone" and w["zones"][pid - 1] != (0, 0):
            assert ed > k, (form, pid, ed)
        elif cost[form] <= k:
            assert ed == cost[form], (form, pid, k, ed)
        elif form.startswith("subs"):
            assert ed > k, (form, pid, k, ed)
    # the same handle without the bit: identical arrays, and every pattern beyond 32 characters goes through the host
    pm = handle(w, k, False)
    try:
        al0 = pm.align_hits_device_numpy(hits)
        info = info_of(pm)
        assert info["aligned_host"] == n_over + n_wide and info["aligned_device"] == hits.size - n_over - n_wide
        # (the strings: of the records that have an alignment -- on this route the host call that aligns a long pattern's
        # record writes none for a record without one and fails)
        has = np.nonzero(~((al["editdist"] == NONE) & (al["start"] == 0) & (al["value"] == 0)))[0]
        al1, ops1, txt1 = pm.align_hits_device_numpy(hits[has], text=True)
    finally:
        pm.close()
    assert al0.tobytes() == al.tobytes()
    assert al1.tobytes() == al[has].tobytes() and ops1 == [ops[i] for i in has] and txt1 == [txt[i] for i in has]


# ---- 2. shapes ----------------------------------------------------------------------------------------------------------
def test_call_shapes():
    """1, 63, 64, 65 and about 300 records, the long ones first, last and interleaved (the scatter by index across block
    edges), some of the 65- and 70-mer among them, and a call without a long record (every block of the wide kernel exits)"""
    w = world()
    k = 2
    recs = w["recs"]
    nl, ns = w["nlong"], w["nshort"]
    long_pool = [r for r in recs if r[1] <= nl]
    over_pool = [r for r in recs if r[1] > nl + ns] * 4
    short_pool = [r for r in recs if nl < r[1] <= nl + ns] + [(e, nl + 1 + e % ns) for e in range(100, 400)]
    calls = [("one long", long_pool[:1]), ("one short", short_pool[:1]), ("one beyond", over_pool[:1]), ("no long", short_pool[:100])]
    for size in (63, 64, 65, 300):
        a, b = long_pool[:size // 2], short_pool[:size - size // 2]
        mixed = [x for pair in zip(a, b) for x in pair] + b[len(a):]
        calls += [("%d long first" % size, a + b), ("%d long last" % size, b + a), ("%d interleaved" % size, mixed)]
    calls.append(("all long", long_pool[:129]))
    calls.append(("with beyond", [x for t in zip(long_pool[:40], short_pool[:40]) for x in t] + over_pool[:10] + long_pool[40:150] + over_pool[10:14]))
    pm = handle(w, k, True)
    try:
        for what, call in calls:
            hits = hit_array(call)
            lens = lengths_of(w, hits)
            pm.reset()
            al, ops, txt = pm.align_hits_device_numpy(hits, text=True)
            info = info_of(pm)
            assert info["aligned_host"] == int((lens > 64).sum()), (what, info)
            assert info["aligned_device"] == int((lens <= 64).sum()), (what, info)
            check_against_host(pm, hits, al, ops, txt, what)
            al2 = pm.align_hits_device_numpy(hits)                    # without the strings
            assert al2.tobytes() == al.tobytes(), what
    finally:
        pm.close()


# ---- 3. -w ----------------------------------------------------------------------------------------------------------------
def test_iupac_letters():
    rng = np.random.default_rng(6440)
    base = [rand_seq(rng, 40) for _ in range(4)]
    pats, conc = [], []
    for i, p in enumerate(base):
        q = list(p)
        for at, letter in ((11, "R"), (27, "Y"))[:1 + i % 2]:           # one and two IUPAC letters
            q[at] = letter
        pats.append("".join(q))
        c = list(p)
        c[11] = "AG"[i % 2]
        c[27] = "CT"[i % 2] if i % 2 else p[27]
        conc.append("".join(c))
    raw, sites = ["\n"], []
    for i, c in enumerate(conc):
        for form in (c, sub_at(rng, c, 20), c[:20] + other(rng, c[20], c[19]) + c[20:], c[:20] + c[21:], sub_at(rng, c, 11)):
            raw.append(rand_seq(rng, 30) + form)
            sites.append((sum(len(x) for x in raw), i + 1))
    raw = "".join(raw) + rand_seq(rng, 30) + "\n"
    recs = sorted({(e + d, pid) for e, pid in sites for d in (-1, 0, 1)})
    w = dict(codes=synth.normalize(raw.encode(), TABLE), pats=pats, zones=[(0, 0)] * len(pats))
    hits = hit_array(recs)
    pm = handle(w, 2, True, wildcards=True)
    try:
        al, ops, txt = pm.align_hits_device_numpy(hits, text=True)
        info = info_of(pm)
        assert info["aligned_host"] == 0 and info["aligned_device"] == hits.size
        check_against_host(pm, hits, al, ops, txt, "-w")
    finally:
        pm.close()
    assert any("+" in s for s in ops) and any("^" in s for s in ops) and any("v" in s for s in ops)
    text = O.Text(w["codes"], TABLE)
    for i, (end, pid) in enumerate(recs):
        _, st, en, ed, _ = O.cli_align(text, pats[pid - 1], end, 2, True, wildcards=True)
        assert (int(al["start"][i]), int(al["end"][i]), int(al["editdist"][i])) == (st, en, ed), (end, pid, al[i], (st, en, ed))


# ---- 4. counts ------------------------------------------------------------------------------------------------------------
COUNT_SETS = {"edits|align": (4 | 16, 2, sat_amd.SEM_FILTER_BITVEC, O.FILTER_BITVEC), "halves|align": (8 | 16, 1, sat_amd.SEM_EXACT_HALVES, O.EXACT_HALVES_KT),
              "align": (16, 2, sat_amd.SEM_FILTER_BITVEC, O.FILTER_BITVEC)}


def count_want(w, k, eng, with_over):
    key = (k, eng, with_over)
    if key not in w["want"]:
        npat = len(w["pats"]) if with_over else w["nlong"] + w["nshort"]
        pats, zones = w["pats"][:npat], w["zones"][:npat]
        text = O.Text(w["codes"], TABLE)
        hits = O.sorted_tuples(O.find_all(text, pats, engine=eng, k=k, indels=True, esb=[z[0] for z in zones], eeb=[z[1] for z in zones]))
        eds = [O.cli_align(text, pats[pid - 1], end, k, True, esb=zones[pid - 1][0], eeb=zones[pid - 1][1])[3] for end, pid, _ in hits]
        w["want"][key] = (pats, zones, hits, eds)
    return w["want"][key]


@pytest.mark.parametrize("M", [0, 2])
@pytest.mark.parametrize("name", list(COUNT_SETS))
def test_counts(name, M):
    w = world()
    bits, k, sem, eng = COUNT_SETS[name]
    pats, zones, hits, eds = count_want(w, k, eng, False)
    assert len({pid for _, pid, _ in hits if pid <= w["nlong"]}) == w["nlong"] and any(pid > w["nlong"] for _, pid, _ in hits)
    wc, wcap, winfo = count_rule.tally(hits, lambda i: eds[i], len(pats), k, M)
    pm = handle(w, k, True, pats=pats, zones=zones, sem=sem, bits=bits)
    try:
        for chunk in (1 << 30, (w["n"] + 2) // 3, 193):
            counts, capped, info = pm.count_all(max_count=M, chunk=chunk)
            assert counts.tolist() == wc, (name, M, chunk)
            assert capped.tolist() == wcap, (name, M, chunk)
            for f in ("tallied", "skipped", "bogus"):
                assert info[f] == winfo[f], (name, M, chunk, f, info[f], winfo[f])
            assert info["aligned_host"] == 0 and info["aligned_device"] > 0, (name, M, chunk, info)
    finally:
        pm.close()


def test_counts_with_a_70_mer():
    """the 65- and the 70-mer in the list: their hits, and only theirs, are aligned by the host; the tallies are the rule's"""
    w = world()
    bits, k, sem, eng = COUNT_SETS["edits|align"]
    pats, zones, hits, eds = count_want(w, k, eng, True)
    n_over = sum(1 for _, pid, _ in hits if len(pats[pid - 1]) > 64)
    assert n_over >= 2
    wc, wcap, winfo = count_rule.tally(hits, lambda i: eds[i], len(pats), k, 0)
    for chunk in (1 << 30, 193):
        pm = handle(w, k, True, pats=pats, zones=zones, sem=sem, bits=bits)
        try:
            counts, capped, info = pm.count_all(chunk=chunk)
        finally:
            pm.close()
        assert counts.tolist() == wc and capped.tolist() == wcap, chunk
        for f in ("tallied", "skipped", "bogus"):
            assert info[f] == winfo[f], (chunk, f, info[f], winfo[f])
        assert 0 < info["aligned_host"] and info["aligned_device"] > 0, info
        if chunk == 1 << 30:
            assert info["aligned_host"] == n_over, (info, n_over)


# ---- 5. the pairing stage -------------------------------------------------------------------------------------------------
def test_pairing_stage():
    """pm_pcr_scan / pm_pcr_pair under -k 1 with 40-mer primer pairs: the same amplicons and strings with the bit and without;
    with it the round's re-alignment leaves nothing to the host"""
    g = PC.load("pcr_a")
    ents = PC.entries_of(g["fasta"])
    table = synth.table_for(ents)
    raw = synth.stream(ents)
    codes = synth.normalize(raw, table)
    n = len(raw)
    s = raw.decode()
    starts, at = [], 1
    for e in ents:
        starts.append(at)
        at += len(e) + 1
    rng = np.random.default_rng(6450)
    sites = [(starts[0] + 200, starts[0] + 450), (starts[1] + 300, starts[1] + 600), (starts[2] + 100, starts[2] + 220), (starts[2] + 1500, starts[2] + 1560)]
    prim = []
    for j, (a, b) in enumerate(sites):
        assert 100 <= b + 40 - a <= 400
        f, r = s[a:a + 40], s[b:b + 40]
        assert "N" not in f + r and "\n" not in f + r
        if j == 1:
            f = sub_at(rng, f, 17)                                    # one substitution
        if j == 2:
            r = r[:21] + r[22:] + s[b + 40]                           # one deleted base
        prim += [f, r]
    patterns = prim + [synth.revcomp(p) for p in prim]
    got = {}
    for long_align in (True, False):
        pm = sat_amd.PatternMatch(k=1, indels=True, long_align=long_align)
        try:
            for i, p in enumerate(patterns):
                pm.add_pattern(p, i + 1)
            pm.init(codes, table)
            pm.pcr_setup(amplicon_max=420, entry_starts=starts)
            pm.reset()
            before = pm.pcr_stats()
            held = 0
            for begin in range(0, n, 1000):
                held += pm.pcr_scan(begin, min(n, begin + 1000))
            rec, ops, txt = pm.pcr_pair(n, False, text=True)
            after = pm.pcr_stats()
        finally:
            pm.close()
        assert held >= 2 * len(sites)
        grown = after["aligned_host"] - before["aligned_host"]
        if long_align:
            assert grown == 0 and after["aligned_device"] - before["aligned_device"] > 0, (before, after)
        else:
            assert grown > 0, (before, after)
        got[long_align] = (rec.tobytes(), ops, txt, sorted(int(x) for x in rec["pair"]))
    assert got[True] == got[False]
    assert len(set(got[True][3])) == len(sites), got[True][3]


# ---- 6. the command line ----------------------------------------------------------------------------------------------------
def test_primer_match_counts():
    """pm_primer_match -c -k 2 with primers of up to 60 nt: the device's counts with the bit (PM_GPU_LONG=20, 16), without it
    (4) and the caller's own tally loop (PM_GPU_COUNTS=0) write the same bytes -- the reference's, where recorded"""
    pm_bin, cs_bin = os.path.join(HOST, "pm_primer_match"), os.path.join(HOST, "pm_compress_seq")
    assert os.path.exists(pm_bin) and os.path.exists(cs_bin), "run __graft_entry__.build()"
    with open(os.path.join(ROOT, "tests", "golden", "cli_long_edits.json")) as f:
        g = json.load(f)
    assert sum(33 <= len(p) <= 64 for p in g["primers_txt"].split()) >= 10
    c = g["cases"]["k2_counts"]
    assert "-c" in c["options"] and c["options"][c["options"].index("-k") + 1] == "2"
    base = {k: v for k, v in os.environ.items() if k not in ("PM_GPU_LONG", "PM_GPU_COUNTS", "PM_LONG_EDITS", "PM_DEBUG")}
    with tempfile.TemporaryDirectory() as d:
        fa, pf = os.path.join(d, "db.fa"), os.path.join(d, "primers.P")
        with open(fa, "w") as f:
            f.write(g["fasta"])
        with open(pf, "w") as f:
            f.write(g["primers_txt"])
        r = subprocess.run([cs_bin, "-i", fa, "-n", "true"], capture_output=True)
        assert r.returncode == 0, r.stderr
        outs = {}
        for what, env in (("20", dict(PM_GPU_COUNTS="1", PM_GPU_LONG="20")), ("4", dict(PM_GPU_COUNTS="1", PM_GPU_LONG="4")),
                          ("16", dict(PM_GPU_COUNTS="1", PM_GPU_LONG="16")), ("host", dict(PM_GPU_COUNTS="0", PM_GPU_LONG="20"))):
            r = subprocess.run([pm_bin, "-i", fa, "-P", pf] + c["options"], capture_output=True, timeout=300, env=dict(base, **env))
            assert r.returncode == 0, (what, r.stderr[-500:])
            outs[what] = r.stdout
        assert outs["20"] == outs["4"] == outs["16"] == outs["host"]
        got = outs["20"].decode("latin1")
        assert sorted(got.splitlines()) == sorted(c["normalized"].splitlines()) and len(got) == len(c["normalized"])
