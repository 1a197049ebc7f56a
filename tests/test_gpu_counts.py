"""GPU: pm_count_scan / pm_counts -- the caller's tally loop (`primer_match -c [-M max]`) on the device.

The expected tallies are built without the product: the ORACLE's hits (adversarial.oracle_hits), the oracle's
re-alignment (pmoracle.cli_align) and the rule of tests/count_rule.py.  The library's hits come from its own scan, so
every case is also a parity run of the scan."""
import os

import numpy as np
import pytest

import sat_amd
import adversarial as A
import count_rule
from oracle import pmoracle as O

pytestmark = pytest.mark.gpu

SEEDS = range(300)
_EXPECT = {}


def expected(c, M):
    """(counts, capped, info) of the case under max_count M, from the oracle alone"""
    key = (c["seed"], M)
    if key not in _EXPECT:
        if ("hits", c["seed"]) not in _EXPECT:
            hits = A.oracle_hits(c)
            assert hits is not None, "seed %d: the reference rejects the option set" % c["seed"]
            text = O.Text(c["stream"], c["table"])
            eds = []
            for end, pid, _ in hits:
                z = c["zones"][pid - 1] if c["zones"] else (0, 0)
                eds.append(O.cli_align(text, c["patterns"][pid - 1], end, c["k"], c["indels"], esb=z[0], eeb=z[1], wildcards=c["wild"])[3])
            _EXPECT[("hits", c["seed"])] = (hits, eds)
        hits, eds = _EXPECT[("hits", c["seed"])]
        _EXPECT[key] = count_rule.tally(hits, lambda i: eds[i], len(c["patterns"]), c["k"], M)
    return _EXPECT[key]


def handle(c, window=None, host_only=False):
    import torch
    with A.knobs(c["env"]):
        pm = sat_amd.PatternMatch(k=c["k"], indels=c["indels"], semantics=c["sem"], wildcards=c["wild"])
    for i, p in enumerate(c["patterns"]):
        z = c["zones"][i] if c["zones"] else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    if host_only:
        pm.init_host(c["stream"], c["table"])
    elif window is not None:
        pm.init(c["stream"], c["table"], window=window)
    elif c["host"]:
        pm.init(c["stream"], c["table"])
    else:
        dev = torch.from_numpy(c["stream"]).cuda()
        pm.init_device(dev.data_ptr(), c["n"], c["table"], keepalive=dev)
    if not host_only:
        pm.set_capacity(c["cap"])
    return pm


def check(c, M, got, what, device_route=True, want=None, describe=A.describe):
    """want: the expectation where it does not come from expected() (another generator's case); device_route None: the case
    decides where its records are re-aligned, and the caller checks that"""
    counts, capped, info = got
    wc, wcap, winfo = want or expected(c, M)
    ctx = (what, "M", M, describe(c))
    print("counts %s M %d seed %d: tallied %d skipped %d bogus %d aligned device/host %d/%d record bytes to host %d" % (
        what, M, c["seed"], info["tallied"], info["skipped"], info["bogus"], info["aligned_device"], info["aligned_host"], info["record_bytes_to_host"]))
    assert counts.shape == (len(c["patterns"]), c["k"] + 1)
    assert counts.tolist() == wc, ctx
    assert capped.tolist() == wcap, ctx
    for f in ("tallied", "skipped", "bogus"):
        assert info[f] == winfo[f], ctx + (f, info[f], winfo[f])
    assert info["first_bogus"] == winfo["first_bogus"], ctx
    # every hit that was not skipped was re-aligned somewhere; on a resident handle with primers of <= 32 characters nearly all on the device
    assert info["aligned_device"] + info["aligned_host"] >= info["tallied"] + info["bogus"], ctx
    if device_route:                                              # resident stream, primers of <= 32 characters, k <= 3: no quiet way round the kernel
        assert info["aligned_host"] == 0, ctx
    elif device_route is not None:
        assert info["aligned_device"] == 0, ctx


def walk(pm, c, ends, M):
    pm.reset()
    pos = 0
    for e in ends:
        e = min(int(e), c["n"])
        if e > pos:
            pm.count_scan(pos, e, M)
            pos = e
    return pm.counts()


@pytest.mark.parametrize("block", range(10))
def test_counts_of_adversarial_seeds(block):
    """count_all, three ranges and ranges of 193 positions, M in {0, 1, 3}, one handle per seed (pm_reset between)"""
    for seed in SEEDS[30 * block:30 * block + 30]:
        c = A.small_case(seed)
        pm = handle(c)
        try:
            n = c["n"]
            for M in (0, 1, 3):
                check(c, M, pm.count_all(max_count=M), "count_all")
                check(c, M, walk(pm, c, (n // 3, 2 * (n // 3), n), M), "three ranges")
                check(c, M, walk(pm, c, list(range(193, n, 193)) + [n], M), "ranges of 193")
            pm.reset()                                              # pm_reset clears
            counts, capped, info = pm.counts()
            assert int(counts.sum()) == 0 and int(capped.sum()) == 0 and info["tallied"] == info["skipped"] == info["bogus"] == 0
        finally:
            pm.close()


@pytest.mark.parametrize("block", range(10))
def test_counts_with_ranges_cut_by_the_library(block, monkeypatch):
    """PM_DENSE_BOUND=400: the library scans a range in pieces (pm_api.cpp scan_range); the tallies accumulate over them"""
    for seed in SEEDS[30 * block:30 * block + 30]:
        c = A.small_case(seed)
        for bound in (400, 6000, 400000):                           # (a case with several records per position cannot get below 400 in a piece of 256 positions)
            monkeypatch.setenv("PM_DENSE_BOUND", str(bound))
            pm = handle(c)
            try:
                got = {M: pm.count_all(max_count=M) for M in (0, 3)}
                break
            except sat_amd.PmError as e:
                if e.code != -2 or "smaller ranges" not in str(e) or bound == 400000:
                    raise
            finally:
                pm.close()
        for M in (0, 3):
            check(c, M, got[M], "pieces")


@pytest.mark.parametrize("block", range(10))
def test_counts_on_a_windowed_handle(block):
    """pm_init_windowed: the stream is not in HBM as a whole, the re-alignment runs on the host, the tallies are the same"""
    for seed in SEEDS[30 * block:30 * block + 30]:
        c = A.small_case(seed)
        pm = handle(c, window=1024)
        try:
            for M in (0, 3):
                check(c, M, pm.count_all(max_count=M, chunk=700), "windowed", device_route=False)
        finally:
            pm.close()


def test_call_order():
    c = A.small_case(5)
    pm = handle(c)
    try:
        n = c["n"]
        pm.reset()
        pm.scan_view(0, n // 2)
        with pytest.raises(sat_amd.PmError) as e:                   # pm_scan, then pm_count_scan
            pm.count_scan(n // 2, n)
        assert e.value.code == -1
        pm.reset()
        pm.count_scan(0, n // 2, 3)
        with pytest.raises(sat_amd.PmError) as e:                   # pm_count_scan, then pm_scan
            pm.scan_view(n // 2, n)
        assert e.value.code == -1
        with pytest.raises(sat_amd.PmError) as e:                   # max_count changes
            pm.count_scan(n // 2, n, 4)
        assert e.value.code == -1
        with pytest.raises(sat_amd.PmError) as e:                   # ranges must be consecutive
            pm.count_scan(n // 2 + 5, n, 3)
        assert e.value.code == -1
        pm.count_scan(n // 2, n, 3)
        check(c, 3, pm.counts(), "after refused calls")
    finally:
        pm.close()
    ho = handle(c, host_only=True)                                  # a pm_init_host handle has no scan of any kind
    try:
        with pytest.raises(sat_amd.PmError) as e:
            ho.count_scan(0, c["n"])
        assert e.value.code == -1
    finally:
        ho.close()


def oracle_run_tally(unit, reps, k, indels, engine, M):
    """the oracle alone on `unit` x reps with the one primer: (row of the primer, info, number of hits)"""
    own = {"A": "A" * 20, "AC": "AC" * 10}[unit]
    text = O.Text(np.tile(np.array(["ACGT".index(x) for x in unit], dtype=np.uint8), reps), b"ACGT\n")
    eng = O.pick_engine(text, [own], k, indels) if engine is None else engine
    hits = O.sorted_tuples(O.find_all(text, [own], engine=eng, k=k, indels=indels))
    eds = [O.cli_align(text, own, end, k, indels)[3] for end, _, _ in hits]
    counts, capped, info = count_rule.tally(hits, lambda i: eds[i], 1, k, M)
    return np.array(counts[0], dtype=np.int64), capped[0], info, len(hits)


@pytest.mark.parametrize("unit,reps", [("A", 200000), ("AC", 100000)])
@pytest.mark.parametrize("k,indels,sem", [(0, False, sat_amd.SEM_AUTO), (2, False, sat_amd.SEM_AUTO), (2, True, sat_amd.SEM_AUTO),
                                          (2, False, sat_amd.SEM_SHIFT_AND_INEXACT), (2, True, sat_amd.SEM_SHIFT_AND_INEXACT)])
def test_one_pattern_owns_the_range(unit, reps, k, indels, sem):
    """A x 200000 and (AC) x 100000 with the primers A x 20 and (AC) x 10 among 1000 random ones.  k = 0 and the bare
    k-error automaton (shift_and_inexact.cc:249-352 reports every end position) give ONE id a hit at every (second)
    position -- the case the tally kernels' block tables are for; filter_bitvec (-K 2 / -k 2 by itself) chains
    candidates that lie within 2k + 1 of each other (filter_bitvec.cc:103-116): the whole run is one chain and one hit.

    Closed form, without the product: the stream is periodic, so the tallies are those of its two edges plus a constant
    per period.  The oracle (find_all + cli_align + tests/count_rule.py) gives the tallies of the same text at 1000 and
    2000 periods; their difference is 1000 periods' worth, and the tallies at the full length follow by adding whole
    thousands of periods.  Under M = 1000 the first 1000 tallied hits of the id lie inside the first 2000 periods (a period
    that tallied nothing would tally nothing anywhere), so the row and the cap are the oracle's at 2000 periods, and
    what is skipped grows by the hits of the further periods.  For M = 0 also equal to find_all + align_hits on the host."""
    rng = np.random.default_rng(len(unit) * 10 + k)
    n = len(unit) * reps
    stream = np.tile(np.array(["ACGT".index(x) for x in unit], dtype=np.uint8), reps)
    pats = ["".join("ACGT"[x] for x in rng.integers(0, 4, 20)) for _ in range(1000)]
    pats = [p for p in pats if len(set(p)) > 2]                      # (nothing near a homopolymer or a dinucleotide repeat)
    own = {"A": "A" * 20, "AC": "AC" * 10}[unit]
    pats.insert(417, own)
    own_idx = 417
    chained = k > 0 and sem == sat_amd.SEM_AUTO
    engine = None if sem == sat_amd.SEM_AUTO else O.SHIFT_AND_INEXACT
    assert (reps - 2000) % 1000 == 0
    more = (reps - 2000) // 1000                                     # further thousands of periods
    for M in (0, 1000):
        row_a, _, info_a, hits_a = oracle_run_tally(unit, 1000, k, indels, engine, M)
        row_b, cap_b, info_b, hits_b = oracle_run_tally(unit, 2000, k, indels, engine, M)
        if M == 0:
            want_row = row_b + more * (row_b - row_a)
            want = dict(tallied=info_b["tallied"] + more * (info_b["tallied"] - info_a["tallied"]), skipped=0,
                        bogus=info_b["bogus"] + more * (info_b["bogus"] - info_a["bogus"]))
            want_cap = 0
        else:
            want_row, want_cap = row_b, cap_b
            want = dict(tallied=info_b["tallied"], skipped=info_b["skipped"] + more * (hits_b - hits_a), bogus=info_b["bogus"])
            assert chained or (int(row_b.sum()) == M and cap_b == 1)       # (the cap is met well inside 2000 periods)
        pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sem)
        try:
            for i, p in enumerate(pats):
                pm.add_pattern(p, i + 1)
            pm.init(stream, b"ACGT\n")
            if chained:
                assert pm.selected()[0] == sat_amd.SEM_FILTER_BITVEC
            counts, capped, info = pm.count_all(max_count=M, chunk=1 << 16)
            print("one pattern owns the range: %s k %d indels %d sem %d M %d: %s, row %s, expected %s %s" % (unit, k, indels, sem, M, info, counts[own_idx].tolist(), want_row.tolist(), want))
            assert counts[own_idx].tolist() == want_row.tolist()
            assert int(counts.sum()) == int(counts[own_idx].sum())           # the random primers have no hit in such text
            assert capped.tolist() == [int(i == own_idx and want_cap) for i in range(len(pats))]
            for f in ("tallied", "skipped", "bogus"):
                assert info[f] == want[f], (f, info[f], want[f])
            assert info["aligned_host"] == 0
            if chained:                                              # one chain, one hit, whatever the cap
                assert counts[own_idx].tolist() == [1, 0, 0]
            if k == 0:
                exact = n - 19 if unit == "A" else (n - 20) // 2 + 1
                assert counts[own_idx].tolist() == [M or exact]
            if M == 0:
                hits = pm.find_all()
                al = pm.align_hits(hits)
                host = np.zeros_like(counts)
                ok = al["editdist"] <= k
                np.add.at(host, (hits["pid"][ok].astype(np.int64) - 1, al["editdist"][ok].astype(np.int64)), 1)
                assert counts.tolist() == host.tolist()
        finally:
            pm.close()
