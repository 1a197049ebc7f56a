"""GPU: pcr_match's pairing stage in HBM (pm_pcr_setup / pm_pcr_feed / pm_pcr_scan / pm_pcr_pair) through
the C ABI against tests/pcr_rule.py, with the alignments of the library's host re-alignment (align_hits_text).

The stream is pcr_a's (3 entries of 3,000 bases).  The primers are cut from it so that the hit lists hold: an amplicon
that starts at the first base of the stream and one that ends at its last, one over an N run, a pair whose ends lie in two
entries, and a pair of 6 nt primers whose synthetic hit list has more than 1,024 hits of one id and windows of more than
64 partners (the write pass hands those to the whole wave); reverse-complement ids and filler hits have no partner hits
at all.  Lists of 0, 1, 63, 64, 65 and about 3,000 hits, with -a, -b and UniSTS size bounds (one pair's lower bound lies
below -d: the clamp wraps).  Candidate count, survivors, their order, alignments, strings and N counts must be equal."""
import numpy as np
import pytest

import pcr_cases as PC
import pcr_rule as R
import sat_amd
import synth
from sat_amd import pattern_match as P

pytestmark = pytest.mark.gpu
PM_E_INVALID = -1
STRIDE = 64          # bytes per alignment string: the synthetic hits lie anywhere, and what the DP makes of such a place is longer than a real hit's


class World:
    def __init__(self, short_pair=True):
        g = PC.load("pcr_a")
        ents = PC.entries_of(g["fasta"])
        self.table = synth.table_for(ents)
        self.raw = synth.stream(ents)
        self.codes = synth.normalize(self.raw, self.table)
        self.n = len(self.raw)
        self.starts, at = [], 1
        for e in ents:
            self.starts.append(at)
            at += len(e) + 1
        s = self.raw.decode()
        q = s.index("N", self.starts[1] + 200)                        # an N run well inside an entry
        e3 = self.starts[2] + len(ents[2])                            # behind the last base of the stream
        # (forward site start, reverse site start, length): stream indices
        sites = [(1, 301, 20),                                        # the amplicon starts at the stream's first base
                 (e3 - 400, e3 - 20, 20),                             # ... ends at its last
                 (q - 70, q + 40, 20),                                # over the N run
                 (self.starts[0] + 2950, self.starts[1] + 80, 20)]    # the two ends in different entries
        sites.append((self.starts[1] + 1000, self.starts[1] + 1050, 6 if short_pair else 20))
        for a, b, L in sites:
            assert "N" not in s[a:a + L] + s[b:b + L] and "\n" not in s[a:a + L] + s[b:b + L]
        prim = [x for a, b, L in sites for x in (s[a:a + L], s[b:b + L])]
        self.sites = sites
        self.nprim = len(prim)
        self.patterns = prim + [synth.revcomp(p) for p in prim]
        self.nruns = s[q - 70:q + 60].count("N")

    def handle(self, k, indels):
        pm = sat_amd.PatternMatch(k=k, indels=indels)
        for i, p in enumerate(self.patterns):
            pm.add_pattern(p, i + 1)
        pm.init(self.codes, self.table)
        return pm

    def rule(self, k, indels, **o):
        return R.Rule(self.nprim, [0] + [len(p) for p in self.patterns], k, indels, o.get("any_orientation", False), o.get("length_between", False),
                      o.get("amplicon_min", 0), o.get("amplicon_max", 2000), o.get("size_slack", -1), o.get("sizes"))

    def hit_list(self):
        """about 3,000 hits: the planted sites first, then the dense synthetic pair, then filler"""
        rng = np.random.default_rng(77)
        hits = []
        for j, (a, b, L) in enumerate(self.sites):
            hits += [(a + L, 2 * j + 1, 0), (b + L, 2 * j + 2, 0)]
        a, b, L = self.sites[4]
        lo = a - 500
        hits += [(p, 10, 0) for p in range(lo + 50, lo + 1250) if (p, 10, 0) not in hits]          # > 1,024 hits of one id
        hits += [(p, 9, 0) for p in range(lo, lo + 1200, 3) if (p, 9, 0) not in hits]
        seen = set(hits)
        while len(hits) < 3000:                                       # reverse-complement ids and pairs 1..4: hardly any partner in reach
            h = (int(rng.integers(1, self.n)), int(rng.integers(1, 2 * self.nprim + 1)), int(rng.integers(0, 3)))
            if h[1] not in (9, 10) and (h[0], h[1]) not in {(x[0], x[1]) for x in seen}:
                hits.append(h)
                seen.add(h)
        return hits


def to_records(hits):
    a = np.zeros(len(hits), dtype=sat_amd.HIT_DTYPE)
    if hits:
        t = np.array(hits, dtype=np.int64)
        a["end"], a["pid"], a["k"] = t[:, 0], t[:, 1], t[:, 2]
    return a


OPTIONS = {
    "default": dict(amplicon_max=420),
    "allorient": dict(any_orientation=True, amplicon_max=420),
    "between": dict(length_between=True, amplicon_min=10, amplicon_max=390),
    # pair 1's lower bound lies below -d (size_lb - size_slack wraps), pair 5's bounds cut its window
    "sizes": dict(amplicon_max=420, size_slack=30, sizes=[(5, 400), (350, 400), (100, 140), (100, 200), (40, 70)]),
}
CONFIGS = [(2, True), (1, False)]


@pytest.fixture(scope="module")
def worlds():
    """per (k, indels): the handle, the hit list and the host's re-alignment of every hit in it -- computed once, not changed"""
    w = World()
    hits = w.hit_list()
    out = {}
    for k, indels in CONFIGS:
        pm = w.handle(k, indels)
        out[(k, indels)] = (pm, realign(pm, to_records(hits), k))
    yield w, hits, out
    for pm, _ in out.values():
        pm.close()


def realign(pm, recs, k):
    """{(end, pid, k): ((start, end, editdist), alignment string, matching text)} from the host's re-alignment.  The strings
    only where the hit re-aligns within k -- no other hit can be part of a survivor, and where the DP gives up at a row
    (a synthetic hit at a place that does not match at all) there are none to ask for."""
    al = pm.align_hits(recs)
    good = np.flatnonzero((al["editdist"] >= 0) & (al["editdist"] <= k))
    _, ops, txt = pm.align_hits_text(recs[good], stride=STRIDE)
    strings = {int(i): (ops[j], txt[j]) for j, i in enumerate(good)}
    return {(int(recs["end"][i]), int(recs["pid"][i]), int(recs["k"][i])):
            ((int(al["start"][i]), int(al["end"][i]), int(al["editdist"][i])),) + strings.get(i, (None, None)) for i in range(recs.size)}


def setup(pm, w, o):
    lb = ub = None
    if o.get("sizes"):
        lb, ub = [s[0] for s in o["sizes"]], [s[1] for s in o["sizes"]]
    pm.pcr_setup(any_orientation=o.get("any_orientation", False), length_between=o.get("length_between", False),
                 amplicon_min=o.get("amplicon_min", 0), amplicon_max=o.get("amplicon_max", 2000), size_slack=o.get("size_slack", -1),
                 size_lb=lb, size_ub=ub, entry_starts=w.starts)


def check_round(pm, w, rule, res, held, scanned_to, more, text=True):
    """one pm_pcr_pair against the rule on the same held hits; returns (survivors of the rule, carried hits)"""
    before = pm.pcr_stats()
    got = pm.pcr_pair(scanned_to, more, text=text, stride=STRIDE)
    rec, ops, txt = got if text else (got, None, None)
    want, ncand, carried = R.round_survivors(rule, held, scanned_to, more, lambda h: res[h][0], w.starts, w.raw)
    st = pm.pcr_stats()
    assert (st["held"], st["candidates"], st["survivors"]) == (len(held), ncand, len(want))
    assert rec.size == len(want)
    for i, (h, h1, al, al1, alen, pi, nc) in enumerate(want):
        r = rec[i]
        assert (int(r["hit"]["end"][0]), int(r["hit"]["pid"][0]), int(r["hit"]["k"][0])) == h, i
        assert (int(r["hit"]["end"][1]), int(r["hit"]["pid"][1]), int(r["hit"]["k"][1])) == h1, i
        assert not r["hit"]["aux"].any()
        assert (int(r["al"]["start"][0]), int(r["al"]["end"][0]), int(r["al"]["editdist"][0])) == al, i
        assert (int(r["al"]["start"][1]), int(r["al"]["end"][1]), int(r["al"]["editdist"][1])) == al1, i
        assert (int(r["amplicon_len"]), int(r["pair"]), int(r["ncount"])) == (alen, pi, nc), i
        if text:
            assert ops[i] == (res[h][1], res[h1][1]) and txt[i] == (res[h][2], res[h1][2]), i
    # only survivors crossed PCIe: no hit record was copied to the host, none was re-aligned there
    stride = STRIDE
    assert st["aligned_host"] == before["aligned_host"]
    assert st["bytes_to_host"] - before["bytes_to_host"] == len(want) * (P.PCR_AMPLICON_DTYPE.itemsize + (4 * stride if text else 0))
    return want, carried


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("opt", sorted(OPTIONS))
@pytest.mark.parametrize("size", [0, 1, 63, 64, 65, 3000])
def test_feed_and_pair_against_the_rule(worlds, config, opt, size):
    w, hits, per = worlds
    pm, res = per[config]
    o = OPTIONS[opt]
    rule = w.rule(config[0], config[1], **o)
    setup(pm, w, o)
    pm.reset()
    held = hits[:size]
    pm.pcr_feed(to_records(held))
    want, carried = check_round(pm, w, rule, res, held, w.n, False)
    assert carried == []
    assert pm.pcr_pair(w.n, False).size == 0 and pm.pcr_stats()["held"] == 0        # every hit was dropped
    if size == 3000:
        # the list does what the test is about
        l, pairs, _ = R.candidates(rule, held, w.n, False)
        per_hit = {}
        for i, j in pairs:
            per_hit[(i, l[j][1])] = per_hit.get((i, l[j][1]), 0) + 1
        if opt != "sizes":
            assert max(per_hit.values()) > 64 and len(pairs) > 10000
            pinds = {s[5] for s in want}
            assert {1, 2, 3, 5} <= pinds and 4 not in pinds                             # the pair across two entries is not reported
            assert any(s[2][0] == 1 for s in want) and any(s[3][1] == w.n - 1 for s in want)  # the stream's first base, and its last (an alignment's end is the hit's key)
            assert any(s[5] == 3 and s[6] == w.nruns and s[6] > 0 for s in want)         # N's inside an amplicon
            # (the dense pair's 6 nt primers: -k 2 re-aligns about a tenth of all places within k, -K 1 one in two hundred)
            assert sum(1 for s in want if s[5] == 5) > (50 if config[1] else 0)
        else:
            # pair 1's wrapped lower bound reads as a negative window start: the pair is still found; pair 5 within 40 - 30 .. 70 + 30
            assert 1 in {s[5] for s in want} and all(10 <= s[4] <= 100 for s in want if s[5] == 5)


@pytest.mark.parametrize("config", CONFIGS)
@pytest.mark.parametrize("opt", ["default", "between"])
def test_three_rounds(worlds, config, opt):
    """the same hits fed in three rounds with more = 1, 1, 0: deferred hits stay held and pair later, also as partners of
    hits that come behind them"""
    w, hits, per = worlds
    pm, res = per[config]
    o = OPTIONS[opt]
    rule = w.rule(config[0], config[1], **o)
    setup(pm, w, o)
    pm.reset()
    cuts = [(0, 4300, 1), (4300, 4700, 1), (4700, w.n, 0)]               # the middle cuts run through the dense pair
    held, total, deferred = [], [], 0
    for lo, hi, more in cuts:
        new = [h for h in hits if lo < h[0] <= hi]
        pm.pcr_feed(to_records(new))
        held = held + new
        want, held = check_round(pm, w, rule, res, held, hi, more, text=(more == 0))
        deferred += len(held)
        total += want
    assert held == [] and deferred > 100
    one, _, _ = R.round_survivors(rule, hits, w.n, False, lambda h: res[h][0], w.starts, w.raw)
    assert sorted(PC.line_of(s) for s in total) == sorted(PC.line_of(s) for s in one)


def test_reset_empties_the_held_list(worlds):
    w, hits, per = worlds
    pm, _ = per[CONFIGS[0]]
    setup(pm, w, OPTIONS["default"])
    pm.reset()
    pm.pcr_feed(to_records(hits[:100]))
    pm.reset()
    assert pm.pcr_pair(w.n, False).size == 0
    st = pm.pcr_stats()
    assert st["held"] == 0 and st["bytes_to_host"] == 0
    with pytest.raises(sat_amd.PmError) as e:
        pm.pcr_feed(to_records([(5, 2 * w.nprim + 1, 0)]))              # an id the handle does not have
    assert e.value.code == PM_E_INVALID


@pytest.fixture(scope="module")
def scan_world():
    """20 nt primers only, the lists pm_pcr_match scans: handles for pcr_scan and for find_all"""
    w = World(short_pair=False)
    pms = {c: w.handle(*c) for c in CONFIGS}
    yield w, pms
    for pm in pms.values():
        pm.close()


@pytest.mark.parametrize("config", CONFIGS)
def test_scan_equals_feed_of_the_scanned_hits(scan_world, config):
    w, pms = scan_world
    pm = pms[config]
    o = OPTIONS["default"]
    setup(pm, w, o)
    found = pm.find_all()
    hits = sorted(zip(found["end"].tolist(), found["pid"].tolist(), found["k"].tolist()))
    assert len(hits) >= 8
    res = realign(pm, found, config[0])
    rule = w.rule(config[0], config[1], **o)
    pm.reset()
    pm.pcr_feed(found)
    want, _ = check_round(pm, w, rule, res, hits, w.n, False)
    assert {s[5] for s in want} >= {1, 2, 3}
    pm.reset()
    got = 0
    for begin in range(0, w.n, 1000):
        got += pm.pcr_scan(begin, min(w.n, begin + 1000))
    assert got == len(hits)
    want2, _ = check_round(pm, w, rule, res, hits, w.n, False)
    assert want2 == want
    # ... and round by round, a round per range: the same amplicons
    pm.reset()
    total = []
    for begin in range(0, w.n, 1000):
        end = min(w.n, begin + 1000)
        pm.pcr_scan(begin, end)
        rec = pm.pcr_pair(end, end < w.n)
        total += [(int(r["pair"]), int(r["al"]["start"][0]), int(r["al"]["end"][0]), int(r["al"]["start"][1]), int(r["al"]["end"][1]),
                   int(r["al"]["editdist"][0]), int(r["al"]["editdist"][1]), int(r["al"]["end"][1] - r["al"]["start"][0]), int(r["ncount"])) for r in rec]
    assert sorted(total) == sorted(PC.line_of(s) for s in want)


def test_modes_do_not_mix(scan_world):
    w, pms = scan_world
    pm = pms[CONFIGS[0]]
    setup(pm, w, OPTIONS["default"])
    pm.reset()
    pm.pcr_scan(0, 1000)
    buf = np.zeros(16, dtype=sat_amd.HIT_DTYPE)
    for call in (lambda: pm.scan(1000, 2000, buf), lambda: pm.scan_view(1000, 2000), lambda: pm.count_scan(1000, 2000)):
        with pytest.raises(sat_amd.PmError) as e:
            call()
        assert e.value.code == PM_E_INVALID
    assert pm.pcr_scan(1000, 2000) >= 0                                  # the refused calls changed nothing
    pm.reset()
    pm.scan_view(0, 1000)
    with pytest.raises(sat_amd.PmError) as e:
        pm.pcr_scan(1000, 2000)
    assert e.value.code == PM_E_INVALID
    pm.reset()
    pm.count_scan(0, 1000)
    with pytest.raises(sat_amd.PmError) as e:
        pm.pcr_scan(1000, 2000)
    assert e.value.code == PM_E_INVALID
    pm.reset()


def test_setup_on_a_windowed_handle_is_unsupported(scan_world):
    w, _ = scan_world
    pm = sat_amd.PatternMatch(k=1)
    for i, p in enumerate(w.patterns):
        pm.add_pattern(p, i + 1)
    pm.init(w.codes, w.table, window=4096)
    with pytest.raises(sat_amd.PmError) as e:
        setup(pm, w, OPTIONS["default"])
    assert e.value.code == -2
    pm.close()
