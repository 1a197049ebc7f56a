"""GPU: pm_scan / pm_scan_view enqueue the scan of the range they expect next before the host has collected the current
range's hits (finalize_sync in csrc/pm_api.cpp).  That look-ahead scan refills the record buffer from slot 0,
so every landing source must be out of its way.  Expected values come from the oracle, or from the closed form of the dense
stream that tests/test_dense_closed_form.py pins to the oracle; pm_scan_stats' `lookahead` proves that the situation occurred.

The dense tests use ranges of R = 2^21 characters.  Measured on an MI355X with scripts/lookahead_scan_time.py (ids 1, 2; scan
= pm_last_kernel_time of one range, best of three; copy = the range's 16-byte records over a 64 GB/s link, a lower bound):

    option set            records/range   scan      copy >=    at R = 2^23: scan, copy >=
    k0 (pm_seed_scan)     2,097,152       25.9 ms   0.52 ms    100.7 ms, 2.10 ms
    inexact_K1 (pair)     2,097,152       0.50 ms   0.52 ms    0.74 ms, 2.10 ms
    inexact_k1 (edits)    4,194,304       3.37 ms   1.05 ms    9.58 ms, 4.19 ms
    bases_K1 (pair)       2,097,152       0.50 ms   0.52 ms    0.74 ms, 2.10 ms

So the copy is NOT ten times the scan for any option set at any R up to 2^23 (2.8 times at best): on this stream, where
every position is a hit, the scans are far slower than on ordinary text.  The overlap does not need that ratio.  The
look-ahead is enqueued before the copy to the host begins and starts to refill the record buffer from slot 0 at once, so a
copy out of that buffer is overtaken as soon as it takes longer than the scan's first writes, and 32 MB take >= 0.5 ms.
Shown once: with the landing of the unsorted case put back as it was (copy from the record buffer behind the look-ahead)
all eight cases with ids (2, 1) and (7, 7) fail in the first walk with "hits of a later range" -- range (0, 2^21] came back
holding ends of (2^21, 2^22], wholly for the fast scans and in part for k0 -- and the four cases with ids (1, 2), the
device-sorted control, pass."""
import numpy as np
import pytest

import count_rule
import dense_stream as D
import synth
import sat_amd
from oracle import pmoracle as O
from test_gpu_windowed import min_window

pytestmark = pytest.mark.gpu

R = 1 << 21


def fields(v):
    return v["end"].astype(np.int64), v["pid"].astype(np.int64), v["k"].astype(np.int64)


def in_order(end, pid, k):
    """(end, pid, k) order: a stable sort of a sorted list moves nothing"""
    return np.array_equal(np.lexsort((k, pid, end)), np.arange(end.size))


def walk_view(pm, ranges):
    return [pm.scan_view(b, e).copy() for b, e in ranges]


def walk_scan(pm, ranges, cap=65536):
    """pm_scan with a small `out` buffer: the `more` loop of find_patterns(chunk=R)"""
    out = np.zeros(cap, dtype=sat_amd.HIT_DTYPE)
    spans = []
    for b, e in ranges:
        n, more = pm.scan(b, e, out)
        parts = [out[:n].copy()]
        while more:
            n, more = pm.scan(e, e, out)
            parts.append(out[:n].copy())
        spans.append(np.concatenate(parts))
    return spans


def equal_ranges(n, step):
    return [(b, min(n, b + step)) for b in range(0, n, step)]


def irregular_ranges(r):
    """r, r/2, 3r/2, r: the guess of the next range is wrong twice (the unused scan is drained), then right again"""
    cuts = [0, r, r + r // 2, 3 * r, 4 * r]
    return list(zip(cuts[:-1], cuts[1:]))


def check_walk(spans, ranges, n, want, reach, min_records, tag, deferring=False):
    """every range's span in (end, pid, k) order and not beyond the range; the spans together are `want` (three arrays in that
    order).  deferring: an engine that may hand a hit out one range later (filter_bitvec.cc:118-121: a cluster that can
    still grow waits), so only each call's span is in order (include/pm_gpu.h, pm_scan) and the whole is compared sorted."""
    for (b, e), v in zip(ranges, spans):
        end, pid, k = fields(v)
        assert end.size >= min_records, (tag, b, e, end.size)
        assert in_order(end, pid, k), (tag, b, e, "not in (end, pid, k) order")
        if end.size:
            # a copy that the next range's scan overwrote holds that range's records
            hi = e if e < n else n + reach
            assert end.max() <= hi, (tag, b, e, int(end.min()), int(end.max()), "hits of a later range")
    got = fields(np.concatenate(spans))
    if deferring:
        o = np.lexsort((got[2], got[1], got[0]))
        got = tuple(g[o] for g in got)
    for g, w, name in zip(got, want, ("end", "pid", "k")):
        assert g.size == w.size, (tag, name, g.size, w.size)
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError((tag, name, "first difference at hit", at, int(g[at]), int(w[at])))


# ---- (b) passthrough landing on the dense stream ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def dense_codes():
    return D.codes(4 * R)


@pytest.mark.parametrize("ids", D.IDS, ids=lambda t: "ids%d_%d" % t)
@pytest.mark.parametrize("name", list(D.OPTION_SETS))
def test_passthrough_landing_under_the_lookahead_scan(name, ids, dense_codes):
    """One range's hits take >= 0.5 ms to cross to the host and the next range's scan, enqueued before that copy, refills the
    record buffer from slot 0 meanwhile: a landing that copies from that buffer behind the look-ahead comes back holding the
    next range's records (seen in all eight unsorted cases, see the module docstring)."""
    kw, _, zone = D.OPTION_SETS[name]
    n = dense_codes.size
    want = D.expected(name, ids, n)
    pm = sat_amd.PatternMatch(**kw)
    for p, i in zip(D.PATTERNS, ids):
        pm.add_pattern(p, i, zone, 0)
    pm.init(dense_codes, D.TABLE)
    if name == "bases_K1":                                            # the flagged-records form (exact_bases -K on the seed family): the records are the final hits
        assert pm.selected()[1] == sat_amd.KERNEL_SEED and pm.describe().startswith(("kernel=pm_pair_scan", "kernel=pm_seed_scan")), pm.describe()
    for walk, ranges, grow in (("view", equal_ranges(n, R), 3), ("scan", equal_ranges(n, R), 3), ("irregular", irregular_ranges(R), 2)):
        pm.reset()
        before = pm.scan_stats()["lookahead"]
        spans = (walk_scan if walk == "scan" else walk_view)(pm, ranges)
        ahead = pm.scan_stats()["lookahead"] - before
        assert ahead >= grow, (name, ids, walk, ahead)
        check_walk(spans, ranges, n, want, 32, R // 2, (name, ids, walk))
    pm.close()


# ---- (c) every landing source on ordinary text -------------------------------------------------------------------------

TEXT_LEN = 2 ** 18
STEP = 2 ** 15
# name -> (k, indels, semantics, oracle engine (None: the automatic choice), exact_start_bases, short primers mixed in)
TEXT_SETS = {
    "k0": (0, True, sat_amd.SEM_AUTO, None, 0, False),
    "K2": (2, False, sat_amd.SEM_AUTO, None, 0, False),
    "k2_cluster_dp": (2, True, sat_amd.SEM_AUTO, None, 0, False),
    "k1_short_class": (1, True, sat_amd.SEM_FILTER_BITVEC, O.FILTER_BITVEC, 0, True),
    "halves_K1_host_stage": (1, False, sat_amd.SEM_EXACT_HALVES, O.EXACT_HALVES_KT, 0, False),
    "bases_K1": (1, False, sat_amd.SEM_EXACT_BASES, O.EXACT_BASES_KT, 4, False),
}
ID_KINDS = ("ascending", "reversed", "strands_share")
_TEXT = {}


def ordinary_text(short):
    """(codes, table, primers of both strands): built once per kind and left alone"""
    if short not in _TEXT:
        rng = np.random.default_rng(2024)
        ents = synth.make_entries(rng, 3, TEXT_LEN, n_runs=2, repeats=True)
        fwd = synth.make_patterns(rng, ents, 400, length=22, planted=1.0, extras=False)
        if short:
            fwd = fwd[:300] + synth.make_patterns(rng, ents, 100, length=19, minlen=16, planted=1.0, extras=False)
        table = synth.table_for(ents)
        _TEXT[short] = (synth.normalize(synth.stream(ents), table), table, fwd + [synth.revcomp(p) for p in fwd])
    return _TEXT[short]


def make_ids(kind, npat):
    half = npat // 2
    if kind == "ascending":
        return list(range(1, npat + 1))
    if kind == "reversed":
        return list(range(npat, 0, -1))
    return list(range(1, half + 1)) * 2                                # the reverse strand under its forward primer's id


def text_handle(name, pats, ids, codes, table, kind):
    k, indels, sem, _, zone, _ = TEXT_SETS[name]
    pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sem)
    for p, i in zip(pats, ids):
        pm.add_pattern(p, i, zone, 0)
    if kind == "resident":
        pm.init(codes, table)
        return pm
    # a window that holds a range (a range in pieces has no look-ahead) and is a small part of the stream
    window = max(min_window(pats, k, indels, sem=sem, zones=[(zone, 0)] * len(pats)), 4 * STEP)
    if kind == "windowed":
        pm.init(codes, table, window=window)
    else:
        pm.init_packed(sat_amd.pack_codes(codes, 3), 3, codes.size, table, window=window)
    return pm


@pytest.mark.parametrize("id_kind", ID_KINDS)
@pytest.mark.parametrize("name", list(TEXT_SETS))
def test_every_landing_source_in_ranges_vs_oracle(name, id_kind):
    k, indels, sem, eng, zone, short = TEXT_SETS[name]
    codes, table, pats = ordinary_text(short)
    n = codes.size
    ids = make_ids(id_kind, len(pats))
    text = O.Text(codes, table)
    if eng is None:
        eng = O.pick_engine(text, pats, k, indels)
    h = O.find_all(text, pats, engine=eng, k=k, indels=indels, ids=ids, esb=[zone] * len(pats) if zone else None)
    we, wp, wk = fields(h)
    o = np.lexsort((wk, wp, we))
    want = (we[o], wp[o], wk[o])
    assert want[0].size > 200, (name, want[0].size)
    r = 4 * STEP
    irregular = irregular_ranges(r) + equal_ranges(n, r)[4:]
    for kind in ("resident", "windowed", "packed_windowed"):
        pm = text_handle(name, pats, ids, codes, table, kind)
        for walk, ranges in (("equal", equal_ranges(n, STEP)), ("irregular", irregular)):
            pm.reset()
            before = pm.scan_stats()["lookahead"]
            spans = walk_view(pm, ranges)
            ahead = pm.scan_stats()["lookahead"] - before
            check_walk(spans, ranges, n, want, 64, 0, (name, id_kind, kind, walk), deferring=k > 0)
            if name == "halves_K1_host_stage":
                assert ahead == 0, (name, kind, walk, ahead)            # the control: a host finalize stage enqueues nothing
            elif kind == "resident" or walk == "equal":                 # (a window holds four of the equal ranges: none is cut into pieces)
                assert ahead >= 3, (name, id_kind, kind, walk, ahead, pm.describe())
        if kind != "resident":
            res = pm.residency()
            assert res["window"] > 0 and res["loads"] > 1, res
        pm.close()


# ---- (d) a look-ahead scan nobody collects -----------------------------------------------------------------------------

_SMALL = {}


def small_case(k=0, indels=True, ids_reversed=True):
    """(a fresh handle, its stream, patterns and ids, the oracle's hits: computed once)"""
    codes, table, pats = ordinary_text(False)
    ids = make_ids("reversed" if ids_reversed else "ascending", len(pats))
    if (k, indels, ids_reversed) not in _SMALL:
        text = O.Text(codes, table)
        eng = O.FILTER_BITVEC if k else O.pick_engine(text, pats, k, indels)
        _SMALL[(k, indels, ids_reversed)] = O.find_all(text, pats, engine=eng, k=k, indels=indels, ids=ids)
    h = _SMALL[(k, indels, ids_reversed)]
    pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sat_amd.SEM_FILTER_BITVEC if k else sat_amd.SEM_AUTO)
    for p, i in zip(pats, ids):
        pm.add_pattern(p, i)
    pm.init(codes, table)
    return pm, codes, table, pats, ids, h


def two_ranges_then(pm):
    """leaves the scan of (2 STEP, 3 STEP] enqueued and returns the look-ahead count from before.  pm_scan_stats waits for a
    look-ahead in flight, so the caller reads the count (it survives pm_reset) only after the call it is about: enqueued(pm, before)"""
    pm.reset()
    before = pm.scan_stats()["lookahead"]
    pm.scan_view(0, STEP)
    pm.scan_view(STEP, 2 * STEP)
    return before


def enqueued(pm, before):
    assert pm.scan_stats()["lookahead"] - before == 2, (pm.scan_stats(), before)


@pytest.mark.parametrize("k,indels", [(0, True), (2, True)])
def test_abandoned_lookahead_reset_and_direct_calls(k, indels):
    pm, codes, table, pats, ids, h = small_case(k, indels)
    n = codes.size
    want = O.sorted_tuples(h)
    # pm_reset, then the whole stream in one range
    before = two_ranges_then(pm)
    pm.reset()
    enqueued(pm, before)
    assert sat_amd.sorted_tuples(pm.scan_view(0, n)) == want
    # a direct scan of an unrelated range and its device finalize stage
    before = two_ranges_then(pm)
    lo, hi = 5 * STEP + 123, 7 * STEP + 7
    cnt = pm.scan_candidates(lo, hi, to_host=False)
    enqueued(pm, before)
    assert pm.candidates_device()[1] == cnt
    got = sat_amd.sorted_tuples(pm.finalize_device(hi, last=False))
    if k == 0:                                                          # the records are the hits
        assert got == [t for t in want if lo < t[0] <= hi]
    else:                                                               # clusters at the edges wait for more text: the decided ones are the oracle's
        inside = lambda ts: [t for t in ts if lo + 64 < t[0] <= hi - 64]
        assert inside(got) == inside(want) and len(inside(want)) > 10, (len(inside(got)), len(inside(want)))
    # and the handle is unharmed
    pm.reset()
    assert sat_amd.sorted_tuples(pm.find_all(chunk=STEP)) == want
    pm.close()


def test_abandoned_lookahead_count_all():
    k = 1
    pm, codes, table, pats, ids, h = small_case(k, True, ids_reversed=False)
    before = two_ranges_then(pm)
    counts, capped, info = pm.count_all(max_count=0)
    enqueued(pm, before)
    pm.close()
    text = O.Text(codes, table)
    hits = O.sorted_tuples(h)                                         # (ids 1..N: id - 1 is the pattern's index)
    eds = [O.cli_align(text, pats[pid - 1], end, k, True)[3] for end, pid, _ in hits]
    want, _, winfo = count_rule.tally(hits, lambda i: eds[i], len(pats), k, 0)
    assert np.array_equal(counts, np.array(want, dtype=np.uint64)), (int(counts.sum()), int(np.sum(want)))
    assert info["tallied"] == winfo["tallied"] > 200 and info["bogus"] == winfo["bogus"], (info, winfo)


def test_candidates_device_under_a_lookahead():
    """after a pm_scan_view that left a look-ahead scan in flight the record buffer is that scan's: pm_candidates_device hands
    out records of one fully scanned range, or none"""
    pm, codes, table, pats, ids, h = small_case(0, True)
    before = two_ranges_then(pm)
    ptr, cnt = pm.candidates_device()
    rec = pm.copy_records(ptr, cnt)
    enqueued(pm, before)
    if cnt:
        ends = rec["end"].astype(np.int64)
        lo = int(ends.min() - 1) // STEP * STEP
        assert ends.max() <= lo + STEP + 64, (cnt, int(ends.min()), int(ends.max()))
    # the next range still comes out right
    want = [t for t in O.sorted_tuples(h) if 2 * STEP < t[0] <= 3 * STEP]
    assert sat_amd.sorted_tuples(pm.scan_view(2 * STEP, 3 * STEP)) == want
    pm.close()


def test_close_under_a_lookahead():
    pm, codes, table, pats, ids, h = small_case(0, True)
    twin = small_case(0, True)[0]                                     # the same calls on a second handle: its count says what close() met
    two_ranges_then(pm)
    pm.close()
    assert pm._h is None
    enqueued(twin, two_ranges_then(twin))
    twin.close()
    # the device is fine afterwards: a fresh handle gives the oracle's hits
    pm2, _, _, _, _, h2 = small_case(0, True)
    assert sat_amd.sorted_tuples(pm2.find_all()) == O.sorted_tuples(h2)
    pm2.close()


# ---- patterns that share an id under bare shift_and_inexact -k ----------------------------------------------------------

def test_shared_ids_keep_shift_and_inexact_off_the_edit_seed_plan():
    """The edit-distance seed plan keeps one record per (id, end), the automaton reports every pattern (shift_and_inexact.cc:316-335):
    with ids that repeat the option set runs on the bit-parallel family, and a forced seed kernel is refused.  (The hits of
    that case are the dense test's, inexact_k1 with ids (7, 7).)"""
    codes = D.codes(D.N0)
    kw = dict(k=1, indels=True, semantics=sat_amd.SEM_SHIFT_AND_INEXACT)
    for ids, seed in (((1, 2), True), ((7, 7), False)):
        pm = sat_amd.PatternMatch(**kw)
        for p, i in zip(D.PATTERNS, ids):
            pm.add_pattern(p, i)
        pm.init(codes, D.TABLE)
        assert (pm.selected()[1] == sat_amd.KERNEL_SEED) == seed, (ids, pm.selected(), pm.describe())
        got = fields(pm.scan_view(0, D.N0))
        for g, w in zip(got, D.expected("inexact_k1", ids, D.N0)):
            assert np.array_equal(g, w), (ids, g.size, w.size)
        pm.close()
    pm = sat_amd.PatternMatch(kernel=sat_amd.KERNEL_SEED, **kw)
    for p in D.PATTERNS:
        pm.add_pattern(p, 7)
    with pytest.raises(sat_amd.PmError, match="share an id"):
        pm.init(codes, D.TABLE)
    pm.close()
