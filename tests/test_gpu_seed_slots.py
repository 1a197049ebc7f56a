"""GPU: the record lists of the pm_seed.hip plans at their limits.  Every kernel of that file writes its records into slots
a wave reserves 64 at a time (SEED_OUT_BLOCK) with one atomic on the list's counter: the counter goes on counting past the
list's capacity, nothing is written at or beyond it, and the slots of a block that stay empty are marked as holes.

(1) the record buffer (pm_set_capacity) at, just below and just above whole blocks, for every kernel that writes pm_hit
    records that way; (2) the seed list between a plan's two kernels overflowing, which the library answers by itself (a
    larger list, the range scanned again).  Expected values: the oracle, and for (2) the closed form of the dense stream
    (tests/dense_stream.py) over the same plan's records at 4,096 characters."""
import numpy as np
import pytest

import dense_stream as D
import synth
import sat_amd
from oracle import pmoracle as O

pytestmark = pytest.mark.gpu

HALVES = dict(k=1, indels=True, semantics=sat_amd.SEM_EXACT_HALVES, kernel=sat_amd.KERNEL_SEED)
EDITS = dict(k=1, indels=True, semantics=sat_amd.SEM_FILTER_BITVEC, kernel=sat_amd.KERNEL_SEED)
BASES = dict(k=1, indels=True, semantics=sat_amd.SEM_EXACT_BASES, kernel=sat_amd.KERNEL_SEED)
# name -> (PatternMatch arguments, environment, what pm_describe begins with, oracle engine, exact_start_bases); the kernel
# that fills the record buffer in brackets
PLANS = {
    "half_ranked": (HALVES, {}, "kernel=pm_half_scan+pm_half_verify ", O.EXACT_HALVES_KT, 0),                # [pm_half_verify]
    "half_bloom": (HALVES, {"PM_HALF_SCAN": "bloom"}, "kernel=pm_seed_scan ", O.EXACT_HALVES_KT, 0),         # [pm_seed_scan<0,0,true>]
    "edit_scan": (EDITS, {}, "kernel=pm_edit_scan+pm_edits_verify ", O.FILTER_BITVEC, 0),                    # [pm_edits_verify]
    "edit_bloom": (EDITS, {"PM_EDIT_SCAN": "bloom"}, "kernel=pm_seed_scan+pm_edits_verify ", O.FILTER_BITVEC, 0),   # [pm_edits_verify behind pm_seed_scan<20,1,false,true>]
    "bases": (BASES, {}, "kernel=pm_edit_scan+pm_edits_verify ", O.EXACT_BASES_KT, 8),                       # [pm_bases_verify]
}
CAPS = (1, 63, 64, 65, 127, 128, 129)
_TEXT = []


def small_text():
    """(codes, table, patterns): three entries of 1,400 bases with N runs and repeats, a too-short one; some 500 primers of 20..31
    characters cut from them with up to two changes.  Built once and left alone."""
    if not _TEXT:
        rng = np.random.default_rng(6464)
        ents = synth.make_entries(rng, 3, 1400, n_runs=1, repeats=True, short=True)
        pats = []
        for L in (20, 22, 25, 30):
            pats += synth.make_patterns(rng, ents, 130, length=L, planted=1.0, indel_frac=0.5, extras=False)
        pats = [p for p in dict.fromkeys(pats) if 20 <= len(p) <= 32 and set(p) <= set("ACGT")]
        table = synth.table_for(ents)
        _TEXT.append((synth.normalize(synth.stream(ents), table), table, pats))
    return _TEXT[0]


def handle(name, pats, codes, table, ids=None):
    kw, _, begins, _, zone = PLANS[name]
    pm = sat_amd.PatternMatch(**kw)
    for i, p in enumerate(pats):
        pm.add_pattern(p, ids[i] if ids else i + 1, zone, 0)
    pm.init(codes, table)
    assert pm.selected() == (kw["semantics"], sat_amd.KERNEL_SEED), (name, pm.selected())
    assert pm.describe().startswith(begins), (name, pm.describe())
    return pm


@pytest.mark.parametrize("name", list(PLANS))
def test_record_buffer_of_whole_blocks_and_one_off(name, monkeypatch):
    """pm_set_capacity(cap) for cap around one and two blocks of 64 slots: pm_scan reports the overflow, grows the buffer
    and scans again, and the hits are those of a generous buffer -- which are the oracle's (exact_halves.cc:120-224,
    filter_bitvec.cc:88-177, exact_bases.cc:69-129)."""
    kw, env, _, eng, zone = PLANS[name]
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    codes, table, pats = small_text()
    E = [zone] * len(pats) if zone else None
    want = O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=eng, k=kw["k"], indels=kw["indels"], esb=E))
    assert len(want) > max(CAPS), (name, len(want))                  # every capacity tried is too small for the hits alone
    pm = handle(name, pats, codes, table)
    generous = sat_amd.sorted_tuples(pm.find_all())
    pm.close()
    assert generous == want, (name, len(generous), len(want))
    for cap in CAPS:
        pm = handle(name, pats, codes, table)
        pm.set_capacity(cap)
        got = sat_amd.sorted_tuples(pm.find_all())
        pm.close()
        assert got == generous, (name, cap, len(got), len(generous))


def dense_records(name, n):
    """the records one scan of the whole dense stream of n characters leaves in the record buffer, as (end, pid, k) in that
    order, and the handle's counters.  The record buffer starts large and grows on demand (the caller's part, as in
    PatternMatch.scan_candidates): what this test is about is the list the library owns."""
    pm = handle(name, D.PATTERNS, D.codes(n), D.TABLE, ids=(1, 2))
    capacity = 1 << 24
    pm.set_capacity(capacity)
    cnt = None
    while cnt is None:
        pm.scan_async(0, n)
        try:
            cnt = pm.scan_wait()
        except sat_amd.PmError as err:
            assert err.code == sat_amd.PM_E_OVERFLOW and err.required > capacity, (name, n, err)
            capacity = int(err.required * 1.25) + 1024
            pm.set_capacity(capacity)
    st = pm.scan_stats()
    ptr, have = pm.candidates_device()
    assert have == cnt, (name, n, have, cnt)
    rec = pm.copy_records(ptr, cnt)
    pm.close()
    end, pid, k = rec["end"].astype(np.int64), rec["pid"].astype(np.int64), rec["k"].astype(np.int64)
    o = np.lexsort((k, pid, end))
    return (end[o], pid[o], k[o]), st


@pytest.mark.parametrize("name", ["edit_scan", "half_ranked"])
def test_seed_list_overflows_between_the_two_kernels(name):
    """On "AC" * 2^20 against (AC)^10 and (CA)^10 every position ends an exact occurrence of a pattern (and of a half), so
    the scan kernel writes a seed record per position at least: 2^21 records into a list of 2^21 / 6 + 2^20 slots.  The
    library enlarges the list and scans again inside pm_scan_wait (internal_rescans), and the records in the record
    buffer -- the automaton's candidates after the dedup for the edit-distance plan, the successful extensions for
    exact_halves -- are the closed form of the same plan's records at 4,096 characters, where nothing overflows."""
    n = 1 << 21
    base, st0 = dense_records(name, D.N0)
    assert st0["internal_rescans"] == 0 and 0 < st0["between_stages"] <= D.N0 // 6 + (1 << 20), (name, st0)
    end, pid, k = base
    # period 2 between the edges: the body moved by two characters is the body again
    a, b = (end > D.EDGE) & (end <= D.N0 - D.EDGE - 2), (end > D.EDGE + 2) & (end <= D.N0 - D.EDGE)
    assert a.sum() == b.sum() >= (D.N0 - 2 * D.EDGE - 2) // 2, (name, int(a.sum()), int(b.sum()))
    assert np.array_equal(end[a] + 2, end[b]) and np.array_equal(pid[a], pid[b]) and np.array_equal(k[a], k[b]), name
    got, st = dense_records(name, n)
    print(name, "n = 4096:", st0, "n = 2^21:", st, "records:", got[0].size)
    assert st["between_stages"] > n // 6 + (1 << 20), (name, st)
    assert st["internal_rescans"] >= 1, (name, st)
    for g, w, field in zip(got, D.extend(base, n), ("end", "pid", "k")):
        assert g.size == w.size, (name, field, g.size, w.size)
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError((name, field, "first difference at record", at, int(g[at]), int(w[at])))
