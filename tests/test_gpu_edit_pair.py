"""GPU: the edit plan's first stage on the pair geometry beyond -k 2 on one tile: with edit_pair=True (the
PM_EDIT_PAIR bit of pm_config.long_patterns) every pattern tile of a larger list at -k 2, -k 1 under filter_bitvec and bare
shift_and_inexact (pm_pair_edit_scan_k1: the two tests (0,1,0) and (2,3,0)) and exact_bases -k 1 / -k 2 run
pm_pair_edit_scan + pm_pair_edit_resolve where pm_edit_scan ran.  The hits are the oracle's either way; without the bit, and
with PM_EDIT_PAIR=off beside it, every handle describes itself as before.

Text and primers: tests/test_gpu_seed_slots.small_text() (three entries with N runs and repeats, a too-short one, some 500
primers of 20..31 characters with 0..2 changes, half of them indels); PM_SEED_TILE cuts them into tiles."""
import numpy as np
import pytest

import dense_stream as D
import sat_amd
import synth
import test_gpu_exhaustive as EX
import test_gpu_long_edits as LE
import test_gpu_seed_slots as SS
from oracle import pmoracle as O

pytestmark = pytest.mark.gpu

NEW = "kernel=pm_pair_edit_scan+pm_pair_edit_resolve+"
OLD = "kernel=pm_edit_scan+pm_edits_verify "
BITVEC, INEXACT, BASES = sat_amd.SEM_FILTER_BITVEC, sat_amd.SEM_SHIFT_AND_INEXACT, sat_amd.SEM_EXACT_BASES
# routed option sets: name -> (k, semantics, oracle engine, exact_start_bases, tiles (0: one tile, no PM_SEED_TILE), verify kernel, tests)
ROUTED = {
    "k2_tiles2": (2, BITVEC, O.FILTER_BITVEC, 0, 2, "pm_edits_verify", 14),
    "k2_tiles3": (2, INEXACT, O.SHIFT_AND_INEXACT, 0, 3, "pm_edits_verify", 14),
    "k1_bitvec": (1, BITVEC, O.FILTER_BITVEC, 0, 0, "pm_edits_verify", 2),
    "k1_inexact": (1, INEXACT, O.SHIFT_AND_INEXACT, 0, 0, "pm_edits_verify", 2),
    "k1_bitvec_tiles3": (1, BITVEC, O.FILTER_BITVEC, 0, 3, "pm_edits_verify", 2),
    "bases_k1": (1, BASES, O.EXACT_BASES_KT, 8, 0, "pm_bases_verify", 2),
    "bases_k2": (2, BASES, O.EXACT_BASES_KT, 8, 0, "pm_bases_verify", 14),
    "bases_k2_tiles2": (2, BASES, O.EXACT_BASES_KT, 8, 2, "pm_bases_verify", 14),
}
_WANT = {}


def tile_env(monkeypatch, npat, tiles):
    monkeypatch.delenv("PM_EDIT_PAIR", raising=False)
    monkeypatch.delenv("PM_EDIT_SCAN", raising=False)
    if tiles:
        monkeypatch.setenv("PM_SEED_TILE", str((npat + tiles - 1) // tiles))
    else:
        monkeypatch.delenv("PM_SEED_TILE", raising=False)


def engine(pats, k, sem, bit=True, zone=0, ids=None, **kw):
    pm = sat_amd.PatternMatch(k=k, indels=True, semantics=sem, kernel=sat_amd.KERNEL_SEED if sem == BASES else sat_amd.KERNEL_AUTO,
                              edit_pair=bit, **kw)
    for i, p in enumerate(pats):
        pm.add_pattern(p, ids[i] if ids else i + 1, zone, 0)
    return pm


def want_of(name):
    if name not in _WANT:
        k, _, eng, zone, _, _, _ = ROUTED[name]
        codes, table, pats = SS.small_text()
        E = [zone] * len(pats) if zone else None
        _WANT[name] = O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=eng, k=k, indels=True, esb=E))
    return _WANT[name]


def new_route(d, name):
    _, _, _, _, tiles, verify, tests = ROUTED[name]
    assert d.startswith(NEW + verify + " tiles=%d tests=%d " % (max(tiles, 1), tests)), (name, d)


# ---- 1. routing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ROUTED))
def test_routing(name, monkeypatch):
    """with the bit: the pair geometry; without it, and with PM_EDIT_PAIR=off beside it: pm_edit_scan, as before"""
    k, sem, _, zone, tiles, _, _ = ROUTED[name]
    codes, table, pats = SS.small_text()
    tile_env(monkeypatch, len(pats), tiles)
    seen = {}
    for what, bit, off in (("bit", True, False), ("clear", False, False), ("off", True, True)):
        if off:
            monkeypatch.setenv("PM_EDIT_PAIR", "off")
        pm = engine(pats, k, sem, bit=bit, zone=zone)
        try:
            pm.init(codes, table)
            seen[what] = pm.describe()
        finally:
            pm.close()
    new_route(seen["bit"], name)
    assert seen["clear"].startswith(OLD + "tiles=%d " % max(tiles, 1)), (name, seen["clear"])
    assert seen["off"] == seen["clear"], (name, seen)


@pytest.mark.parametrize("what", ["k2_one_tile", "halves_k1", "K2", "k0", "k3"])
def test_the_bit_leaves_the_other_option_sets_alone(what, monkeypatch):
    kw = {"k2_one_tile": dict(k=2, indels=True, semantics=BITVEC), "halves_k1": dict(k=1, indels=True, semantics=sat_amd.SEM_EXACT_HALVES),
          "K2": dict(k=2, indels=False, semantics=BITVEC), "k0": dict(k=0, indels=True), "k3": dict(k=3, indels=True)}[what]
    codes, table, pats = SS.small_text()
    tile_env(monkeypatch, len(pats), 0)
    seen = []
    for bit in (False, True):
        pm = sat_amd.PatternMatch(edit_pair=bit, **kw)
        for i, p in enumerate(pats):
            pm.add_pattern(p, i + 1)
        try:
            pm.init(codes, table)
            seen.append(pm.describe())
        finally:
            pm.close()
    assert seen[0] == seen[1], (what, seen)
    if what == "k2_one_tile":
        assert seen[0].startswith(NEW + "pm_edits_verify tiles=1 tests=14 fields=2-of-4 x 5 bases, displaced by |d| <= 2 window=20 "), seen[0]
    else:
        assert "pm_pair_edit" not in seen[0], (what, seen[0])


# ---- 2. parity with the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1 << 26, 193])
@pytest.mark.parametrize("name", list(ROUTED))
def test_parity(name, chunk, monkeypatch):
    k, sem, _, zone, tiles, _, _ = ROUTED[name]
    codes, table, pats = SS.small_text()
    want = want_of(name)
    assert len(want) > 128, (name, len(want))
    tile_env(monkeypatch, len(pats), tiles)
    pm = engine(pats, k, sem, zone=zone)
    try:
        pm.init(codes, table)
        new_route(pm.describe(), name)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
    finally:
        pm.close()
    assert got == want, (name, chunk, len(got), len(want))


# ---- 3. tiles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_seed_records_index_their_own_tile(k, monkeypatch):
    """three tiles with hits in each; the first two tiles' primers change places and the ids (given by place) follow"""
    codes, table, pats = SS.small_text()
    pats = pats[:len(pats) // 3 * 3]
    per = len(pats) // 3
    tile_env(monkeypatch, len(pats), 3)
    want = O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=O.SHIFT_AND_INEXACT, k=k, indels=True))
    for t in range(3):
        assert any(t * per < pid <= (t + 1) * per for _, pid, _ in want), t
    swapped = pats[per:2 * per] + pats[:per] + pats[2 * per:]
    place = lambda pid: pid + per if pid <= per else (pid - per if pid <= 2 * per else pid)
    got = []
    for lst in (pats, swapped):
        pm = engine(lst, k, INEXACT)
        try:
            pm.init(codes, table)
            assert pm.describe().startswith(NEW + "pm_edits_verify tiles=3 "), pm.describe()
            got.append(sat_amd.sorted_tuples(pm.find_all()))
        finally:
            pm.close()
    assert got[0] == want, (k, len(got[0]), len(want))
    assert got[1] == sorted((e, place(pid), d) for e, pid, d in want), k


@pytest.mark.parametrize("name", ["k1_bitvec", "k2_inexact"])
def test_a_wide_tile_beside_a_narrow_one(name, monkeypatch):
    """the case of tests/test_gpu_long_edits.py: the second of two tiles holds the primers of 33..64 characters"""
    c = LE.mixed_case()
    pats = LE.mixed_pats(rest=False)
    k, sem, _, _, _ = LE.MIXED_OPTS[name]
    order = sorted(range(len(pats)), key=lambda i: (len(pats[i]) > 32, i))
    main = [i for i in order if len(pats[i]) >= 20]
    tile_env(monkeypatch, len(main), 2)
    pm = sat_amd.PatternMatch(k=k, indels=True, semantics=sem, long_edits=True, edit_pair=True)
    for i in order:
        pm.add_pattern(pats[i], i + 1)
    try:
        pm.init(c["codes"], c["table"])
        d = pm.describe()
        assert d.startswith(NEW + "pm_edits_verify tiles=2 ") and "wide tiles=1)" in d, d
        got = sat_amd.sorted_tuples(pm.find_all())
    finally:
        pm.close()
    assert got == LE.mixed_want(name, rest=False)


def test_natural_tiling(monkeypatch):
    """no PM_SEED_TILE: 300,000 random 20-mers and their reverse complements are three tiles of 200,000; 2,000 of them are
    planted in a 16 Mbp random stream with 0..2 edits.  Both routes give the same hits and every planted site is found."""
    tile_env(monkeypatch, 0, 0)
    rng = np.random.default_rng(30020)
    n, npri, nsite = 16 << 20, 300000, 2000
    codes = rng.integers(0, 4, size=n, dtype=np.uint8)
    prim = rng.integers(0, 4, size=(npri, 20), dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    fwd = [bytes(letters[r]).decode() for r in prim]
    pats = fwd + [synth.revcomp(p) for p in fwd]
    sites = []
    for s in range(nsite):
        pi = int(rng.integers(0, npri))
        ne = s % 3
        w = "".join(synth.mutate(rng, fwd[pi], nsub=int(ne > 0), nins=int(ne > 1 and s % 2 == 0), ndel=int(ne > 1 and s % 2 == 1)))
        at = 1000 + s * 8000
        codes[at:at + len(w)] = [b"ACGT".index(ch) for ch in w.encode()]
        sites.append((pi + 1, at + len(w)))
    got = []
    for bit in (True, False):
        pm = engine(pats, 2, BITVEC, bit=bit)
        try:
            pm.init(codes, LE.TABLE)
            d = pm.describe()
            assert d.startswith((NEW + "pm_edits_verify tiles=3 tests=14 ") if bit else (OLD + "tiles=3 ")), d
            h = pm.find_all()
            got.append(np.stack([h["end"].astype(np.int64), h["pid"].astype(np.int64), h["k"].astype(np.int64)], axis=1))
        finally:
            pm.close()
    a, b = (g[np.lexsort((g[:, 2], g[:, 1], g[:, 0]))] for g in got)
    assert a.shape == b.shape and np.array_equal(a, b), (a.shape, b.shape)
    have = set(zip(a[:, 1].tolist(), a[:, 0].tolist()))
    for pid, end in sites:
        assert any((pid, e) in have for e in range(end - 2, end + 3)), (pid, end)


# ---- 4. stream edges -----------------------------------------------------------------------------------------------------
def edges_case():
    """tests/test_gpu_long_edits.edges_case with primers of 20..32 characters: ends in the stream's first L + 6 characters
    (first characters missing too), in its last four (trailing characters deleted), one across an end-of-sequence character"""
    rng = np.random.default_rng(5572)
    e0, e1, e2 = LE.rand_seq(rng, 150), LE.rand_seq(rng, 90), LE.rand_seq(rng, 130)
    raw = (e0 + "\n" + e1 + "\n" + e2).encode()
    codes = synth.normalize(raw, LE.TABLE)
    pats = []
    for L in (20, 21, 25, 31, 32):
        pats += [e0[:L], "G" + e0[:L - 1], "CA" + e0[:L - 2], e0[2:L + 2], e0[1:12] + e0[13:L + 2], e0[3:L + 3]]
        pats += [e2[-L:], e2[-L:-1] + "C", e2[-L + 2:] + "GT", e2[-L - 2:-2], e2[-L - 1:-12] + e2[-11:] + "A", e2[-L - 3:-3]]
    across = e0[-12:] + "A" + e1[:12]
    pats += [across, e1[:24], e1[-24:], e1[1:25], e0[-25:-1]]
    pats += [LE.rand_seq(rng, 22) for _ in range(5)] + [e1[10:32], e0[5:28]]
    return dict(codes=codes, pats=pats, across=pats.index(across) + 1)


@pytest.mark.parametrize("k", [1, 2])
def test_stream_edges(k, monkeypatch):
    c = edges_case()
    codes, pats, n = c["codes"], c["pats"], c["codes"].size
    want = LE.oracle_hits(codes, LE.TABLE, pats, k, O.FILTER_BITVEC)
    assert c["across"] not in {pid for _, pid, _ in want}
    assert any(e < len(pats[pid - 1]) for e, pid, _ in want) and any(e >= n - 3 for e, pid, _ in want)
    tile_env(monkeypatch, len(pats), 3)
    for chunk in (1 << 26, 37, 3):
        pm = engine(pats, k, BITVEC)
        try:
            pm.init(codes, LE.TABLE)
            assert pm.describe().startswith(NEW + "pm_edits_verify tiles=3 "), pm.describe()
            got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        finally:
            pm.close()
        assert got == want, (k, chunk, got, want)


# ---- 5. lists at their limits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k2_tiles3", "k1_bitvec"])
def test_record_buffer_of_whole_blocks_and_one_off(name, monkeypatch):
    k, sem, _, zone, tiles, _, _ = ROUTED[name]
    codes, table, pats = SS.small_text()
    tile_env(monkeypatch, len(pats), tiles)
    generous = want_of(name)
    for cap in (63, 64, 65, 129):
        pm = engine(pats, k, sem, zone=zone)
        try:
            pm.init(codes, table)
            new_route(pm.describe(), name)
            pm.set_capacity(cap)
            got = sat_amd.sorted_tuples(pm.find_all())
        finally:
            pm.close()
        assert got == generous, (name, cap, len(got), len(generous))


DENSE_DECOY = "GGGGGTTTTTGGGGGTTTTT"                                   # the first tile's only primer: nowhere near the "AC" stream


def dense_records(k, n):
    """tests/test_gpu_seed_slots.dense_records on three tiles of one primer each: the decoy, (AC)^10, (CA)^10"""
    pm = engine([DENSE_DECOY] + D.PATTERNS, k, INEXACT, ids=(9, 1, 2))
    try:
        pm.init(D.codes(n), D.TABLE)
        assert pm.describe().startswith(NEW + "pm_edits_verify tiles=3 tests=%d " % (2 if k == 1 else 14)), pm.describe()
        hits = sat_amd.sorted_tuples(pm.find_all()) if n == D.N0 else None
        capacity = 1 << 24
        pm.set_capacity(capacity)
        cnt = None
        while cnt is None:
            pm.scan_async(0, n)
            try:
                cnt = pm.scan_wait()
            except sat_amd.PmError as err:
                assert err.code == sat_amd.PM_E_OVERFLOW and err.required > capacity, (k, n, err)
                capacity = int(err.required * 1.25) + 1024
                pm.set_capacity(capacity)
        st = pm.scan_stats()
        ptr, have = pm.candidates_device()
        assert have == cnt, (k, n, have, cnt)
        rec = pm.copy_records(ptr, cnt)
    finally:
        pm.close()
    end, pid, lvl = rec["end"].astype(np.int64), rec["pid"].astype(np.int64), rec["k"].astype(np.int64)
    o = np.lexsort((lvl, pid, end))
    return (end[o], pid[o], lvl[o]), st, hits


@pytest.mark.parametrize("k", [1, 2])
def test_lists_overflow_in_a_later_tile(k, monkeypatch):
    """On "AC" * 2^20 every position is a suspect and a seed record of the second and of the third tile -- 2^21 of each, into
    a suspect list of 2^21 / 10 + 2^20 and a seed list of 2^21 / 6 + 2^20 slots -- and of none in the first.  The library
    enlarges both and scans again; the records are the closed form of the same handle's records at 4,096 characters, whose
    hits are the oracle's."""
    monkeypatch.delenv("PM_EDIT_PAIR", raising=False)
    monkeypatch.delenv("PM_EDIT_SCAN", raising=False)
    monkeypatch.setenv("PM_SEED_TILE", "1")
    n = 1 << 21
    base, st0, hits0 = dense_records(k, D.N0)
    want0 = O.sorted_tuples(O.find_all(O.Text(D.codes(D.N0), D.TABLE), [DENSE_DECOY] + D.PATTERNS, engine=O.SHIFT_AND_INEXACT, k=k, indels=True, ids=[9, 1, 2]))
    assert hits0 == want0 and len(want0) > D.N0, (k, len(hits0), len(want0))
    assert st0["internal_rescans"] == 0 and 0 < st0["edit_suspects"] <= D.N0 // 10 + (1 << 20), (k, st0)
    got, st, _ = dense_records(k, n)
    print("k =", k, "n = 4096:", st0, "n = 2^21:", st, "records:", got[0].size)
    assert st["edit_suspects"] > n // 10 + (1 << 20) and st["between_stages"] > n // 6 + (1 << 20), (k, st)
    assert st["internal_rescans"] >= 2, (k, st)
    for g, w, field in zip(got, D.extend(base, n), ("end", "pid", "k")):
        assert g.size == w.size, (k, field, g.size, w.size)
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError((k, field, "first difference at record", at, int(g[at]), int(w[at])))


# ---- 6. beside the other classes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_beside_the_short_class_and_the_residue(k, monkeypatch):
    codes, table, main = SS.small_text()
    rng = np.random.default_rng(1818)
    text = bytes(np.frombuffer(table, dtype=np.uint8)[codes]).decode()
    short = []
    while len(short) < 30:
        a = int(rng.integers(0, len(text) - 20))
        w = text[a:a + 18]
        if set(w) <= set("ACGT") and w not in short:
            short.append(w)
    a = next(i for i in range(200, len(text)) if set(text[i:i + 24]) <= set("ACGT"))
    with_n = text[a:a + 9] + "N" + text[a + 10:a + 24]
    pats = main[:200] + short + [with_n] + main[200:]
    want = O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=O.FILTER_BITVEC, k=k, indels=True))
    assert any(len(pats[pid - 1]) == 18 for _, pid, _ in want) and len(want) > 128
    tile_env(monkeypatch, len(main), 2)
    pm = engine(pats, k, BITVEC)
    try:
        pm.init(codes, table)
        d = pm.describe()
        assert d.startswith(NEW + "pm_edits_verify tiles=2 tests=%d " % (2 if k == 1 else 14)), d
        assert "pm_short_edit_scan for 30 patterns of 16..19 characters" in d and "for 1 patterns the seed plan does not take" in d, d
        got = sat_amd.sorted_tuples(pm.find_all())
    finally:
        pm.close()
    assert got == want, (k, len(got), len(want))


# ---- 7. other stream forms -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["windowed", "packed"])
@pytest.mark.parametrize("name", ["k2_tiles3", "k1_bitvec"])
def test_windowed_and_packed(name, form, monkeypatch):
    k, sem, _, zone, tiles, _, _ = ROUTED[name]
    codes, table, pats = SS.small_text()
    tile_env(monkeypatch, len(pats), tiles)
    pm = engine(pats, k, sem, zone=zone)
    try:
        if form == "windowed":
            probe = engine(pats, k, sem, zone=zone)
            probe.init(np.zeros(64, dtype=np.uint8), table, window=1)
            window = probe.residency()["window"]
            probe.close()
            assert window < codes.size // 2, (window, codes.size)
            pm.init(codes, table, window=window)
        else:
            bits = max(1, (len(table) - 1).bit_length())
            pm.init_packed(sat_amd.pack_codes(codes, bits), bits, codes.size, table)
        new_route(pm.describe(), name)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=700 if form == "windowed" else 1 << 26))
        res = pm.residency()
    finally:
        pm.close()
    if form == "windowed":
        assert res["window"] > 0 and res["loads"] > 1, res
    else:
        assert res["bits"] > 0, res
    assert got == want_of(name), (name, form, len(got), len(want_of(name)))


# ---- 8. every text within one edit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [20, 24, 32])
def test_every_text_within_one_edit(L, monkeypatch):
    """the two tests (0,1,0) and (2,3,0) and the one-edit edit_cost lose nothing: every text one edit away from the primer,
    between end-of-sequence characters, beside 1,500 decoys"""
    tile_env(monkeypatch, 0, 0)
    rng = np.random.default_rng(200 + L)
    p = EX.PATTERNS[L]
    variants = sorted(EX.edit_variants(p, 1))
    assert len(variants) > 6 * L                                      # (3 L substitutions, L deletions, 4 (L + 1) insertions, less the texts reached twice)
    parts = EX.stream_of(variants, rng)
    codes = synth.normalize(synth.stream(parts), EX.TABLE)
    pats = [p] + ["".join(rng.choice(list("ACGT"), size=L).tolist()) for _ in range(1500)]
    want = O.sorted_tuples(O.find_all(O.Text(codes, EX.TABLE), pats, engine=O.FILTER_BITVEC, k=1, indels=True))
    ends = np.array(sorted({e for e, pid, _ in want if pid == 1}))
    for a, b in EX.entry_bounds(parts):                               # (every variant ends a hit of the primer: the oracle's list is no empty yardstick)
        i = np.searchsorted(ends, a, side="right")
        assert i < ends.size and ends[i] <= b, (L, a, b)
    pm = engine(pats, 1, BITVEC)
    try:
        pm.init(codes, EX.TABLE)
        assert pm.describe().startswith(NEW + "pm_edits_verify tiles=1 tests=2 "), pm.describe()
        got = sat_amd.sorted_tuples(pm.find_all())
    finally:
        pm.close()
    assert got == want, (L, len(got), len(want))
