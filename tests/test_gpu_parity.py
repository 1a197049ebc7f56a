"""GPU: the HIP path, called through the C ABI, against (a) the committed reference outputs in
tests/golden and (b) the oracle on seeded random inputs.  Bit-exact (integer work)."""
import glob
import json
import os

import numpy as np
import pytest

import synth
import sat_amd
from oracle import pmoracle as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(p for p in glob.glob(os.path.join(GOLD, "*.json")) if "config1" not in p and not os.path.basename(p).startswith(("cli_", "pcr_")))
SEL2SEM = {0: sat_amd.SEM_AUTO, 1: sat_amd.SEM_KEYWORD_TREE, 2: sat_amd.SEM_KEYWORD_TREE, 4: sat_amd.SEM_SHIFT_AND,
           5: sat_amd.SEM_FILTER_BITVEC, 12: sat_amd.SEM_EXACT_HALVES, 14: sat_amd.SEM_EXACT_HALVES,
           100: sat_amd.SEM_SHIFT_AND_INEXACT}
KERNELS = [sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_SEED, sat_amd.KERNEL_AUTO]
SEED_OK = lambda sem, k, indels: sem != sat_amd.SEM_EXACT_BASES


def gpu_hits(codes, table, patterns, sem, k, indels, kernel=sat_amd.KERNEL_BITPAR, chunk=1 << 26, esb=None, eeb=None):
    pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sem, kernel=kernel)
    for i, p in enumerate(patterns):
        pm.add_pattern(p, i + 1, 0 if esb is None else esb[i], 0 if eeb is None else eeb[i])
    pm.init(codes, table)
    out = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
    pm.close()
    return out


def load(path):
    with open(path) as f:
        c = json.load(f)
    table = c["table"].encode("latin1")
    codes = synth.normalize(synth.stream(c["entries"]), table)
    pats = c["patterns"]
    return c, codes, table, pats + [sat_amd.reverse_comp(p) for p in pats]


def test_config1_known_answer():
    with open(os.path.join(GOLD, "config1_db_test_seq.json")) as f:
        c = json.load(f)
    raw = np.frombuffer(c["stream_latin1"].encode("latin1"), dtype=np.uint8)
    for sem in (sat_amd.SEM_AUTO, sat_amd.SEM_KEYWORD_TREE, sat_amd.SEM_SHIFT_AND):
        assert gpu_hits(raw, None, c["patterns"], sem, 0, True) == [(27, 10, 0)]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-5] for p in CASES])
def test_golden_engine_hits(path, kernel, monkeypatch):
    monkeypatch.setenv("PM_BITPAR_SEGLEN", "512")      # many segments: exercises halo + ownership
    c, codes, table, allp = load(path)
    monkeypatch.setenv("PM_SEED_CHUNK", "16384")
    monkeypatch.setenv("PM_SEED_GROUP", "3")
    ran = 0
    for name, e in c["engine"].items():
        if kernel == sat_amd.KERNEL_SEED and not SEED_OK(SEL2SEM[e["sel"]], e["k"], e["indels"]):
            continue
        try:
            got = gpu_hits(codes, table, allp, SEL2SEM[e["sel"]], e["k"], e["indels"], kernel)
        except sat_amd.PmError as err:
            # forcing the seed family on an option set it does not cover must fail loudly, never fall back
            assert kernel == sat_amd.KERNEL_SEED and err.code == -2, (c["name"], name, err)
            continue
        assert got == [tuple(h) for h in e["hits"]], (c["name"], name, kernel)
        ran += 1
    assert ran >= 7


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("kernel", [sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_AUTO])
def test_random_vs_oracle(seed, kernel, monkeypatch):
    monkeypatch.setenv("PM_BITPAR_SEGLEN", str([256, 768, 4096][seed % 3]))
    monkeypatch.setenv("PM_SEED_CHUNK", str([16384, 32768, 1 << 19][seed % 3]))
    monkeypatch.setenv("PM_SEED_GROUP", str([1, 2, 256][seed % 3]))
    rng = np.random.default_rng(77 + seed)
    ents = synth.make_entries(rng, int(rng.integers(1, 5)), int(rng.integers(300, 3000)), n_runs=int(rng.integers(0, 4)),
                              repeats=(seed % 2 == 0), short=(seed % 3 == 0))
    L = int(rng.integers(12, 31))
    pats = synth.make_patterns(rng, ents, int(rng.integers(20, 400)), length=L, planted=0.6,
                               minlen=(L - 5 if seed % 2 else None), indel_frac=0.4)
    table = synth.table_for(ents)
    raw = synth.stream(ents)
    codes = synth.normalize(raw, table)
    allp = pats + [synth.revcomp(p) for p in pats]
    for norm in (True, False):
        text = O.Text(codes, table) if norm else O.Text(np.frombuffer(raw, dtype=np.uint8))
        data, tb = (codes, table) if norm else (np.frombuffer(raw, dtype=np.uint8), None)
        for sem, osel, k, ind in [(sat_amd.SEM_AUTO, 0, 0, True), (sat_amd.SEM_AUTO, 0, 1, True), (sat_amd.SEM_AUTO, 0, 1, False),
                                  (sat_amd.SEM_AUTO, 0, 2, True), (sat_amd.SEM_AUTO, 0, 2, False),
                                  (sat_amd.SEM_SHIFT_AND_INEXACT, 100, 2, True), (sat_amd.SEM_SHIFT_AND_INEXACT, 100, 3, False),
                                  (sat_amd.SEM_FILTER_BITVEC, 5, 1, True), (sat_amd.SEM_EXACT_HALVES, 12, 2, True)]:
            eng = O.pick_engine(text, allp, k, ind) if osel == 0 else osel
            want = O.sorted_tuples(O.find_all(text, allp, engine=eng, k=k, indels=ind))
            got = gpu_hits(data, tb, allp, sem, k, ind, kernel)
            assert got == want, (seed, norm, sem, k, ind, kernel, len(want), len(got))


@pytest.mark.parametrize("row_slots", [2, 3, 5])
def test_pair_plan_row_overflow_and_shared_keys_vs_oracle(row_slots, monkeypatch):
    """The pair plan's slot table with tiny rows (PM_PAIR_ROW: 1, 2 or 4 slots per row of 32 keys and the overflow
    marker): most keys lie beyond their row's slots and reach pm_pair_verify as "walk the key's pattern list" --
    together with families of patterns that share their first or last ten bases (more than three patterns per key: the
    slot's walk flag) and exact duplicates.  -K 1 and -K 2, every engine that builds on the candidates, tiny scan chunks:
    the hits must be the oracle's (shift_and_inexact.cc:249-352, filter_bitvec.cc:88-177, exact_halves.cc:120-197)."""
    monkeypatch.setenv("PM_PAIR_ROW", str(row_slots))
    monkeypatch.setenv("PM_SEED_CHUNK", "16384")
    monkeypatch.setenv("PM_SEED_GROUP", "3")
    rng = np.random.default_rng(500 + row_slots)
    ents = synth.make_entries(rng, 3, 6000, n_runs=2, repeats=True, short=True)
    pats = synth.make_patterns(rng, ents, 900, length=20, planted=0.5)
    # families: nine patterns with the same first ten bases, seven with the same last ten, five equal in the middle
    s0 = ents[0]
    a = 700
    head, tail, mid = s0[a:a + 10].replace("N", "A"), s0[a + 40:a + 50].replace("N", "C"), s0[a + 85:a + 95].replace("N", "G")
    rnd = lambda n: "".join(rng.choice(list("ACGT"), size=n).tolist())
    pats += [head + rnd(10) for _ in range(9)] + [rnd(10) + tail for _ in range(7)] + [rnd(5) + mid + rnd(5) for _ in range(5)]
    pats += [s0[a:a + 20].replace("N", "A")] * 3 + [s0[a + 30:a + 50].replace("N", "C"), s0[a + 80:a + 100].replace("N", "G")]
    pats += [synth.mutate(rng, s0[a:a + 20].replace("N", "A"), nsub=2), synth.mutate(rng, s0[a + 30:a + 50].replace("N", "C"), nsub=1)]
    pats += [p + rnd(int(rng.integers(1, 12))) for p in pats[:60]]         # longer ones (the plan looks at the last 20 bases)
    allp = pats + [synth.revcomp(p) for p in pats]
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    text = O.Text(codes, table)
    for sem, osel, k in [(sat_amd.SEM_SHIFT_AND_INEXACT, 100, 2), (sat_amd.SEM_SHIFT_AND_INEXACT, 100, 1), (sat_amd.SEM_AUTO, 0, 2),
                         (sat_amd.SEM_AUTO, 0, 1), (sat_amd.SEM_EXACT_HALVES, 12, 2)]:
        eng = O.pick_engine(text, allp, k, False) if osel == 0 else osel
        want = O.sorted_tuples(O.find_all(text, allp, engine=eng, k=k, indels=False))
        pm = sat_amd.PatternMatch(k=k, indels=False, semantics=sem, kernel=sat_amd.KERNEL_SEED)
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        assert "pm_pair_scan" in pm.describe() and "row_slots=%d" % row_slots in pm.describe(), pm.describe()
        got = sat_amd.sorted_tuples(pm.find_all(chunk=1 << 26))
        pm.close()
        assert got == want and len(want) > 30, (row_slots, sem, k, len(want), len(got))


@pytest.mark.parametrize("row_slots", [None, 2, 3])
def test_pair_plan_flagged_slots_with_nothing_in_common(row_slots, monkeypatch):
    """What the consume stage of pm_pair_scan must not dismiss although none of a slot's three patterns is near the
    window: keys beyond their row's slots (the row's overflow marker holds no pattern: its fields read AAAAAAAAAA, and
    a window without an A differs from that in all ten bases) and keys with more than three patterns whose fourth
    differs from the third everywhere.  For every field pair: six row mates (same key fields but for the key's last two
    bases) with A-free other fields, and five patterns on one key, the other fields of the fourth and fifth chosen
    against the third's.  scripts/fuzz_families.py seed 1175 found the -K 1 case (the flag used to enter the third
    count as -8: 10 - 8 - 2 = 0 was "not suspicious").  Oracle: shift_and_inexact.cc:249-352, exact_halves.cc:120-197."""
    if row_slots is not None:
        monkeypatch.setenv("PM_PAIR_ROW", str(row_slots))
    monkeypatch.setenv("PM_SEED_CHUNK", "16384")
    rng = np.random.default_rng(1175)
    rnd = lambda n, al="ACGT": "".join(rng.choice(list(al), size=n).tolist())
    shift = lambda w, j: "".join("ACGT"[("ACGT".index(c) + j) % 4] for c in w)
    pats = []
    for fa in range(4):
        for fb in range(fa + 1, 4):
            others = [f for f in range(4) if f not in (fa, fb)]
            def build(ka, kb, o1, o2):
                fields = [None] * 4
                fields[fa], fields[fb], fields[others[0]], fields[others[1]] = ka, kb, o1, o2
                return "".join(fields)
            ka, kb3 = rnd(5), rnd(3)
            for tail2 in ("AA", "AC", "CG", "GT", "TA", "TT"):       # row mates: the key's bit index differs, its row does not
                pats.append(build(ka, kb3 + tail2, rnd(5, "CGT"), rnd(5, "CGT")))
            ka, kb = rnd(5), rnd(5)                                   # five patterns on one key
            o = rnd(10)
            for w in (o, rnd(10), shift(o, 1), shift(o, 2), shift(o, 3)):   # the 4th and 5th differ from the 3rd in all ten bases
                pats.append(build(ka, kb, w[:5], w[5:]))
    pats += [rnd(int(rng.integers(1, 8))) + p for p in pats[:20]]     # longer ones (the plan looks at the last 20 bases)
    sites = []
    for p in pats:
        sites += [p, synth.mutate(rng, p, nsub=1), synth.mutate(rng, p, nsub=2), synth.mutate(rng, p, nsub=3)]
    order = rng.permutation(len(sites))
    raw = ("\n" + "".join(rnd(int(rng.integers(3, 60))) + sites[i] for i in order) + rnd(50) + "\n").encode()
    table = b"ACGT\n"
    codes = synth.normalize(raw, table)
    text = O.Text(codes, table)
    allp = pats + [synth.revcomp(p) for p in pats]
    for sem, eng, k in [(sat_amd.SEM_SHIFT_AND_INEXACT, 100, 1), (sat_amd.SEM_SHIFT_AND_INEXACT, 100, 2), (sat_amd.SEM_FILTER_BITVEC, 5, 1),
                        (sat_amd.SEM_EXACT_HALVES, 12, 1), (sat_amd.SEM_EXACT_HALVES, 12, 2)]:
        want = O.sorted_tuples(O.find_all(text, allp, engine=eng, k=k, indels=False))
        pm = sat_amd.PatternMatch(k=k, indels=False, semantics=sem, kernel=sat_amd.KERNEL_SEED)
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        assert "pm_pair_scan" in pm.describe() and (row_slots is None or "row_slots=%d" % row_slots in pm.describe()), pm.describe()
        got = sat_amd.sorted_tuples(pm.find_all(chunk=1 << 26))
        pm.close()
        assert got == want and len(want) >= len(pats), (row_slots, sem, k, len(want), len(got), sorted(set(want) - set(got))[:5])


def test_chunked_scan_equals_whole(monkeypatch):
    """find_patterns is resumable: small pm_scan ranges give the same hit set,
    including clusters and seeds that straddle range boundaries."""
    c, codes, table, allp = load(CASES[-1])
    for sem, k, ind in [(sat_amd.SEM_AUTO, 0, True), (sat_amd.SEM_AUTO, 1, True), (sat_amd.SEM_AUTO, 1, False),
                        (sat_amd.SEM_AUTO, 2, True), (sat_amd.SEM_AUTO, 2, False)]:
        for kernel in (sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_AUTO):
            whole = gpu_hits(codes, table, allp, sem, k, ind, kernel)
            for chunk in (97, 1000, 4096):
                assert gpu_hits(codes, table, allp, sem, k, ind, kernel, chunk=chunk) == whole, (sem, k, ind, kernel, chunk)


def test_sharded_candidates_then_finalize():
    """The multi-GPU decomposition on one device: candidates of disjoint stream shards, merged,
    then one pm_finalize == single scan."""
    c, codes, table, allp = load(CASES[0])
    n = codes.size
    for k, ind in [(0, True), (1, True), (1, False), (2, False), (2, True)]:
        pm = sat_amd.PatternMatch(k=k, indels=ind)
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        whole = sat_amd.sorted_tuples(pm.find_all())
        pm.reset()
        cuts = [0, n // 3 + 5, 2 * n // 3 - 7, n]
        parts = [pm.scan_candidates(cuts[i], cuts[i + 1]) for i in range(3)]
        merged = np.concatenate(parts[::-1])            # arrival order must not matter
        assert sat_amd.sorted_tuples(pm.finalize(merged, n, last=True)) == whole, (k, ind)
        pm.close()


def test_edge_cases():
    table = b"ACGT\n"
    # empty stream, stream shorter than the pattern, match flush with both stream ends
    pat = "ACGTTGCAACGTAGCT"
    enc = lambda s: synth.normalize(s.encode(), table)
    assert gpu_hits(np.zeros(0, dtype=np.uint8), table, [pat], sat_amd.SEM_AUTO, 0, True) == []
    assert gpu_hits(enc("\nACGT\n"), table, [pat], sat_amd.SEM_AUTO, 2, True) == \
        O.sorted_tuples(O.find_all(O.Text(enc("\nACGT\n"), table), [pat], engine=5, k=2, indels=True))
    s = pat + "\n"                                   # no leading EOS: pattern starts at stream index 0
    for k, ind, eng in [(0, True, 2), (2, False, 5), (2, True, 5), (2, True, 100), (2, False, 100)]:
        sem = sat_amd.SEM_SHIFT_AND_INEXACT if eng == 100 else sat_amd.SEM_AUTO
        text = O.Text(enc(s), table)
        want = O.sorted_tuples(O.find_all(text, [pat, pat[2:] + "AC"], engine=eng, k=k, indels=ind))
        for kernel in (sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_AUTO):
            assert gpu_hits(enc(s), table, [pat, pat[2:] + "AC"], sem, k, ind, kernel) == want, (k, ind, eng, kernel)


@pytest.mark.parametrize("norm", [True, False])
def test_extensions_read_past_the_end_of_the_stream(norm):
    """exact_halves / exact_bases extend a seed found right at the end of the stream over characters the
    stream no longer has: the reference reads the zero padding of the mapped file there (mapFile.h:49-57,
    primer_alignment.cc:573-574) -- code 0, i.e. 'A' on a normalized stream, a byte no primer holds (a substitution)
    on a raw one -- and reports hits that end up to len2 characters beyond the last one.  Found by
    scripts/fuzz_families.py (seed 1090): the whole-pattern windows of the seed kernels end inside the stream."""
    table = b"ACGT\n"
    rng = np.random.default_rng(90)
    body = "".join("ACGT"[c] for c in rng.integers(0, 4, 1500))
    tail = "GATTACAGGCTTACCGTCAATGCCTGAAGTCCATGTTGCA"                        # the stream's last 40 characters
    raw = ("\n" + body + tail).encode()
    pats = []
    for L in (14, 20, 21, 24, 32):
        len2 = L - L // 2
        for t in range(1, len2 + 2):                               # t = len2 + 1: the left half itself hangs over (never a hit)
            p = tail[len(tail) - (L - t):] + "A" * t
            pats.append(p)
            pats.append(p[:-1] + "C")                              # one substitution in the overhang
            if L - t - 1 >= L // 2:
                i = L - t - 1
                pats.append(p[:i] + "ACGT"[("ACGT".index(p[i]) + 1) % 4] + p[i + 1:])       # one in the right half on the stream
            pats.append("ACGT"[("ACGT".index(p[0]) + 2) % 4] + p[1:])                          # one in the left half
            if t >= 2:
                pats.append(p[:-2] + "CG")                         # two in the overhang
    pats = list(dict.fromkeys(pats))
    data, tb = (synth.normalize(raw, table), table) if norm else (np.frombuffer(raw, dtype=np.uint8), None)
    text = O.Text(data, table) if norm else O.Text(data)
    total = 0
    for sem, eng, k, ind in [(sat_amd.SEM_EXACT_HALVES, 12, 0, False), (sat_amd.SEM_EXACT_HALVES, 12, 1, False), (sat_amd.SEM_EXACT_HALVES, 12, 2, False),
                             (sat_amd.SEM_EXACT_HALVES, 12, 1, True), (sat_amd.SEM_EXACT_HALVES, 12, 2, True), (sat_amd.SEM_AUTO, 0, 1, True)]:
        use = [p for p in pats if len(p) >= 16] if ind else pats   # (exact_halves -k on the seed family: 16..32 characters)
        e = O.pick_engine(text, use, k, ind) if eng == 0 else eng
        want = O.sorted_tuples(O.find_all(text, use, engine=e, k=k, indels=ind))
        beyond = [h for h in want if h[0] > len(raw)]
        assert beyond or (not norm and k == 0), (sem, k, ind)      # (on a raw stream every character past the end is a substitution)
        total += len(beyond)
        for kernel in (sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_SEED, sat_amd.KERNEL_AUTO):
            assert gpu_hits(data, tb, use, sem, k, ind, kernel) == want, (norm, sem, k, ind, kernel)
    assert total > 0
    # exact_bases: the mandated first block found right at the end, the remainder extended past it
    # (exact_bases.cc:92-121); a mandated last block keeps the whole pattern on the stream
    use = [p for p in pats if len(p) >= 20]
    for esb, eeb in [(8, 0), (6, 3), (0, 7)]:
        E, F = [esb] * len(use), [eeb] * len(use)
        for k, ind in [(1, False), (2, False), (1, True), (2, True)]:
            want = O.sorted_tuples(O.find_all(text, use, engine=8, k=k, indels=ind, esb=E, eeb=F))
            beyond = [h for h in want if h[0] > len(raw)]
            assert bool(beyond) == (esb >= eeb) or not norm, (esb, eeb, k, ind, len(beyond))
            for kernel in (sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_SEED):
                got = gpu_hits(data, tb, use, sat_amd.SEM_EXACT_BASES, k, ind, kernel, esb=E, eeb=F)
                assert got == want, (norm, esb, eeb, k, ind, kernel, len(want), len(got), sorted(set(want) - set(got))[:4])
            if not ind:
                # two position shards (pm_finalize_device_owned): the one with the end of the stream owns what ends beyond it
                pm = sat_amd.PatternMatch(k=k, indels=False, semantics=sat_amd.SEM_EXACT_BASES, kernel=sat_amd.KERNEL_SEED)
                for i, p in enumerate(use):
                    pm.add_pattern(p, i + 1, esb, eeb)
                pm.init(data, tb)
                n, cut, guard, parts = len(raw), 700, 200, []
                for own_lo, own_hi in ((0, cut), (cut, n)):
                    g_lo, g_hi = max(0, own_lo - guard), min(n, own_hi + guard)
                    pm.reset()
                    pm.scan_candidates(g_lo, g_hi, to_host=False)
                    parts += sat_amd.sorted_tuples(pm.finalize_device(0, sort=True, owned=(own_lo, own_hi, g_lo, None if g_hi == n else g_hi)))
                pm.close()
                assert sorted(parts) == want, (norm, esb, eeb, k, len(want), len(parts))


@pytest.mark.parametrize("nchars", [11, 15, 19, 23])
def test_overhang_on_a_stream_shorter_than_the_patterns(nchars):
    """a stream of fewer characters than a pattern.  The left half (exact_halves) / the mandated first block
    (exact_bases) is still found inside it and extended over the mapped file's zero padding; the loop over the overhangs
    must not stop at the first one that does not fit (pm_api.cpp stream_end_overhang_candidates)."""
    table = b"ACGT\n"
    tail = "GATTACAGGCTTACCGTCAATGCC"[:nchars - 1]
    raw = ("\n" + tail).encode()
    data = synth.normalize(raw, table)
    text = O.Text(data, table)
    pats = []
    for L in (20, 22, 24):
        for t in range(1, L - L // 2 + 1):
            if L - t <= len(tail):
                p = tail[len(tail) - (L - t):] + "A" * t
                pats += [p, p[:-1] + "C"]
    pats = list(dict.fromkeys(pats))
    assert pats
    for sem, eng, k in [(sat_amd.SEM_EXACT_HALVES, 12, 1), (sat_amd.SEM_EXACT_HALVES, 12, 2)]:
        want = O.sorted_tuples(O.find_all(text, pats, engine=eng, k=k, indels=False))
        assert any(h[0] > len(raw) for h in want), (nchars, k)
        for kernel in (sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_SEED):
            assert gpu_hits(data, table, pats, sem, k, False, kernel) == want, (nchars, sem, k, kernel)
    E, F = [8] * len(pats), [0] * len(pats)
    for k in (1, 2):
        want = O.sorted_tuples(O.find_all(text, pats, engine=8, k=k, indels=False, esb=E, eeb=F))
        for kernel in (sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_SEED):
            assert gpu_hits(data, table, pats, sat_amd.SEM_EXACT_BASES, k, False, kernel, esb=E, eeb=F) == want, (nchars, k, kernel)


def test_edit_plan_matches_that_end_with_the_stream():
    """-k on the seed family at the very end of the stream: a match whose last characters need a pattern character
    deleted is seeded by the window one or two positions behind its end, where the stream has no windows
    (scripts/fuzz_families.py seed 1308).  Patterns = the stream's last 18..31 characters with one or two characters
    inserted / substituted / removed at every place near their end; with and without an entry end in front.
    Oracle: shift_and_inexact.cc:249-352, filter_bitvec.cc:88-177."""
    table = b"ACGT\n"
    rng = np.random.default_rng(1308)
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    for tail_eos in (False, True):
        raw = ("\n" + rnd(4000) + ("\n" if tail_eos else "")).encode()
        core = raw[:-1] if tail_eos else raw
        pats = []
        for L in (18, 19, 20, 21, 25, 31):
            site = core[-L:].decode()
            for i in range(L - 8, L + 1):
                for c in "ACGT":
                    pats.append(site[:i] + c + site[i:])                           # one character the stream does not have
                    for i2 in range(i, L + 1):
                        pats.append(site[:i] + c + site[i:i2] + "G" + site[i2:])   # two of them
                    if i < L:
                        pats.append(site[:i] + c + site[i + 1:])                   # substitution
                        pats.append(site[:i] + site[i + 1:])                       # the stream has one more
        pats = [p for p in dict.fromkeys(pats) if 20 <= len(p) <= 32]
        codes = synth.normalize(raw, table)
        text = O.Text(codes, table)
        for sem, eng, k in [(sat_amd.SEM_FILTER_BITVEC, 5, 2), (sat_amd.SEM_FILTER_BITVEC, 5, 1), (sat_amd.SEM_SHIFT_AND_INEXACT, 100, 2),
                            (sat_amd.SEM_SHIFT_AND_INEXACT, 100, 1), (sat_amd.SEM_EXACT_HALVES, 12, 2)]:
            want = O.sorted_tuples(O.find_all(text, pats, engine=eng, k=k, indels=True))
            at_end = [h for h in want if h[0] >= len(core) - 1]
            assert len(at_end) > 50, (sem, k, len(at_end))
            for kernel in (sat_amd.KERNEL_SEED, sat_amd.KERNEL_BITPAR):
                got = gpu_hits(codes, table, pats, sem, k, True, kernel)
                assert got == want, (tail_eos, sem, k, kernel, len(want), len(got), sorted(set(want) - set(got))[:5])


@pytest.mark.parametrize("lead_eos", [False, True])
def test_exact_bases_at_both_ends_of_the_stream(lead_eos):
    """exact_bases extends every occurrence of the mandated block (exact_bases.cc:92-121): leftwards over however
    much text there is in front (a pattern whose first characters are deleted at the start of the stream,
    primer_alignment.cc:657-662), rightwards past the end.  On the seed family the block occurrences come from
    whole-pattern windows, which do not exist there (scripts/fuzz_families.py seed 42595: hit at end 19)."""
    table = b"ACGT\n"
    rng = np.random.default_rng(42595)
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    body = rnd(3000)
    raw = (("\n" if lead_eos else "") + body).encode()
    pats = []
    for L in (20, 22, 27, 32):
        head, tail = body[:L], body[-L:]
        for d in (0, 1, 2):
            for site in (head, tail):
                pats.append(site[d:] + rnd(d))                      # first d characters gone (the last ones random)
                pats.append(rnd(d) + site[:L - d])                  # shifted right: the last d characters hang over
                pats.append(synth.mutate(rng, site[d:] + site[:d], nsub=1))
                if d:
                    pats.append(site[:3] + site[3 + d:] + rnd(d))   # d characters deleted inside
                    pats.append(site[:L - 4 - d] + site[L - 4:] + rnd(d))
    pats = [p for p in dict.fromkeys(pats) if 20 <= len(p) <= 32]
    codes = synth.normalize(raw, table)
    text = O.Text(codes, table)
    found = 0
    for esb, eeb in [(8, 0), (0, 8), (6, 7), (7, 6)]:
        E, F = [esb] * len(pats), [eeb] * len(pats)
        for k, ind in [(1, True), (2, True), (1, False), (2, False)]:
            want = O.sorted_tuples(O.find_all(text, pats, engine=8, k=k, indels=ind, esb=E, eeb=F))
            found += len([h for h in want if h[0] < 40 or h[0] > len(raw) - 3])
            for kernel in (sat_amd.KERNEL_SEED, sat_amd.KERNEL_BITPAR):
                got = gpu_hits(codes, table, pats, sat_amd.SEM_EXACT_BASES, k, ind, kernel, esb=E, eeb=F)
                assert got == want, (lead_eos, esb, eeb, k, ind, kernel, len(want), len(got), sorted(set(want) - set(got))[:4], sorted(set(got) - set(want))[:4])
    assert found > 40, found


def test_candidate_overflow_is_reported_and_recovered():
    table = b"ACGT\n"
    codes = synth.normalize(("\n" + "A" * 5000 + "\n").encode(), table)
    pm = sat_amd.PatternMatch(k=0)
    pm.add_pattern("AAAAAAAA", 1)
    pm.init(codes, table)
    pm.set_capacity(16)
    hits = pm.find_all()
    assert hits.size == 5000 - 8 + 1
    pm.close()


def test_halves_seed_overflow_is_recovered():
    """exact_halves -k on the seed kernels reserves output slots 64 at a time: a buffer smaller
    than the reservations must be reported (PM_E_OVERFLOW) and grown by pm_scan, same hits."""
    c, codes, table, allp = load([p for p in CASES if "small_mixed" in p][0])
    want = None
    for cap in (1 << 20, 64, 1000):
        pm = sat_amd.PatternMatch(k=1, indels=True, kernel=sat_amd.KERNEL_SEED)
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        assert pm.selected() == (sat_amd.SEM_EXACT_HALVES, sat_amd.KERNEL_SEED)
        pm.set_capacity(cap)
        got = sat_amd.sorted_tuples(pm.find_all())
        pm.close()
        if want is None:
            want = got
        assert got == want and len(got) > 0, (cap, len(got), len(want))
    assert want == [tuple(h) for h in c["engine"]["auto_k1"]["hits"]]


def test_host_added_edge_records_overflow_reports_the_need():
    """PM_E_OVERFLOW raised by the records the host adds at the stream's edges (pm_api.cpp: edits_start_candidates /
    edits_end_candidates, stream_start_candidates, stream_end_overhang_candidates, the exact_bases -k edge blocks).
    From a record buffer of one entry a whole-stream scan overflows exactly twice: first with the kernels' count, then --
    the buffer now holds just that -- with the kernels' count plus the host's records; the third scan succeeds and
    leaves the records a generous buffer gets."""
    table = b"ACGT\n"
    rng = np.random.default_rng(2033)
    body = "".join("ACGT"[c] for c in rng.integers(0, 4, 2000))
    head, tail = body[:32], body[-32:]
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    codes = synth.normalize(body.encode(), table)
    text = O.Text(codes, table)
    n = codes.size
    cut = lambda L: [head[:L], head[32 - L:], tail[:L], tail[32 - L:]]
    at_start, at_end, beyond = (lambda h: h[0] <= 32), (lambda h: h[0] > n - 4), (lambda h: h[0] > n)
    cases = [
        # edit start / end rules: the automaton's candidates that end in the first Lw + 2k + 2 and the last four characters
        ("edits", dict(k=2, indels=True, semantics=sat_amd.SEM_FILTER_BITVEC), 5, cut(22), 0, lambda h: at_start(h) or at_end(h)),
        # stream_start_candidates: a pattern whose first character is missing in front of stream index 0 (end 19, one error)
        ("start", dict(k=1, indels=False, semantics=sat_amd.SEM_SHIFT_AND_INEXACT), 100, cut(20) + [other(body[0]) + body[:19]], 0, lambda h: h[0] < 20),
        # stream_end_overhang_candidates: the last t pattern characters lie on the zero padding behind the stream
        ("overhang", dict(k=1, indels=False, semantics=sat_amd.SEM_EXACT_HALVES), 12, cut(22) + [tail[-(22 - t):] + "A" * t for t in (1, 2, 5)], 0, beyond),
        # exact_bases -k: occurrences of the mandated first block in the first and last 56 characters
        ("blocks", dict(k=1, indels=True, semantics=sat_amd.SEM_EXACT_BASES), 8, cut(22) + [head[1:22] + "G", "C" + tail[-21:]], 8, lambda h: h[0] < 40 or h[0] > n - 3),
    ]
    for name, opts, eng, pats, esb, is_edge in cases:
        E, F = [esb] * len(pats), [0] * len(pats)
        want = O.sorted_tuples(O.find_all(text, pats, engine=eng, k=opts["k"], indels=opts["indels"], esb=E, eeb=F))
        assert any(is_edge(h) for h in want), (name, want)

        def handle():
            pm = sat_amd.PatternMatch(kernel=sat_amd.KERNEL_SEED, **opts)
            for i, p in enumerate(pats):
                pm.add_pattern(p, i + 1, esb, 0)
            pm.init(codes, table)
            assert pm.selected()[1] == sat_amd.KERNEL_SEED, name
            return pm

        def records(pm, count):
            ptr, cnt = pm.candidates_device()
            assert cnt == count, (name, cnt, count)
            return sorted(r.tobytes() for r in pm.copy_records(ptr, cnt))

        pm = handle()
        pm.scan_async(0, n)
        generous = records(pm, pm.scan_wait())
        pm.close()
        pm = handle()
        capacity, needs, got = 1, [], None
        pm.set_capacity(capacity)
        while got is None:
            assert len(needs) < 4, (name, needs)
            pm.scan_async(0, n)
            try:
                got = pm.scan_wait()
            except sat_amd.PmError as err:
                assert err.code == sat_amd.PM_E_OVERFLOW and "pm_set_capacity" in str(err), (name, err)
                assert err.required > capacity, (name, err.required, capacity)
                needs.append(err.required)
                capacity = err.required
                pm.set_capacity(capacity)
        print(name, "kernel records, with the host's:", needs, "after the scan:", got, "of", len(generous))
        assert len(needs) == 2 and needs[0] < needs[1], (name, needs)
        if name in ("start", "overhang"):
            # no dedup behind these rules and one record per hit: the kernels' records are the oracle's hits inside the
            # stream, the host's the edge hits, and the second need is exactly what the generous buffer ends up holding
            host = sum(1 for h in want if is_edge(h))
            assert needs == [len(generous) - host, len(generous)] and len(generous) == len(want), (name, needs, host, len(generous))
        else:
            assert needs[0] >= got, (name, needs, got)              # (the dedup only ever removes records)
        assert records(pm, got) == generous and got > 0, (name, got, len(generous))
        pm.close()


def test_internal_suspect_buffer_overflow_rescans_inside_the_library():
    """The pair plan's suspect list (between pm_pair_scan and pm_pair_verify) is sized for random streams; on
    3 x 1.4 Mbp of A against A^20 and its neighbours every window is a suspect of every field pair: the
    buffer overflows, the library enlarges it and scans the range again by itself -- the caller's record
    buffer (large enough all along) is neither blamed nor reallocated, pm_scan_wait returns PM_OK -- and
    every window comes back with its distance (shift_and_inexact.cc:249-352, substitutions only)."""
    table = b"ACGT\n"
    lens = [1_400_000, 1_400_000, 1_400_017]
    codes = synth.normalize(("\n" + "".join("A" * n + "\n" for n in lens)).encode(), table)
    pats = ["A" * 20, "A" * 19 + "C", "A" * 7 + "G" + "A" * 6 + "T" + "A" * 5, "C" + "A" * 19, "ACGT" * 5]
    pm = sat_amd.PatternMatch(k=2, indels=False, semantics=sat_amd.SEM_SHIFT_AND_INEXACT, kernel=sat_amd.KERNEL_SEED)
    for i, p in enumerate(pats):
        pm.add_pattern(p, i + 1)
    pm.init(codes, table)
    assert "pm_pair_scan" in pm.describe()
    pm.set_capacity(1 << 25)
    pm.scan_async(0, codes.size)
    n = pm.scan_wait()                                              # no PmError: the rescan is the library's business
    per_pattern = sum(x - 19 for x in lens)
    assert 4 * per_pattern <= n <= 4 * per_pattern + 64          # + the automaton's few stream-start records (shift_and_inexact.cc:162-164)
    ptr, cnt = pm.candidates_device()
    rec = pm.copy_records(ptr, cnt)
    rec = rec[rec["end"] > 24]                                      # past the stream start (ends 21..24 of the first entry dropped)
    for pid, d in ((1, 0), (2, 1), (3, 2), (4, 1)):
        m = rec["pid"] == pid
        assert m.sum() == per_pattern - 4 and (rec["k"][m] == d).all(), (pid, int(m.sum()))
    assert not (rec["pid"] == 5).any()
    pm.close()


def test_device_finalize_equals_host_finalize():
    """pm_finalize_device (hipCUB sort + segmented pass on the GPU) == the host stage, incl. clusters
    on tandem repeats and the deferral at the end of a partial range."""
    c, codes, table, allp = load([p for p in CASES if "varlen_repeats" in p][0])
    n = codes.size
    for k in (1, 2):
        pm = sat_amd.PatternMatch(k=k, indels=False, semantics=sat_amd.SEM_FILTER_BITVEC)
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        cands = pm.scan_candidates(0, n)
        host = sat_amd.sorted_tuples(pm.finalize(cands, n, last=True))
        pm.reset()
        pm.scan_candidates(0, n, to_host=False)
        dev = sat_amd.sorted_tuples(pm.finalize_device(n, last=True))
        assert dev == host and len(host) > 0, (k, len(dev), len(host))
        # two ranges: the first finalize must hold back clusters that may still grow
        pm.reset()
        cut = n // 2
        pm.scan_candidates(0, cut, to_host=False)
        a = sat_amd.sorted_tuples(pm.finalize_device(cut, last=False))
        pm.scan_candidates(cut, n, to_host=False)
        b = sat_amd.sorted_tuples(pm.finalize_device(n, last=True))
        assert sorted(a + b) == host, (k, "split")
        pm.close()


@pytest.mark.parametrize("case", ["varlen_repeats", "dense_indels", "small_mixed"])
def test_device_halves_rule_equals_host_stage(case):
    """exact_halves (-K 1 on whole-pattern candidates with clean-half flags, -k 1 on extended half
    seeds): the per-pattern "end beyond the last kept end" rule as a device sort + walk
    (pm_halves_rule) == the host stage == the oracle, incl. tandem repeats where the rule bites.
    It is stateless: a partial range, or host-side state, sends the caller to pm_finalize."""
    c, codes, table, allp = load([p for p in CASES if case in p][0])
    n = codes.size
    for indels in (False, True):
        pats = [p for p in allp if 16 <= len(p) <= 32] if indels else allp
        if len(pats) < 4:
            continue
        pm = sat_amd.PatternMatch(k=1, indels=indels, semantics=sat_amd.SEM_EXACT_HALVES)
        for i, p in enumerate(pats):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        want = O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=sat_amd.SEM_EXACT_HALVES, k=1, indels=indels))
        pm.scan_candidates(0, n, to_host=False)
        try:
            dev = sat_amd.sorted_tuples(pm.finalize_device(n, last=True))
        except sat_amd.PmError as e:
            assert e.code == -2 and pm.selected()[1] != sat_amd.KERNEL_SEED      # bit-parallel family: host stage only
            pm.close()
            continue
        assert dev == want and len(want) > 0, (case, indels, len(dev), len(want))
        cands = pm.scan_candidates(0, n)
        host = sat_amd.sorted_tuples(pm.finalize(cands, n, last=True))
        assert host == want
        pm.scan_candidates(0, n, to_host=False)
        with pytest.raises(sat_amd.PmError):             # host-side state now exists: not fresh
            pm.finalize_device(n, last=True)
        pm.reset()
        pm.scan_candidates(0, n // 2, to_host=False)
        with pytest.raises(sat_amd.PmError):             # partial range
            pm.finalize_device(n // 2, last=False)
        pm.reset()
        hits = []
        pm.find_patterns(hits, chunk=n + 1)              # pm_scan over the whole stream takes the device path
        assert sorted((h[0], h[1], h[2]) for h in hits) == want
        pm.close()


@pytest.mark.parametrize("case", ["varlen_repeats", "dense_indels", "small_mixed"])
def test_device_cluster_dp_equals_host_stage(case):
    """filter_bitvec with edits on the seed family: pm_finalize_device (sort, chain clusters and the
    banded DP with the reference's end-column and traceback rules on the GPU) == the host stage and
    the golden hits; also in two ranges (clusters that may still grow are held back)."""
    c, codes, table, allp = load([p for p in CASES if case in p][0])
    n = codes.size
    pats = [p for p in allp if 20 <= len(p) <= 32]
    if len(pats) < 4:
        pytest.skip("patterns of this fixture are shorter than 20")
    for k in (2, 1):
        pm = sat_amd.PatternMatch(k=k, indels=True, semantics=sat_amd.SEM_FILTER_BITVEC, kernel=sat_amd.KERNEL_SEED)
        for i, p in enumerate(pats):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        cands = pm.scan_candidates(0, n)
        host = sat_amd.sorted_tuples(pm.finalize(cands, n, last=True))
        want = O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=5, k=k, indels=True))
        assert host == want
        pm.reset()
        pm.scan_candidates(0, n, to_host=False)
        dev = sat_amd.sorted_tuples(pm.finalize_device(n, last=True))
        assert dev == host and len(host) > 0, (case, k, len(dev), len(host))
        pm.reset()
        cut = n // 2
        pm.scan_candidates(0, cut, to_host=False)
        a = sat_amd.sorted_tuples(pm.finalize_device(cut, last=False))
        pm.scan_candidates(cut, n, to_host=False)
        b = sat_amd.sorted_tuples(pm.finalize_device(n, last=True))
        assert sorted(a + b) == host, (case, k, "split")
        pm.close()


def _sharded_owned(codes, table, pats, k, indels, shards, guard, halo=64):
    """Every shard builds its own engine over its slice of the stream (+ guard band + halo), scans
    the guard range and reports what it owns -- bench.py's multi-GPU data path, ranks run in turn."""
    n = codes.size
    size = (n + shards - 1) // shards
    out = []
    for r in range(shards):
        lo, hi = r * size, min(n, (r + 1) * size)
        glo, ghi = max(0, lo - guard - halo), min(n, hi + guard + halo)
        local = np.ascontiguousarray(codes[glo:ghi])
        pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sat_amd.SEM_FILTER_BITVEC,
                                  kernel=sat_amd.KERNEL_SEED if indels else sat_amd.KERNEL_AUTO)
        for i, p in enumerate(pats):
            pm.add_pattern(p, i + 1)
        pm.init(local, table)
        g_lo = 0 if glo == 0 else lo - guard - glo
        g_hi = ghi - glo if ghi == n else hi + guard - glo
        pm.scan_candidates(g_lo, g_hi, to_host=False)
        hits = pm.finalize_device(0, owned=(lo - glo, hi - glo, g_lo, None if ghi == n else g_hi)).copy()
        hits["end"] += glo
        out.append(hits)
        pm.close()
    return out


@pytest.mark.parametrize("case", ["varlen_repeats", "dense_indels"])
@pytest.mark.parametrize("indels", [False, True])
def test_position_sharded_finalize_equals_single_scan(case, indels):
    """shards that finalize their own clusters (pm_finalize_device_owned) concatenate
    to the single-scan filter_bitvec result -- no candidate gather, no merge, text stays local."""
    c, codes, table, allp = load([p for p in CASES if case in p][0])
    pats = [p for p in allp if 20 <= len(p) <= 32] if indels else allp
    if len(pats) < 4:
        pytest.skip("patterns of this fixture are shorter than 20")
    for k in (1, 2):
        want = O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=5, k=k, indels=indels))
        for shards in (2, 3, 7):
            parts = _sharded_owned(codes, table, pats, k, indels, shards, guard=512)
            got = [tuple(int(v) for v in (h["end"], h["pid"], h["k"])) for part in parts for h in part]
            assert sorted(got) == want and len(want) > 0, (case, indels, k, shards, len(got), len(want))


def test_position_sharded_finalize_refuses_cut_chain():
    """A tandem repeat longer than the guard band across a shard edge: the chain's fate is not
    decidable inside the shard, and the call says so instead of reporting a different hit."""
    rng = np.random.default_rng(5)
    left = "".join(rng.choice(list("ACGT"), size=700).tolist())
    right = "".join(rng.choice(list("ACGT"), size=700).tolist())
    ents = [left + "A" * 400 + right]
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    pats = ["A" * 20, left[100:120]]
    want = O.sorted_tuples(O.find_all(O.Text(codes, table), pats, engine=5, k=2, indels=False))
    with pytest.raises(sat_amd.PmError):
        _sharded_owned(codes, table, pats, 2, False, 2, guard=64)
    parts = _sharded_owned(codes, table, pats, 2, False, 2, guard=512)      # wide enough: decided by one shard
    got = [tuple(int(v) for v in (h["end"], h["pid"], h["k"])) for part in parts for h in part]
    assert sorted(got) == want


def test_cli_lines_via_align_hits():
    """Engine hits + pm_align_hits (the CLI's per-hit re-alignment) reproduce the lines the real
    primer_match prints with -A '%i %r %s %e %S %E %d' (tests/golden cli sections)."""
    for path in CASES:
        c, codes, table, allp = load(path)
        n = len(c["patterns"])
        starts, pos = [], 1
        for s_ in c["entries"]:
            starts.append(pos)
            pos += len(s_) + 1
        starts = np.array(starts)
        for name, e in c["cli"].items():
            pm = sat_amd.PatternMatch(k=e["k"], indels=e["indels"])
            for i, p in enumerate(allp):
                pm.add_pattern(p, i + 1)
            pm.init(codes, table)
            hits = pm.find_all()
            al = pm.align_hits(hits)
            lines = []
            for h, a in zip(hits, al):
                assert a["editdist"] <= e["k"], "bogus hit"
                base = starts[np.searchsorted(starts, a["start"], side="right") - 1]
                pid = int(h["pid"])
                lines.append("%d %s %d %d %d %d %d" % (pid - n if pid > n else pid, "R" if pid > n else "F",
                                                     a["start"] - base, a["end"] - base, a["start"], a["end"], a["editdist"]))
            assert sorted(lines) == e["lines"], (c["name"], name)
            pm.close()


@pytest.mark.parametrize("seed", range(3))
def test_exact_base_constraints_vs_oracle(seed):
    """-s/-e style exact_start_bases / exact_end_bases: exact_bases engine and the constrained
    verifies of filter_bitvec / exact_halves (bit-parallel family + host DP)."""
    rng = np.random.default_rng(900 + seed)
    ents = synth.make_entries(rng, 3, int(rng.integers(400, 2000)), n_runs=2, repeats=(seed % 2 == 0))
    L = int(rng.integers(16, 24))
    pats = synth.make_patterns(rng, ents, int(rng.integers(10, 60)), length=L, planted=0.8, indel_frac=0.5)
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    allp = pats + [synth.revcomp(p) for p in pats]
    text = O.Text(codes, table)
    for esb, eeb in [(8, 0), (0, 7), (6, 9), (3, 0)]:
        E, F = [esb] * len(allp), [eeb] * len(allp)
        for sem, k, ind in [(sat_amd.SEM_AUTO, 1, True), (sat_amd.SEM_AUTO, 2, True), (sat_amd.SEM_AUTO, 2, False),
                            (sat_amd.SEM_FILTER_BITVEC, 2, True), (sat_amd.SEM_EXACT_HALVES, 1, True)]:
            eng = {sat_amd.SEM_AUTO: O.pick_engine(text, allp, k, ind, E, F), sat_amd.SEM_FILTER_BITVEC: 5,
                   sat_amd.SEM_EXACT_HALVES: 12}[sem]
            want = O.sorted_tuples(O.find_all(text, allp, engine=eng, k=k, indels=ind, esb=E, eeb=F))
            got = gpu_hits(codes, table, allp, sem, k, ind, sat_amd.KERNEL_AUTO, esb=E, eeb=F)
            assert got == want, (seed, esb, eeb, sem, k, ind, eng, len(want), len(got))


def test_pattern_tiling_gives_identical_hits(monkeypatch):
    """Primer sets too large for one LDS filter are cut into tiles (one launch each): same hit set."""
    c, codes, table, allp = load(CASES[0])
    for k, ind in [(0, True), (1, False), (2, False)]:
        monkeypatch.delenv("PM_SEED_TILE", raising=False)
        one = gpu_hits(codes, table, allp, sat_amd.SEM_AUTO, k, ind, sat_amd.KERNEL_SEED)
        monkeypatch.setenv("PM_SEED_TILE", "37")
        pm = sat_amd.PatternMatch(k=k, indels=ind, kernel=sat_amd.KERNEL_SEED)
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        assert "tiles=%d" % ((len(allp) + 36) // 37) in pm.describe() or "tiles=" in pm.describe()
        many = sat_amd.sorted_tuples(pm.find_all())
        pm.close()
        assert many == one and len(one) > 0, (k, ind)


@pytest.mark.parametrize("seed", range(3))
def test_iupac_wildcards_exact(seed):
    """-w / -W exact search (shift_and with IUPAC classes) on the bit-parallel family vs the oracle."""
    rng = np.random.default_rng(800 + seed)
    ents = synth.make_entries(rng, 3, int(rng.integers(500, 3000)), n_runs=5, repeats=(seed % 2 == 0))
    L = int(rng.integers(8, 14))
    pats = []
    for p in synth.make_patterns(rng, ents, int(rng.integers(10, 80)), length=L, planted=0.9, indel_frac=0.0, extras=False):
        p = list(p)
        for _ in range(int(rng.integers(0, 3))):
            p[int(rng.integers(0, len(p)))] = str(rng.choice(list("RYKMSWBDHVN")))
        pats.append("".join(p))
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    text = O.Text(codes, table)
    for tn in (False, True):
        want = O.sorted_tuples(O.find_all(text, pats, engine=4, k=0, wildcards=True, text_n=tn))
        pm = sat_amd.PatternMatch(k=0, wildcards=True, text_n=tn)
        for i, p in enumerate(pats):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        assert pm.selected()[0] == sat_amd.SEM_SHIFT_AND             # (-w on an A,C,G,T,N stream: the seed family takes the primers it can expand)
        got = sat_amd.sorted_tuples(pm.find_all())
        pm.close()
        assert got == want and len(want) > 0, (seed, tn, len(want), len(got))


@pytest.mark.parametrize("seed", range(3))
def test_iupac_wildcards_inexact(seed):
    """-w / -W with k > 0: the engines pick_pattern_index chooses (exact_halves over shift_and for
    k = 1, filter_bitvec for k = 2) and forced ones, edits and substitutions, raw and normalized
    streams, vs the oracle (which tests/test_oracle_vs_ref.py pins to the reference); also the
    caller's re-alignment (editdist_alignment with wildcard-equal cells)."""
    rng = np.random.default_rng(950 + seed)
    ents = synth.make_entries(rng, 3, int(rng.integers(500, 3000)), n_runs=5, repeats=(seed % 2 == 0))
    L = int(rng.integers(14, 22))
    pats = []
    for p in synth.make_patterns(rng, ents, int(rng.integers(10, 60)), length=L, planted=0.9, indel_frac=0.3, extras=False):
        p = list(p)
        for _ in range(int(rng.integers(0, 3))):
            p[int(rng.integers(0, len(p)))] = str(rng.choice(list("RYKMSWBDHVN")))
        pats.append("".join(p))
    table = synth.table_for(ents)
    raw = np.frombuffer(synth.stream(ents), dtype=np.uint8)
    codes = synth.normalize(synth.stream(ents), table)
    total = 0
    for stream_codes, tbl in ((codes, table), (raw, None)):
        text = O.Text(stream_codes, tbl)
        for tn in (False, True):
            for k in (1, 2):
                for indels in (True, False):
                    for sem in (sat_amd.SEM_AUTO, sat_amd.SEM_FILTER_BITVEC, 14, sat_amd.SEM_SHIFT_AND_INEXACT):
                        want = O.find_all(text, pats, engine=sem, k=k, indels=indels, wildcards=True, text_n=tn)
                        pm = sat_amd.PatternMatch(k=k, indels=indels, wildcards=True, text_n=tn, semantics=sem)
                        for i, p in enumerate(pats):
                            pm.add_pattern(p, i + 1)
                        pm.init(stream_codes, tbl)
                        assert pm.selected()[1] in (sat_amd.KERNEL_BITPAR, sat_amd.KERNEL_SEED)
                        hits = pm.find_all()
                        got = sat_amd.sorted_tuples(hits)
                        assert got == O.sorted_tuples(want), (seed, tbl is None, tn, k, indels, sem, len(got), len(want))
                        total += len(got)
                        if sem == sat_amd.SEM_AUTO and len(got):
                            al = pm.align_hits(hits)
                            for h, a in zip(hits[:50], al[:50]):
                                rc, st, en, ed, val = O.cli_align(text, pats[int(h["pid"]) - 1], int(h["end"]), k, indels, wildcards=True, text_n=tn)
                                if ed == 2**31 - 1:        # no alignment within k at this end ("Bogus hit"): only that verdict is defined
                                    assert a["editdist"] == ed, (seed, h)
                                else:
                                    assert (a["start"], a["end"], a["editdist"], a["value"]) == (st, en, ed, val), (seed, h)
                        pm.close()
    assert total > 0


@pytest.mark.parametrize("seed", range(4))
def test_edit_distance_seed_plan(seed):
    """filter_bitvec / shift_and_inexact with edits (-k 1, -k 2) on the seed kernels: displaced-piece
    seeds, per-seed automaton run, device dedup -- raw candidates and final hits equal the oracle's,
    normalized and raw streams, incl. the stream start (prefix rows), N runs and a short entry."""
    rng = np.random.default_rng(1200 + seed)
    ents = synth.make_entries(rng, 3, int(rng.integers(2000, 9000)), n_runs=3, repeats=(seed % 2 == 0), short=True)
    L = int(rng.integers(20, 27))
    pats = [p for p in synth.make_patterns(rng, ents, int(rng.integers(30, 200)), length=L, planted=0.8, indel_frac=0.5, extras=False)
            if 20 <= len(p) <= 32]
    pats.append(ents[0][2:2 + L])                       # a pattern whose first two characters lie before the stream start
    pats.append(ents[0][:L])
    pats = [p for p in pats if set(p) <= set("ACGT")]   # the seed family takes A,C,G,T patterns
    table = synth.table_for(ents)
    raw = np.frombuffer(synth.stream(ents), dtype=np.uint8)
    codes = synth.normalize(synth.stream(ents), table)
    total = 0
    for stream_codes, tbl in ((codes, table), (raw, None)):
        text = O.Text(stream_codes, tbl)
        for k in (2, 1):
            for sem in (sat_amd.SEM_SHIFT_AND_INEXACT, sat_amd.SEM_FILTER_BITVEC):
                want = O.sorted_tuples(O.find_all(text, pats, engine=sem, k=k, indels=True))
                for chunk in (1 << 26, 1500):
                    pm = sat_amd.PatternMatch(k=k, indels=True, semantics=sem, kernel=sat_amd.KERNEL_SEED)
                    for i, p in enumerate(pats):
                        pm.add_pattern(p, i + 1)
                    pm.init(stream_codes, tbl)
                    assert pm.selected() == (sem, sat_amd.KERNEL_SEED)
                    got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
                    pm.close()
                    assert got == want, (seed, tbl is None, k, sem, chunk, len(got), len(want))
                total += len(want)
    assert total > 0


@pytest.mark.parametrize("env", [{"PM_EDIT_SCAN": "bloom"}, {"PM_EDIT_TABLE_LOG": "16"}, {"PM_EDIT_TABLE_LOG": "26"},
                                 {"PM_SEED_CHUNK": "16384", "PM_SEED_GROUP": "3"}, {"PM_SEED_CHUNK": "2097152"},
                                 {"PM_EDIT_SCAN": "hash"}, {"PM_EDIT_SCAN": "hash", "PM_EDIT_TABLE_LOG": "16"},
                                 {"PM_EDIT_SCAN": "hash", "PM_SEED_CHUNK": "16384", "PM_SEED_GROUP": "3"}, {"PM_PAIR_ROW": "3"}])
def test_edit_distance_plan_switches(env, monkeypatch):
    """The edit-distance plan's first stage under its switches.  -k 2 runs on the pair geometry (pm_pair_edit_scan; round 4)
    unless PM_EDIT_SCAN says otherwise, -k 1 on the hashed-piece plan: the round-1 form (Bloom survivors compacted,
    PM_EDIT_SCAN=bloom), round 2's pm_edit_scan (PM_EDIT_SCAN=hash for -k 2) with a tiny and a huge key map (2^16 bits: nearly every Bloom survivor is
    suspicious; 2^26), small chunks with runs of three per combo, 2 Mi chunks.  Thousands of decoy patterns fill the
    filters and the buckets (full 16-slot buckets, several patterns with the same twelve bases); same candidates
    and hits as the oracle (shift_and_inexact.cc:249-352, filter_bitvec.cc:88-177)."""
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    rng = np.random.default_rng(4242)
    ents = synth.make_entries(rng, 4, 6000, n_runs=2, repeats=True, short=True)
    pats = [p for p in synth.make_patterns(rng, ents, 150, length=22, planted=0.9, indel_frac=0.6, extras=False) if 20 <= len(p) <= 32 and set(p) <= set("ACGT")]
    base = pats[0]
    pats += [base[:-12] + "".join(rng.choice(list("ACGT"), size=12).tolist()) for _ in range(40)]      # shared leading bases
    pats += ["".join(rng.choice(list("ACGT"), size=10).tolist()) + base[-12:] for _ in range(40)]       # the same last twelve bases: one key, many patterns
    pats += ["".join(rng.choice(list("ACGT"), size=21).tolist()) for _ in range(3000)]                  # decoys
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    text = O.Text(codes, table)
    for k, sem in ((2, sat_amd.SEM_SHIFT_AND_INEXACT), (2, sat_amd.SEM_FILTER_BITVEC), (1, sat_amd.SEM_SHIFT_AND_INEXACT)):
        want = O.sorted_tuples(O.find_all(text, pats, engine=sem, k=k, indels=True))
        pm = sat_amd.PatternMatch(k=k, indels=True, semantics=sem, kernel=sat_amd.KERNEL_SEED)
        for i, p in enumerate(pats):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        assert pm.selected() == (sem, sat_amd.KERNEL_SEED)
        got = sat_amd.sorted_tuples(pm.find_all())
        pm.close()
        assert len(want) > 50
        assert got == want, (env, k, sem, len(got), len(want))


@pytest.mark.parametrize("env", [{}, {"PM_HALF_SCAN": "bloom"}, {"PM_SEED_CHUNK": "16384"}])
def test_exact_halves_edits_plans(env, monkeypatch):
    """exact_halves -k 1 / -k 2 (exact_halves.cc:120-224: exact seeds of the halves, banded extension of the partner)
    on the ranked plan (pm_half_scan + pm_half_verify: key bitmap + rank directory in LDS, partner test on the
    carried stream bases) and on the round-1 form behind PM_HALF_SCAN=bloom.  Patterns of 20..32 characters -- for
    31 and 32 the partner window does not fit the carried bases and every key hit goes to the verify kernel --, many
    halves with the same last ten bases (more than the slot's seven), N runs, a short entry, the stream's ends."""
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    rng = np.random.default_rng(777)
    ents = synth.make_entries(rng, 4, 7000, n_runs=3, repeats=True, short=True)
    pats = []
    for L in (20, 21, 25, 26, 30, 31, 32):
        pats += [p for p in synth.make_patterns(rng, ents, 40, length=L, planted=0.9, indel_frac=0.5, extras=False) if 20 <= len(p) <= 32 and set(p) <= set("ACGT")]
    base = pats[0]
    h = len(base) // 2
    pats += ["".join(rng.choice(list("ACGT"), size=h - 10).tolist()) + base[h - 10:h] + "".join(rng.choice(list("ACGT"), size=len(base) - h).tolist()) for _ in range(12)]   # left halves with one key
    pats += [base[:h] + "".join(rng.choice(list("ACGT"), size=len(base) - h - 10).tolist()) + base[-10:] for _ in range(12)]                                                   # right halves with one key
    pats += [ents[0][:24], ents[-1][-26:]]                                  # at the stream's ends
    pats += ["".join(rng.choice(list("ACGT"), size=22).tolist()) for _ in range(2500)]   # decoys
    pats = [p for p in pats if set(p) <= set("ACGT") and 20 <= len(p) <= 32]
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    raw = np.frombuffer(synth.stream(ents), dtype=np.uint8)
    for stream_codes, tbl in ((codes, table), (raw, None)):
        text = O.Text(stream_codes, tbl)
        for k in (1, 2):
            want = O.sorted_tuples(O.find_all(text, pats, engine=sat_amd.SEM_EXACT_HALVES, k=k, indels=True))
            pm = sat_amd.PatternMatch(k=k, indels=True, semantics=sat_amd.SEM_EXACT_HALVES, kernel=sat_amd.KERNEL_SEED)
            for i, p in enumerate(pats):
                pm.add_pattern(p, i + 1)
            pm.init(stream_codes, tbl)
            assert pm.selected() == (sat_amd.SEM_EXACT_HALVES, sat_amd.KERNEL_SEED)
            got = sat_amd.sorted_tuples(pm.find_all())
            pm.close()
            assert len(want) > 100
            assert got == want, (env, tbl is None, k, len(got), len(want))
    # a set of 32-mers only: no half fits the ranked plan's partner test, the round-1 form takes the set
    long_pats = [p for p in synth.make_patterns(rng, ents, 60, length=32, planted=0.9, indel_frac=0.5, extras=False) if len(p) in (31, 32) and set(p) <= set("ACGT")]
    text = O.Text(codes, table)
    want = O.sorted_tuples(O.find_all(text, long_pats, engine=sat_amd.SEM_EXACT_HALVES, k=1, indels=True))
    pm = sat_amd.PatternMatch(k=1, indels=True, semantics=sat_amd.SEM_EXACT_HALVES, kernel=sat_amd.KERNEL_SEED)
    for i, p in enumerate(long_pats):
        pm.add_pattern(p, i + 1)
    pm.init(codes, table)
    assert "pm_half_scan" not in pm.describe()
    assert sat_amd.sorted_tuples(pm.find_all()) == want and len(want) > 10
    pm.close()
    # pattern tiles of both kinds in one handle: the first tile is made of the 32-mers (round-1 form), the second of 22-mers (ranked)
    monkeypatch.setenv("PM_SEED_TILE", str(2 * len(long_pats)))
    mixed = long_pats + [p for p in pats if len(p) == 22][:len(long_pats)]
    want = O.sorted_tuples(O.find_all(text, mixed, engine=sat_amd.SEM_EXACT_HALVES, k=1, indels=True))
    pm = sat_amd.PatternMatch(k=1, indels=True, semantics=sat_amd.SEM_EXACT_HALVES, kernel=sat_amd.KERNEL_SEED)
    for i, p in enumerate(mixed):
        pm.add_pattern(p, i + 1)
    pm.init(codes, table)
    assert "tiles=2" in pm.describe(), pm.describe()
    assert sat_amd.sorted_tuples(pm.find_all()) == want
    pm.close()


def test_edit_distance_device_text_with_repeat_clusters():
    """Stream only in HBM (pm_init_device) + tandem repeats: the long repeat clusters that
    pm_cluster_dp hands back go through the host stage, whose window gather must not disturb the
    device results waiting to be copied (regression: it once freed the sort workspace)."""
    import torch
    rng = np.random.default_rng(77)
    ents = synth.make_entries(rng, 3, 20000, n_runs=2, repeats=True, short=True)
    pats = synth.make_patterns(rng, ents, 300, length=20, planted=0.3)
    allp = [p for p in pats + [synth.revcomp(p) for p in pats] if set(p) <= set("ACGT") and len(p) >= 20]
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    dev = torch.from_numpy(codes).to("cuda:0")
    want = O.sorted_tuples(O.find_all(O.Text(codes, table), allp, engine=5, k=2, indels=True))
    for chunk in (1 << 26, 7000):
        pm = sat_amd.PatternMatch(k=2, indels=True)
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init_device(dev.data_ptr(), dev.numel(), table, keepalive=dev)
        assert pm.selected() == (sat_amd.SEM_FILTER_BITVEC, sat_amd.KERNEL_SEED)
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        pm.close()
        assert got == want and len(want) > 0, (chunk, len(got), len(want))


def test_large_host_stream_upload_equals_device_stream():
    """pm_init with a host stream large enough for the threaded, pinned-staged upload that runs
    beside the table build (pm_api.cpp upload_stream): same hits as the same bytes handed over
    already resident (pm_init_device), and the planted sites are all there."""
    import torch
    rng = np.random.default_rng(2026)
    n = 100_000_000 + 12345                                  # not a multiple of the staging chunk
    codes = rng.integers(0, 4, size=n, dtype=np.uint8)
    codes[0] = 4
    codes[-1] = 4
    codes[rng.integers(1, n - 1, size=40)] = 4               # entry separators
    table = b"ACGT\n"
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    pats, sites = [], []
    for t in range(200):
        a = int(rng.integers(1, n - 40))
        w = codes[a:a + 20]
        if (w > 3).any():
            continue
        pats.append(lut[w].tobytes().decode())
        sites.append(a + 20)
    # sites near the slice edges of the upload threads (6 slices, 8 MiB chunks)
    for a in (n // 6 - 10, 2 * (n // 6) + 3, (8 << 20) - 7, n - 30):
        w = codes[a:a + 20]
        if (w <= 3).all():
            pats.append(lut[w].tobytes().decode())
            sites.append(a + 20)
    res = []
    for mode in ("host", "device"):
        pm = sat_amd.PatternMatch(k=1, indels=False)
        for i, p in enumerate(pats):
            pm.add_pattern(p, i + 1)
        if mode == "host":
            pm.init(codes, table)
        else:
            dev = torch.from_numpy(codes).to("cuda:0")
            pm.init_device(dev.data_ptr(), dev.numel(), table, keepalive=dev)
        res.append(sat_amd.sorted_tuples(pm.find_all()))
        pm.close()
    assert res[0] == res[1] and len(res[0]) >= len(pats)
    found = {(e, p) for e, p, k in res[0] if k == 0}
    assert all((sites[i], i + 1) in found for i in range(len(pats)))


def test_mixed_pattern_set_splits_between_engines():
    """A primer list is rarely uniform.  A few patterns the seed plan does not take (an ambiguity
    letter, 17 or 40 characters) are scanned by the bit-parallel kernels into the same record
    buffer; everything else stays on the seed family.  Same hits as the oracle's engine for every
    option set whose engines report one inner pattern per pattern."""
    rng = np.random.default_rng(99)
    ents = synth.make_entries(rng, 4, 6000, n_runs=2, repeats=True, short=True)
    base = [p for p in synth.make_patterns(rng, ents, 120, length=22, planted=0.8) if set(p) <= set("ACGT") and len(p) >= 20]
    odd = []
    e0 = ents[0]
    for a in (100, 900, 1700):
        w = e0[a:a + 21]
        if set(w) <= set("ACGT"):
            odd.append(w[:9] + "N" + w[10:])                       # an N in the pattern: a mismatch everywhere (no -w)
            odd.append(w[:17])                                     # too short for the edit-distance plan
    w = ents[1][300:340]
    if set(w) <= set("ACGT"):
        odd.append(w)                                              # too long for every seed plan
        odd.append(synth.mutate(rng, w, nsub=1))
    assert len(odd) >= 4
    pats = base[:40] + odd + base[40:]
    allp = pats + [synth.revcomp(p) if set(p) <= set("ACGT") else p for p in pats]
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    text = O.Text(codes, table)
    for k, indels, sem in ((0, False, sat_amd.SEM_AUTO), (2, False, sat_amd.SEM_AUTO), (2, True, sat_amd.SEM_AUTO), (1, True, sat_amd.SEM_FILTER_BITVEC),
                           (2, True, sat_amd.SEM_SHIFT_AND_INEXACT), (1, False, sat_amd.SEM_SHIFT_AND_INEXACT)):
        pm = sat_amd.PatternMatch(k=k, indels=indels, semantics=sem)
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init(codes, table)
        s, kern = pm.selected()
        assert kern == sat_amd.KERNEL_SEED and "patterns the seed plan does not take" in pm.describe(), (k, indels, pm.describe())
        want = O.sorted_tuples(O.find_all(text, allp, engine=s, k=k, indels=indels))
        for chunk in (1 << 26, 5000):
            got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
            assert got == want and len(want) > 0, (k, indels, sem, chunk, len(got), len(want))
        if s == sat_amd.SEM_FILTER_BITVEC:                         # device clustering sees both engines' records
            pm.reset()
            pm.scan_candidates(0, codes.size, to_host=False)
            assert sat_amd.sorted_tuples(pm.finalize_device(codes.size, last=True)) == want
        pm.close()
    # every pattern outside the seed plan: one engine, as before
    pm = sat_amd.PatternMatch(k=2, indels=True)
    for i, p in enumerate(odd):
        pm.add_pattern(p, i + 1)
    pm.init(codes, table)
    assert pm.selected()[1] == sat_amd.KERNEL_BITPAR
    pm.close()


def test_large_hit_lists_come_back_sorted():
    """(end, pid, k) order of a hit list large enough for the sliced, threaded sort (pm_api.cpp
    sort_hits), incl. many equal ends and a skewed distribution of ends."""
    rng = np.random.default_rng(31)
    pm = sat_amd.PatternMatch(k=0)
    pm.add_pattern("ACGTACGTACGTACGTACGT", 1)
    pm.init(np.frombuffer(b"\nACGTACGTACGTACGTACGTAC\n", dtype=np.uint8).copy())
    n = 300_000
    for ends in (rng.integers(1, 1 << 33, size=n), rng.integers(1, 5000, size=n),
                 np.concatenate([rng.integers(1, 100, size=n - 10), rng.integers(1 << 35, 1 << 36, size=10)])):
        c = np.zeros(n, dtype=sat_amd.HIT_DTYPE)
        c["end"] = ends
        c["pid"] = rng.integers(1, 1000, size=n)
        c["k"] = rng.integers(0, 3, size=n)
        got = pm.finalize(c, 1 << 40, last=True, sort=True)          # keyword_tree: pass-through, then the sort
        order = np.lexsort((c["k"], c["pid"], c["end"]))
        assert got.size == n
        assert (got["end"] == c["end"][order]).all() and (got["pid"] == c["pid"][order]).all() and (got["k"] == c["k"][order]).all()
    pm.close()


@pytest.mark.parametrize("path", CASES, ids=[os.path.basename(p)[:-5] for p in CASES])
def test_golden_engine_hits_with_two_mi_chunks(path, monkeypatch):
    """the chunk size large ranges get by default (2 Mi positions per workgroup), forced on the fixtures"""
    monkeypatch.setenv("PM_SEED_CHUNK", "2097152")
    c, codes, table, allp = load(path)
    for name, e in c["engine"].items():
        got = gpu_hits(codes, table, allp, SEL2SEM[e["sel"]], e["k"], e["indels"], sat_amd.KERNEL_AUTO)
        assert got == [tuple(h) for h in e["hits"]], (c["name"], name)


@pytest.mark.parametrize("seed", range(4))
def test_exact_zones_on_the_seed_family(seed):
    """-s/-e/-5/-3 style exact zones with substitution-only search (-K) on 20..32 character primers stay
    on the seed family (pair plan): its exact verify knows the zones -- a substitution inside one fails
    the reference's constrained verifies (pattern_alignment.cc:320-323, primer_alignment.cc:155) --
    for filter_bitvec (zone violations still chain, filter_bitvec.cc:103-116), exact_halves and
    exact_bases (exact_bases.cc:92-121).  Edits (-k): filter_bitvec's cluster DPs and exact_halves'
    extension DPs take the zones on the GPU as before."""
    rng = np.random.default_rng(1200 + seed)
    ents = synth.make_entries(rng, 3, int(rng.integers(600, 2500)), n_runs=2, repeats=(seed % 2 == 0))
    L = int(rng.integers(20, 27))
    pats = synth.make_patterns(rng, ents, int(rng.integers(20, 80)), length=L, planted=0.85)
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    allp = pats + [synth.revcomp(p) for p in pats]
    text = O.Text(codes, table)
    for esb, eeb in [(8, 0), (0, 7), (6, 9), (3, 0), (0, 12)]:
        E, F = [esb] * len(allp), [eeb] * len(allp)
        for sem, k, ind in [(sat_amd.SEM_AUTO, 1, False), (sat_amd.SEM_AUTO, 2, False), (sat_amd.SEM_FILTER_BITVEC, 2, False),
                            (sat_amd.SEM_FILTER_BITVEC, 1, False), (sat_amd.SEM_EXACT_HALVES, 2, False), (sat_amd.SEM_EXACT_HALVES, 1, False),
                            (sat_amd.SEM_FILTER_BITVEC, 2, True), (sat_amd.SEM_EXACT_HALVES, 1, True),
                            (sat_amd.SEM_AUTO, 2, True), (sat_amd.SEM_AUTO, 1, True), (sat_amd.SEM_EXACT_BASES, 1, True), (sat_amd.SEM_EXACT_BASES, 2, True),
                            (sat_amd.SEM_EXACT_BASES, 2, False)]:
            if sem == sat_amd.SEM_EXACT_BASES and max(esb, eeb) < 6:
                continue                                              # select.cc:131: exact_bases needs >= 6 mandated bases
            eng = {sat_amd.SEM_AUTO: O.pick_engine(text, allp, k, ind, E, F), sat_amd.SEM_FILTER_BITVEC: 5, sat_amd.SEM_EXACT_HALVES: 12,
                   sat_amd.SEM_EXACT_BASES: 8}[sem]
            want = O.sorted_tuples(O.find_all(text, allp, engine=eng, k=k, indels=ind, esb=E, eeb=F))
            pm = sat_amd.PatternMatch(k=k, indels=ind, semantics=sem)
            for i, p in enumerate(allp):
                pm.add_pattern(p, i + 1, E[i], F[i])
            pm.init(codes, table)
            assert pm.selected()[1] == sat_amd.KERNEL_SEED, (esb, eeb, sem, k, ind, pm.describe())
            got = sat_amd.sorted_tuples(pm.find_all())
            assert got == want, (seed, esb, eeb, sem, k, ind, eng, len(want), len(got))
            # resumable: small consecutive ranges (seeds and chains across range edges) give the same hits
            assert sat_amd.sorted_tuples(pm.find_all(chunk=193)) == want, (seed, esb, eeb, sem, k, ind, "chunked")
            pm.close()


@pytest.mark.parametrize("seed", range(3))
def test_ambiguous_primers_stay_on_the_seed_family(seed):
    """-w with a few ambiguous primers in a set of plain ones (shift_and.cc:108-117: a pattern
    character accepts the stream letters of its IUPAC compatibility set): primers with up to two
    ambiguity letters are expanded into their concrete variants at table build and scanned by the
    seed kernels; a primer with more goes to the bit-parallel residue engine beside them.  Exact,
    -K 2 and -k 2; hit sets vs the oracle."""
    rng = np.random.default_rng(1500 + seed)
    ents = synth.make_entries(rng, 3, int(rng.integers(1500, 4000)), n_runs=3, repeats=(seed % 2 == 0))
    L = int(rng.integers(20, 26))
    pats = synth.make_patterns(rng, ents, 300, length=L, planted=0.7, indel_frac=0.3, extras=False)
    amb = 0
    for i in range(0, len(pats), 9):                                   # every ninth primer gets one or two ambiguity letters
        p = list(pats[i])
        for _ in range(1 + (i // 9) % 2):
            p[int(rng.integers(0, len(p)))] = str(rng.choice(list("RYKMSWBDHVN")))
        pats[i] = "".join(p)
        amb += 1
    p = list(pats[1])                                                  # one primer beyond the expansion limit
    for j in (2, 5, 9, 13):
        p[j] = "N"
    pats[1] = "".join(p)
    allp = pats + [synth.revcomp_iupac(q) for q in pats]
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    text = O.Text(codes, table)
    for k, indels in ((0, True), (2, False), (2, True)):
        eng = 4 if k == 0 else 5
        want = O.sorted_tuples(O.find_all(text, allp, engine=eng, k=k, indels=indels, wildcards=True, text_n=False))
        pm = sat_amd.PatternMatch(k=k, indels=indels, wildcards=True, text_n=False)
        for i, q in enumerate(allp):
            pm.add_pattern(q, i + 1)
        pm.init(codes, table)
        assert pm.selected()[1] == sat_amd.KERNEL_SEED and "patterns the seed plan does not take" in pm.describe(), pm.describe()
        got = sat_amd.sorted_tuples(pm.find_all())
        assert got == want and len(want) > 20, (seed, k, indels, len(want), len(got))
        assert sat_amd.sorted_tuples(pm.find_all(chunk=997)) == want, (seed, k, indels, "chunked")
        pm.close()


def test_round4_introspection_calls():
    """pm_scan_stats / pm_prepare_device / pm_measure_pair_edit_floor (include/pm_gpu.h, round 4): counters that add up, and the
    measurement call refuses a handle that is not a -K 2 pair-plan handle."""
    import ctypes as C
    L = sat_amd.load_library()
    assert L.pm_prepare_device(0) == 0
    rng = np.random.default_rng(31)
    ents = synth.make_entries(rng, 3, 30000, n_runs=1, repeats=False)
    pats = synth.make_patterns(rng, ents, 400, length=20, planted=0.5)
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    pm = sat_amd.PatternMatch(k=2, indels=False)
    for i, p in enumerate(pats):
        pm.add_pattern(p, i + 1)
    pm.init(codes, table)
    cands = pm.scan_candidates(0, codes.size)
    st = pm.scan_stats()
    assert st["candidates"] == cands.size and st["between_stages"] >= cands.size // 6 and st["internal_rescans"] == 0, (st, cands.size)
    ms1, s1 = pm.measure_pair_edit_floor(1)
    ms2, s2 = pm.measure_pair_edit_floor(2)
    assert ms1 > 0 and ms2 > 0 and s1 > 0 and s2 > 0, (ms1, ms2, s1, s2, st)
    assert sat_amd.sorted_tuples(pm.scan_candidates(0, codes.size)) == sat_amd.sorted_tuples(cands)   # the handle is unharmed
    pm.close()
    pe = sat_amd.PatternMatch(k=2, indels=True)
    for i, p in enumerate(pats):
        pe.add_pattern(p, i + 1)
    pe.init(codes, table)
    with pytest.raises(sat_amd.PmError) as ei:
        pe.measure_pair_edit_floor(1)
    assert ei.value.code == -2
    assert "pm_pair_edit_scan" in pe.describe()
    pe.scan_candidates(0, codes.size, to_host=False)
    assert pe.scan_stats()["between_stages"] > 0
    pe.close()


@pytest.mark.parametrize("k,indels", [(0, False), (2, False), (2, True), (1, True)])
def test_pm_scan_order_with_pattern_ids_in_any_order(k, indels):
    """pm_scan hands its hits out in (end, pid, k) order.  With pattern ids that grow with the pattern index (what the reference's
    callers add, primer_match.cc:1105-1107) the order comes from one keys-only radix sort on the device (pm_cluster.hip
    sort_final_device: key = end | pattern index | k); with ids in any other order the host sorts.  Both must give the oracle's
    hits in that order, whole and in small ranges.  (A handful of hits per range here: whether the host-sorted landing gets out
    of the way of the next range's look-ahead scan is decided by tests/test_gpu_scan_lookahead.py, on ranges of 2^21 hits.)"""
    rng = np.random.default_rng(77 + k)
    ents = synth.make_entries(rng, 3, 5000, n_runs=2, repeats=True)
    pats = synth.make_patterns(rng, ents, 200, length=22, planted=0.8, indel_frac=0.3 if indels else 0.0, extras=False)
    pats = [p for p in pats if 20 <= len(p) <= 32 and set(p) <= set("ACGT")]
    table = synth.table_for(ents)
    codes = synth.normalize(synth.stream(ents), table)
    text = O.Text(codes, table)
    for ids in (list(range(1, len(pats) + 1)), [5 * (len(pats) - i) + 3 for i in range(len(pats))], [int(x) for x in rng.permutation(len(pats)) * 7 + 11]):
        eng = O.pick_engine(text, pats, k, indels)
        want = O.sorted_tuples(O.find_all(text, pats, engine=eng, k=k, indels=indels, ids=ids))
        pm = sat_amd.PatternMatch(k=k, indels=indels)
        for p, i in zip(pats, ids):
            pm.add_pattern(p, i)
        pm.init(codes, table)
        for chunk in (1 << 26, 777):
            pm.reset()
            got, pos = [], 0
            while pos < codes.size:
                e = min(codes.size, pos + chunk)
                v = pm.scan_view(pos, e)
                got += list(zip(v["end"].tolist(), v["pid"].tolist(), v["k"].tolist()))
                pos = e
            assert got == sorted(got), (k, indels, ids[:3], chunk, "not in (end, pid, k) order")
            assert got == want, (k, indels, ids[:3], chunk, len(got), len(want))
        pm.close()
