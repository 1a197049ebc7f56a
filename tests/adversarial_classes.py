"""tests/adversarial.py's small cases with every opt-in primer class in one list: each primer drawn from a length band of
its own -- 16..19 (the short classes), 20..32 (the main class), 33..64 (wide tiles, 4.9 .. 4.12), now
and then 12..15 and 65..70 (the bit-parallel residue) -- under -w with 0 .. 5 ambiguity letters per primer (plain, expanded
into the main class, or the degenerate class of pm_wild_sub_scan, 4.13), and `route`: the permission bits of
pm_config.long_patterns as keyword arguments of sat_amd.PatternMatch, all seven on three cases in four, a random subset on
the fourth.  Streams, zones, engines, k, knobs, record caps, modes as in adversarial.small_case.  Shared by
tests/test_gpu_adversarial_classes.py (fixed seeds) and scripts/fuzz_families.py --oracle --classes (open-ended)."""
import numpy as np

import adversarial as A
import sat_amd

BITS = ("long_patterns", "long_exact", "long_edits", "long_halves", "long_align", "wild_class", "edit_pair")
# (lo, hi, weight) of a primer's length band
BANDS = ((16, 19, 3.0), (20, 32, 3.0), (33, 64, 4.0), (12, 15, 0.5), (65, 70, 0.5))
R806 = "GGACTACNVGGGTWTCTAAT"                                       # 806R: 24 concrete variants
VARIANTS = {c: 1 for c in "ACGT"}
VARIANTS.update({c: 2 for c in "RYKMSW"})
VARIANTS.update({c: 3 for c in "BDHV"})
VARIANTS["N"] = 4


def variants(p):
    v = 1
    for ch in p:
        v *= VARIANTS[ch]
    return v


def kind(p):
    """plain / expanded (at most 16 concrete variants) / degenerate (more)"""
    v = variants(p)
    return "plain" if v == 1 else "expanded" if v <= 16 else "degenerate"


def class_case(seed):
    """One case of the shape of adversarial.small_case (its keys, so that describe / gpu_hits / oracle_hits take it) plus
    `route` and `lens`, the primers' lengths.  600 .. 8000 characters, 4 .. 80 primers x 2 strands."""
    rng = np.random.default_rng([seed, 0xC1A55])                      # (a stream of its own: no case shares its text with small_case(seed))
    style = int(rng.integers(0, 4))
    n = int(rng.integers(600, 8001))
    s = A.make_stream(rng, n, style)
    k = int(rng.integers(0, 3))
    indels = bool(rng.integers(0, 2)) and k > 0
    count = int(rng.integers(4, 81))
    # now and then a residue: five lists in eight have neither a primer of 12..15 nor one of 65..70 characters (exact_halves
    # keeps no residue, and one primer of 10..15 characters keeps a -K list off the pair plan: DESIGN.md 4.8, 4.9, 4.12), one has
    # the long ones only, one the short ones only, one has both
    residue = (0, 0, 0, 0, 0, 2, 1, 3)[int(rng.integers(0, 8))]
    w = np.array([b[2] for b in BANDS])
    w[3] *= residue & 1
    w[4] *= residue >> 1
    pats = []
    for b in rng.choice(len(BANDS), size=count, p=w / w.sum()):
        lo, hi, _ = BANDS[int(b)]
        pats += A.make_patterns(rng, s, 1, lo, hi, k)
    allp = pats + [sat_amd.reverse_comp(p) for p in pats]
    wild = bool(rng.integers(0, 3) == 0)                              # ambiguity codes in the primers (-w) on a third of the cases
    if wild:
        wp = []
        for p in allp:
            q = list(p)
            for _ in range(int(rng.integers(0, 6))):                  # 0 .. 5 ambiguity letters
                i = int(rng.integers(0, len(q)))
                if q[i] in A.IUPAC:
                    q[i] = A.IUPAC[q[i]][int(rng.integers(0, 7))]
            wp.append("".join(q))
        allp = wp
        if rng.integers(0, 3) == 0:                                   # 806R, forward and reversed: two primers of 24 concrete variants
            allp += [R806, R806[::-1]]
    sem, sname = A.SEMS[int(rng.integers(0, len(A.SEMS)))]
    zones = None
    if sem == sat_amd.SEM_EXACT_BASES or rng.integers(0, 3) == 0:    # exact zones on a third of the cases, always for exact_bases
        zones = []
        for p in allp:
            e, f_ = (int(rng.integers(0, 9)), 0) if rng.integers(0, 2) else (0, int(rng.integers(0, 9)))
            if rng.integers(0, 4) == 0:
                e, f_ = int(rng.integers(0, 7)), int(rng.integers(0, 7))
            if sem == sat_amd.SEM_EXACT_BASES and max(e, f_) < 6:
                e = 6 + int(rng.integers(0, 4))
            zones.append((min(e, len(p)), min(f_, len(p))))
    with_n = bool(rng.integers(0, 4) == 0)
    env = {}
    for name, val in A.KNOBS:
        v = val[int(rng.integers(0, len(val)))]
        if v is not None:
            env[name] = v
    cap = [1 << 10, 1 << 14, 1 << 20][int(rng.integers(0, 3))]
    mode = int(rng.integers(0, 4))
    raw = bool(rng.integers(0, 4) == 0)
    table = None if raw else (b"ACGT\nN" if with_n else A.TABLE)
    if with_n:
        s = s.copy()
        s[rng.integers(0, n, int(rng.integers(1, 40)))] = 5
    if not raw and rng.integers(0, 8) == 0:                           # the end-of-entry character first in the table (code 0)
        table = b"\nACGT" + (b"N" if with_n else b"")
        s = np.array([1, 2, 3, 4, 0, 5], dtype=np.uint8)[s]
    stream = np.frombuffer(b"ACGT\nN", dtype=np.uint8)[s].copy() if raw else s
    chunk = int(rng.integers(64, 3000))
    cut = int(rng.integers(n // 4, 3 * n // 4))
    host = bool(rng.integers(0, 3) == 0)
    if rng.integers(0, 4):                                            # all seven bits on three cases in four
        route = {b: True for b in BITS}
    else:                                                             # a random subset: a route beside another route's former path
        route = {b: bool(rng.integers(0, 2)) for b in BITS}
    lens = [len(p) for p in allp]
    return dict(seed=seed, style=style, n=n, k=k, indels=indels, lo=min(lens), hi=max(lens), patterns=allp, sem=sem, sname=sname, zones=zones,
                wild=wild, with_n=with_n, env=env, cap=cap, mode=mode, raw=raw, table=table, stream=stream, chunk=chunk, cut=cut, host=host,
                route=route, lens=lens)


def describe(c):
    return "class " + A.describe(c) + " bits " + "".join("1" if c["route"][b] else "0" for b in BITS)


# ---- the other doors into the library: windowed and packed streams, the device tally, the pairing stage ---------------------
# Shared by tests/test_gpu_adversarial_classes_streams.py, tests/test_gpu_adversarial_classes_stages.py (fixed seeds) and
# scripts/fuzz_families.py --oracle --classes --door ... (open-ended).  What is expected comes from the oracle's hits, the
# oracle's re-alignment (pmoracle.cli_align), tests/count_rule.py and tests/pcr_rule.py; nothing here asks the library.
AMPLICON_MAX = 600
PCR_DENSE = 3000                                                      # pairing cases with more oracle hits are left out (the Python rule stays fast)


def route_of(c):
    """the case's permission bits plus bit 7 (wild_long), which acts only where bit 5 is set"""
    return dict(c["route"], wild_long=True)


def engine(c):
    """a handle with the case's options, knobs, route, patterns and zones; no stream yet"""
    with A.knobs(c["env"]):
        pm = sat_amd.PatternMatch(k=c["k"], indels=c["indels"], kernel=sat_amd.KERNEL_AUTO, semantics=c["sem"], wildcards=c["wild"], **route_of(c))
    try:
        for i, p in enumerate(c["patterns"]):
            z = c["zones"][i] if c["zones"] else (0, 0)
            pm.add_pattern(p, i + 1, z[0], z[1])
    except BaseException:
        pm.close()
        raise
    return pm


def bits_for(table):
    return max(1, (len(table) - 1).bit_length())


def handle(c, window=None, packed=False):
    """the case's handle with its stream: resident as the case says (pm_init from host memory or pm_init_device), with
    `window` pm_init_windowed, with `packed` pm_init_packed (resident or windowed); the case's record capacity"""
    pm = engine(c)
    try:
        if packed:
            bits = bits_for(c["table"])
            pm.init_packed(sat_amd.pack_codes(c["stream"], bits), bits, c["n"], c["table"], window=window)
        elif window is not None or c["host"]:
            pm.init(c["stream"], c["table"], window=window)
        else:
            import torch
            dev = torch.from_numpy(c["stream"]).cuda()
            pm.init_device(dev.data_ptr(), c["n"], c["table"], keepalive=dev)
        pm.set_capacity(c["cap"])
    except BaseException:
        pm.close()
        raise
    return pm


def window_of(c):
    """(the window the windowed doors use, the ranges of find_all): the handle's minimum window plus 0 .. 4 times 64, and
    the case's chunk, bumped by one where it divides the window"""
    pm = engine(c)
    try:
        pm.init(c["stream"], c["table"], window=1)
        w0 = pm.residency()["window"]
    finally:
        pm.close()
    window = w0 + 64 * (c["seed"] % 5)
    return window, (c["chunk"] if c["chunk"] % window else c["chunk"] + 1)


def stream_hits(c, window=None, packed=False, chunk=1 << 26):
    """find_all on a windowed and / or packed handle: (sorted hits, residency figures, describe())"""
    pm = handle(c, window=window, packed=packed)
    try:
        got = sat_amd.sorted_tuples(pm.find_all(chunk=chunk))
        return got, pm.residency(), pm.describe()
    finally:
        pm.close()


def host_aligned(c, L):
    """whether the final hits of a primer of L characters are re-aligned by host threads on a resident handle with the case's
    route (csrc/pm_align.hip): never at k = 0; at k >= 1 beyond 64 characters, and from 33 characters on with
    indels where the long_align bit is clear (substitutions only take the one-diagonal branch up to 64 characters)"""
    return c["k"] >= 1 and (L > 64 or (c["indels"] and L > 32 and not c["route"]["long_align"]))


_ALIGNED = {}


def alignments(c, hits):
    """the oracle's re-alignment (start, end, editdist) of each of the case's oracle hits, computed once per seed"""
    if c["seed"] not in _ALIGNED:
        from oracle import pmoracle as O
        text = O.Text(c["stream"], c["table"])
        out = []
        for end, pid, _ in hits:
            z = c["zones"][pid - 1] if c["zones"] else (0, 0)
            out.append(tuple(O.cli_align(text, c["patterns"][pid - 1], end, c["k"], c["indels"], esb=z[0], eeb=z[1], wildcards=c["wild"])[1:4]))
        _ALIGNED[c["seed"]] = out
    return _ALIGNED[c["seed"]]


def count_expected(c, hits, M):
    """(counts, capped, info, re-aligned) of the case under max_count M from the oracle's hits alone; re-aligned: per
    pattern index, how many of its hits the rule re-aligns (tallied or bogus: not skipped behind the cap)"""
    import count_rule
    al = alignments(c, hits)
    asked = [0] * len(c["patterns"])

    def editdist(i):
        asked[hits[i][1] - 1] += 1
        return al[i][2]
    return count_rule.tally(hits, editdist, len(c["patterns"]), c["k"], M) + (asked,)


def count_walk(pm, c, ends, M):
    pm.reset()
    pos = 0
    for e in ends:
        e = min(int(e), c["n"])
        if e > pos:
            pm.count_scan(pos, e, M)
            pos = e
    return pm.counts()


def chars_of(c):
    """the stream as the characters the library decodes (bytes)"""
    if c["table"] is None:
        return c["stream"].tobytes()
    return np.frombuffer(bytes(c["table"]), dtype=np.uint8)[c["stream"]].tobytes()


def pcr_eligible(c):
    """the list has the form pm_pcr_setup requires: 2n patterns, n even, n+1 .. 2n the reverse complements of 1 .. n in order"""
    p = c["patterns"]
    n = len(p) // 2
    return len(p) % 4 == 0 and all(p[n + i] == sat_amd.reverse_comp(p[i]) for i in range(n))


def pcr_options(c):
    chars = chars_of(c)
    starts = [0] + [i + 1 for i, ch in enumerate(chars) if ch == 10]
    return dict(any_orientation=bool(c["seed"] & 1), length_between=bool(c["seed"] & 2), amplicon_max=AMPLICON_MAX, entry_starts=starts)


def pcr_round_ends(c):
    n = c["n"]
    return [e for e in sorted({n // 3, 2 * (n // 3), n}) if e > 0]


def pcr_expected(c, hits, delivered=None):
    """the three rounds from the oracle's hits, the oracle's re-alignment and tests/pcr_rule.py: a list of
    (scanned_to, more, hits held, survivors, candidate pairs, carried hits) -- a round sees the oracle's hits that end at or
    before scanned_to (the last round: all that are left) plus the hits carried from the round before.  delivered: the hits
    each round's range handed out, where that is not "the hits that end in it" (pcr_run)"""
    import pcr_rule as R
    o = pcr_options(c)
    rule = R.Rule(len(c["patterns"]) // 2, [0] + list(c["lens"]), c["k"], c["indels"], o["any_orientation"], o["length_between"], 0, AMPLICON_MAX, -1, None)
    al = dict(zip(hits, alignments(c, hits)))
    chars = chars_of(c)
    out, held, pos = [], [], 0
    for r, e in enumerate(pcr_round_ends(c)):
        more = e < c["n"]
        held = held + ([h for h in hits if pos < h[0] and (h[0] <= e or not more)] if delivered is None else list(delivered[r]))
        want, ncand, carried = R.round_survivors(rule, held, e, more, lambda h: al[h], o["entry_starts"], chars)
        out.append((e, more, held, want, ncand, carried))
        held, pos = carried, e
    return out


def survivor_of(r):
    """a record of pm_pcr_pair in the form of pcr_rule.round_survivors"""
    hit = lambda j: (int(r["hit"]["end"][j]), int(r["hit"]["pid"][j]), int(r["hit"]["k"][j]))
    al = lambda j: (int(r["al"]["start"][j]), int(r["al"]["end"][j]), int(r["al"]["editdist"][j]))
    return (hit(0), hit(1), al(0), al(1), int(r["amplicon_len"]), int(r["pair"]), int(r["ncount"]))


def pcr_run(c, hits, rounds=None):
    """pm_pcr_setup, then per round pm_pcr_scan and pm_pcr_pair with strings, against pcr_expected; asserts.  Returns figures
    of the run.

    Which round a hit joins.  A range hands out the hits that end in it, with two exceptions that are the reference's own:
    exact_halves / exact_bases extend a seed found inside the range to an end that may lie beyond it (adversarial.gpu_hits,
    `strict`; exact_halves.cc:153-167), so a hit may come a round EARLY; filter_bitvec chains candidates that lie within
    2k + 1 of each other and reports a chain when it can no longer grow (filter_bitvec.cc:103-121), so a hit whose chain
    reaches to within 2k + 1 of the scanned-to position comes a round LATE, however far before it the hit ends (at k = 0:
    a chain of consecutive ends, the last of them the scanned-to position itself); and exact_halves keeps a pattern's "last
    kept end" in seed order, so the library replays seeds only once no earlier one can still come (pm_api.cpp
    finalize_halves_flags: seeds within the longest pattern's length of the scanned-to position wait for the next range).  The
    rule is therefore applied per round to the hits pm_scan hands out for the same three ranges on the same handle -- all
    of them the oracle's, none missing at the end, early ones only from exact_halves / exact_bases, late ones only from these and filter_bitvec
    -- and every round is compared, whatever the engine.  All survivors and the candidate total over the three rounds also
    equal those of the rounds made from the oracle's hits alone (`rounds`), except where a chain of filter_bitvec came late
    (a pair whose window closed in between is the reference's to lose as well); where nothing comes early or late, the two
    forms are the same rounds."""
    rounds = rounds or pcr_expected(c, hits)
    what = describe(c)
    ends = pcr_round_ends(c)
    pm = handle(c)
    try:
        sel = pm.selected()[0]
        early_ok = sel in (sat_amd.SEM_EXACT_HALVES, sat_amd.SEM_EXACT_BASES)
        late_ok = early_ok or sel == sat_amd.SEM_FILTER_BITVEC
        pm.reset()
        delivered, pos = [], 0
        for e in ends:
            delivered.append(sat_amd.sorted_tuples(pm.scan_view(pos, e).copy()))
            pos = e
        assert sorted(h for d in delivered for h in d) == hits, (what, "pm_scan in the rounds' ranges")
        early = sum(1 for r, d in enumerate(delivered) for h in d if h[0] > ends[r] and r + 1 < len(ends))
        late = sum(1 for r, d in enumerate(delivered) for h in d if r > 0 and h[0] <= ends[r - 1])
        assert (early == 0 or early_ok) and (late == 0 or late_ok), (what, "selected", sel, "early", early, "late", late)
        mine = pcr_expected(c, hits, delivered) if early or late else rounds
        pm.pcr_setup(**pcr_options(c))
        pm.reset()
        no_host = not any(host_aligned(c, L) for L in c["lens"])
        got_all, cand_all, pos, strings = [], 0, 0, []
        for e, more, held, want, ncand, carried in mine:
            before, cbefore = pm.pcr_stats(), pm.counts()[2]
            assert pm.pcr_scan(pos, e) == len(held) - before_carried(mine, e), (what, "round to", e)
            rec, ops, txt = pm.pcr_pair(e, more, text=True)
            st, cafter = pm.pcr_stats(), pm.counts()[2]
            pos = e
            got = [survivor_of(r) for r in rec]
            assert not rec["hit"]["aux"].any(), what
            strings.append((e, rec, ops, txt))
            if no_host:                                               # no quiet way round the kernels
                assert st["aligned_host"] == before["aligned_host"] and cafter["aligned_host"] == cbefore["aligned_host"], (what, before, st)
            assert (st["held"], st["candidates"], st["survivors"]) == (len(held), ncand, len(want)), (what, "round to", e, st, len(held), ncand, len(want))
            assert got == want, (what, "round to", e, [x for x in got if x not in want][:3], [x for x in want if x not in got][:3])
            got_all += got
            cand_all += st["candidates"]
        assert mine[-1][5] == [] and rounds[-1][5] == [], what
        same = sorted(got_all) == sorted(s for r in rounds for s in r[3]) and cand_all == sum(r[4] for r in rounds)
        assert same or (late and sel == sat_amd.SEM_FILTER_BITVEC), (what, "all rounds", len(got_all), sum(len(r[3]) for r in rounds), cand_all, sum(r[4] for r in rounds))
        # the strings of a survivor are those of the host's pm_align_hits_text on the same two records
        for e, rec, ops, txt in strings:
            if rec.size:
                _, hops, htxt = pm.align_hits_text(np.ascontiguousarray(rec["hit"]).reshape(-1))
                assert ops == [(hops[2 * i], hops[2 * i + 1]) for i in range(rec.size)], (what, "alignment strings, round to", e)
                assert txt == [(htxt[2 * i], htxt[2 * i + 1]) for i in range(rec.size)], (what, "matching texts, round to", e)
        return dict(survivors=len(got_all), candidates=cand_all, carried=sum(1 for r in mine if r[5]), early=early, late=late, same=same,
                    aligned_device=st["aligned_device"], aligned_host=st["aligned_host"])
    finally:
        pm.close()


def before_carried(rounds, e):
    """how many of the hits a round holds were carried into it"""
    for i, r in enumerate(rounds):
        if r[0] == e:
            return len(rounds[i - 1][5]) if i else 0
    raise KeyError(e)


def edge_seeds(seeds):
    """the seeds whose case edge_case takes, all permission bits on"""
    out = []
    for s in seeds:
        c = class_case(s)
        if c["k"] >= 1 and not c["zones"] and not c["wild"] and all(c["route"].values()) and pcr_eligible(c):
            ch = chars_of(c)
            if set(ch[:40] + ch[-40:]) <= set(b"ACGT"):
                out.append(s)
    return out


def edge_case(seed):
    """class_case(seed) with two of its primers replaced by 40-mers that lie over the two ends of the stream: the first over
    the stream's first 40 - k characters, with k characters of its own in front of them (the k-error automaton starts with
    the first l bits of every pattern set in row l, shift_and_inexact.cc:162-164: a hit at end 40 - k that no whole window
    holds), the second over the last 40 - k characters with k more behind them (found, if at all, in the stream's last
    positions or beyond them); their reverse complements follow in the second half.  For a case with k >= 1, no zones, no -w
    and no end-of-entry character or N in the stream's first and last 40 characters.  These are the records the library's host
    makes for the stream's edges, as long as the longest main-class primer (pm_api.cpp edge_reach): the generator's own
    primers are cut from random places and hardly ever lie there."""
    c = class_case(seed)
    k, half = c["k"], len(c["patterns"]) // 2
    chars = chars_of(c).decode("latin1")
    assert k >= 1 and not c["zones"] and not c["wild"] and pcr_eligible(c) and set(chars[:40] + chars[-40:]) <= set("ACGT"), describe(c)
    other = {"A": "C", "C": "A", "G": "T", "T": "G"}
    first = "".join(other[ch] for ch in chars[40 - k:40])[:k] + chars[:40 - k]
    last = chars[-(40 - k):] + "".join(other[ch] for ch in chars[-40:-40 + k])
    pats = list(c["patterns"])
    pats[0], pats[1] = first, last
    pats[half], pats[half + 1] = sat_amd.reverse_comp(first), sat_amd.reverse_comp(last)
    c["patterns"], c["lens"] = pats, [len(p) for p in pats]
    c["lo"], c["hi"] = min(c["lens"]), max(c["lens"])
    c["seed"] = -seed                                                 # (a cache key of its own: alignments() goes by seed)
    return c
