"""Plain-Python restatement of one round of pcr_match's pairing stage (reference pcr_match.cc:948-1259), the oracle of
the pm_pcr_* tests.  Arbitrary-precision ints; where the reference wraps (unsigned 64-bit comparisons of the UniSTS clamp,
the (unsigned long) and (int) casts of the deviation test) the masks are explicit.

Two forms of the join: `candidates` is the closed form (what one pair of hits decides), `candidates_loop` walks the hits
and zeroes keys the way the reference does.  tests/test_pcr_rule.py holds them against each other and against the
reference's recorded output.

A hit is a tuple (key, id, k): key = stream index behind the last matched character.  An alignment is (start, end, editdist)."""
M64 = (1 << 64) - 1


def s64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


class Rule:
    """n primers (ids 1..n as given: 2j-1 forward, 2j reverse; n+1..2n their reverse complements), patlen[id] for id in
    1..2n (index 0 unused), sizes = [(sizelb, sizeub)] per primer pair or None (no UniSTS file)."""

    def __init__(self, n, patlen, k, indels=True, any_orientation=False, length_between=False, amplicon_min=0, amplicon_max=2000,
                 size_slack=-1, sizes=None):
        self.n, self.patlen, self.k, self.indels = n, list(patlen), k, indels
        self.any_orientation, self.length_between = any_orientation, length_between
        self.amplicon_min, self.amplicon_max, self.size_slack, self.sizes = amplicon_min, amplicon_max, size_slack, sizes
        self.slack = k if indels else 1


def partners(r, pid):
    n = r.n
    pid1 = pid2 = 0
    if pid <= n and pid % 2 == 1:
        pid1 = pid + 1
    elif pid > n and (pid - n) % 2 == 0:
        pid1 = pid - 1
    if r.any_orientation:
        if pid <= n:
            if pid % 2 == 1:
                pid2 = pid + n + 1
            else:
                pid1, pid2 = pid - 1, pid + n - 1
        else:
            if pid % 2 == 0:
                pid2 = pid - n - 1
            else:
                pid1, pid2 = pid + 1, pid - n + 1
    return pid1, pid2


def pair_of(r, pid):
    return (pid - (r.n if pid > r.n else 0) + 1) // 2


def stretch(r, pid, pos):
    """(stretch_min, stretch_max) of a hit of pattern pid at pos (pcr_match.cc:1031-1052)"""
    pid1, pid2 = partners(r, pid)
    smax, smin = r.amplicon_max, r.amplicon_min
    if r.length_between:
        plen = r.patlen[pid1] if pid1 else 0
        if pid2 and r.patlen[pid2] > plen:
            plen = r.patlen[pid2]
        smax += plen + r.patlen[pid]
    if r.sizes is not None and r.size_slack >= 0:
        lb_, ub_ = r.sizes[pair_of(r, pid) - 1]
        ub = (ub_ + r.size_slack) & M64
        lb = (lb_ - r.size_slack) & M64
        if (smax & M64) > ub:
            smax = s64(ub)
        if (smin & M64) < lb:
            smin = s64(lb)
    return s64(smin + pos - r.patlen[pid] - r.slack), s64(smax + pos - r.patlen[pid] + r.slack)


def is_deferred(r, hit, scanned_to, more):
    return bool(more) and scanned_to < stretch(r, hit[1], hit[0])[1]


def candidates(r, hits, scanned_to, more):
    """Closed form.  Returns (held hits in (key, id, k) order, candidate pairs as (i, j) indices into them, carried hits)."""
    l = sorted(hits)
    dfr = [is_deferred(r, h, scanned_to, more) for h in l]
    by_id = {}
    for j, h in enumerate(l):
        by_id.setdefault(h[1], []).append(j)
    pairs = []
    for i, h in enumerate(l):
        if dfr[i]:
            continue
        smin, smax = stretch(r, h[1], h[0])
        for p in partners(r, h[1]):
            if p == 0:
                continue
            for j in by_id.get(p, ()):                  # (key order inside an id)
                if smin <= l[j][0] <= smax and (j > i or dfr[j]):
                    pairs.append((i, j))
    return l, pairs, [h for j, h in enumerate(l) if dfr[j]]


def candidates_loop(r, hits, scanned_to, more):
    """The reference's walk: every processed hit's key is zeroed (pcr_match.cc:1221); same return value."""
    l = sorted(hits)
    live = [h[0] for h in l]
    by_id = {}
    for j, h in enumerate(l):
        by_id.setdefault(h[1], []).append(j)
    pairs = []
    for i, h in enumerate(l):
        smin, smax = stretch(r, h[1], h[0])
        if scanned_to < smax and more:
            continue
        for p in partners(r, h[1]):
            if p == 0:
                continue
            pq = by_id.get(p, [])
            q = 0
            while q < len(pq) and l[pq[q]][0] < smin:
                q += 1
            while q < len(pq) and live[pq[q]] <= smax:
                if live[pq[q]]:
                    pairs.append((i, pq[q]))
                q += 1
        live[i] = 0
    return l, pairs, [h for j, h in enumerate(l) if live[j] != 0]


def locate(entry_starts, pos):
    """SeqDb::locate: index of the last entry that starts at or before pos - 1 (-1: none)"""
    import bisect
    return bisect.bisect_right(entry_starts, pos - 1) - 1


def pind(r, pid, pid1):
    ind, ind1 = pid - (r.n if pid > r.n else 0), pid1 - (r.n if pid1 > r.n else 0)
    return ind // 2 + 1 if ind < ind1 else ind1 // 2 + 1


def survives(r, al, al1, pid, pid1, entry_starts):
    """The filter of pcr_match.cc:1116-1160.  Returns (passes, amplicon_len, pind)."""
    ps, pe, ed = al
    ps1, pe1, ed1 = al1
    alen = pe1 - ps if not r.length_between else ps1 - pe
    pi = pind(r, pid, pid1)
    ok = 0 <= ed <= r.k and 0 <= ed1 <= r.k
    a, b = locate(entry_starts, ps + 1), locate(entry_starts, pe1)
    ok = ok and a >= 0 and b >= 0 and a == b
    ok = ok and r.amplicon_min <= alen <= r.amplicon_max
    if ok and r.sizes is not None and r.size_slack >= 0:
        lb, ub = r.sizes[pi - 1]
        ok = ((alen + r.size_slack) & M64) >= lb and alen <= s32(ub) + r.size_slack
    return ok, alen, pi


def ncount(chars, start, alen):
    """N and n among the characters (bytes of the decoded stream) at start .. start + alen - 1, positions outside the
    stream counting nothing.  The reference starts at ps with -b too."""
    lo, hi = max(start, 0), min(start + alen, len(chars))
    return sum(1 for c in chars[lo:hi] if c in b"Nn") if hi > lo else 0


def round_survivors(r, hits, scanned_to, more, align, entry_starts, chars):
    """One round: (survivors, candidate pair count, carried hits); a survivor is
    (hit, partner, alignment, partner's alignment, amplicon_len, pind, ncount).  align(hit) -> (start, end, editdist)."""
    l, pairs, carried = candidates(r, hits, scanned_to, more)
    cache = {}
    def al(j):
        if j not in cache:
            cache[j] = tuple(align(l[j]))
        return cache[j]
    out = []
    for i, j in pairs:
        ok, alen, pi = survives(r, al(i), al(j), l[i][1], l[j][1], entry_starts)
        if ok:
            out.append((l[i], l[j], al(i), al(j), alen, pi, ncount(chars, al(i)[0], alen)))
    return out, len(pairs), carried
