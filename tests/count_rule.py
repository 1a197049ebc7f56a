"""The tally of `primer_match -c [-M max]` (reference primer_match.cc:1123-1268), restated without the product: per
pattern id, its hits in order of stream end; a hit that comes after the id's total has reached M is skipped (and not
re-aligned); a hit that re-aligns to more than k is the caller's "Bogus hit": not tallied, not counted towards M; every
other hit adds one to count[id][editdist].  Shared by the GPU tests (expected values from the oracle) and
tests/test_counts_abi.py (the rule itself against the real primer_match's recorded output)."""


def tally(hits, editdist, npat, k, max_count=0):
    """hits: (end, id) pairs with ids 1 .. npat, any order; editdist(i) -> re-aligned distance of hits[i] (called only
    for hits that are not skipped).  Returns (counts[npat][k + 1], capped[npat], info)."""
    counts = [[0] * (k + 1) for _ in range(npat)]
    total = [0] * npat
    capped = [0] * npat
    info = dict(tallied=0, skipped=0, bogus=0, first_bogus=None)
    for i in sorted(range(len(hits)), key=lambda j: (hits[j][0], hits[j][1])):
        end, pid = hits[i][0], hits[i][1]
        if max_count > 0 and total[pid - 1] >= max_count:
            info["skipped"] += 1
            continue
        ed = editdist(i)
        if ed < 0 or ed > k:
            info["bogus"] += 1
            if info["first_bogus"] is None or (end, pid) < info["first_bogus"]:
                info["first_bogus"] = (end, pid)
            continue
        counts[pid - 1][ed] += 1
        total[pid - 1] += 1
        info["tallied"] += 1
        if max_count > 0 and total[pid - 1] >= max_count:
            capped[pid - 1] = 1
    return counts, capped, info
