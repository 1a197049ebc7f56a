"""GPU: the device tally at database size -- 100k 20-mers, both strands, 1 GiB ranges: pm_count_scan's tallies equal the
tally of find_all + align_hits (the host route), planted sites show up under their distance, and next to nothing leaves
the device: on uniform text the only records the host sees are clusters at range seams and in the first L characters
(DESIGN.md 2 and 5d)."""
import numpy as np
import pytest

import sat_amd
import test_gpu_fullsize as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k,indels,n", [(2, False, 1_000_000_000), (2, True, 1 << 28)])
def test_count_all_equals_the_host_tally(k, indels, n):
    L, P = 20, 100_000
    dev = F.make_db(n, 141 + int(indels))
    rng = np.random.default_rng(141 + int(indels))
    head = dev[: 1 << 24].cpu().numpy()
    if indels:
        plant = [(p, d) for d in range(3) for (p, _, _, d) in F.plant_edits(head, rng, 200, L, d)]
    else:
        plant = [(p, d) for d in range(3) for (p, _, d) in F.planted(head, rng, 200, L, d)]
    pats = [p for p, _ in plant] + F.random_primers(rng, P - len(plant), L)
    allp = pats + [sat_amd.reverse_comp(p) for p in pats]
    pm = F.engine(allp, k, sat_amd.KERNEL_AUTO, dev, indels=indels)
    try:
        pm.set_capacity(1 << 24 if not indels else 1 << 26)
        counts, capped, info = pm.count_all(chunk=1 << 30)
        print("count_all n %d k %d indels %d: %s" % (n, k, indels, info))
        hits = pm.find_all(chunk=1 << 30)                             # the host route: every hit crosses PCIe and is re-aligned on host threads
        al = pm.align_hits(hits)
        ok = al["editdist"] <= k
        want = np.zeros_like(counts)
        np.add.at(want, (hits["pid"][ok].astype(np.int64) - 1, al["editdist"][ok].astype(np.int64)), 1)
        assert (counts == want).all(), np.argwhere(counts != want)[:5]
        assert info["tallied"] == int(ok.sum()) and info["bogus"] == int((~ok).sum()) and info["skipped"] == 0 and not capped.any()
        assert info["tallied"] >= 600
        for i, (_, d) in enumerate(plant):                            # a site with d substitutions re-aligns to exactly d; with d edits to at most d
            assert (counts[i, d] >= 1) if not indels else (counts[i, :d + 1].sum() >= 1), ("planted site not tallied", i, d, counts[i])
        assert info["record_bytes_to_host"] * 100 <= 16 * info["tallied"], info
        assert info["aligned_host"] * 100 <= info["tallied"], info
    finally:
        pm.close()
