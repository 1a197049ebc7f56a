#!/usr/bin/env python3
"""Measure what the device re-alignment of 33..64 nt primers (bit 4 of pm_config.long_patterns, PM_LONG_ALIGN: DESIGN.md 5d)
changes in a -k 2 count pass and write profiles/long_align.json.

Workload: the bench's synthetic stream (--n, default 3 Gbp, uniform A,C,G,T), 100k random 20-mers on both strands, plus S
40-mers cut from the stream on both strands (a third exact, a third with one edit, a third with two), S in --s (default
0,10,1000), and -- S = "alone" -- a list of 100k such 40-mers with no 20-mer beside them; -k 2: filter_bitvec.  Every list
runs on two handles of one process, both on the edit plan's long route (bit 2): long_patterns = 4 -- the hits of the 40-mers
are compacted, copied to the host and aligned by its threads -- and 4 | 16 -- pm_align_hits_wide_kernel aligns them where
they are.  Timed: the count pass, pm_count_scan over 1 GiB ranges + pm_counts, after one warm-up pass per handle, --runs
runs per handle, the two handles taking turns (min - max of the wall time).  The tallies of the two handles must be equal
before a time is reported.  Each line records aligned_host, aligned_device and record_bytes_to_host of either handle; the
S = 0 line is the list without long primers, whose two times must not differ by more than the spread of the bit-clear
handle's runs (both figures are recorded: "spread_clear_s", "difference_s")."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import sat_amd  # noqa: E402
from short_class import LUT, TABLE, make_stream, short_primers  # noqa: E402

ROUTES = {"clear": False, "align": True}                             # long_patterns = 4 and 4 | 16


def handle(allp, dev, n, long_align):
    pm = sat_amd.PatternMatch(k=2, long_edits=True, long_align=long_align)
    for i, p in enumerate(allp):
        pm.add_pattern(p, i + 1)
    pm.init_device(dev.data_ptr(), n, TABLE, keepalive=dev)
    return pm


def count_pass(pm, chunk):
    t0 = time.perf_counter()
    counts, capped, info = pm.count_all(chunk=chunk)
    return time.perf_counter() - t0, counts, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000_000)
    ap.add_argument("--npat", type=int, default=100_000)
    ap.add_argument("--s", default="0,10,1000,alone")
    ap.add_argument("--length", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_align.json"))
    args = ap.parse_args()
    dev = make_stream(args.n, 7)
    rng = np.random.default_rng(17)
    twenty = [LUT[r].tobytes().decode() for r in rng.integers(0, 4, size=(args.npat, 20), dtype=np.uint8)]
    rows = []
    for S in args.s.split(","):
        alone = S == "alone"
        longs = short_primers(dev, np.random.default_rng(500 + (0 if alone else int(S))), args.npat if alone else int(S), args.length)
        pats = longs if alone else twenty + longs
        allp = pats + [sat_amd.reverse_comp(p) for p in pats]
        pms = {r: handle(allp, dev, args.n, bit) for r, bit in ROUTES.items()}
        row = {"S": S, "n": args.n, "patterns": len(allp), "routes": {}}
        times = {r: [] for r in ROUTES}
        ref = None
        for r in ROUTES:                                             # warm-up pass: buffers grow to their size, tables are built
            warm, counts, info = count_pass(pms[r], args.chunk)
            row["routes"][r] = {"kernel": pms[r].describe(), "warm_s": warm}
            if ref is None:
                ref = counts
            assert (counts == ref).all(), "tallies of the two handles differ at S = %s" % S
        row["tallied"] = int(ref.sum())
        for _ in range(args.runs):                                   # the handles take turns
            for r in ROUTES:
                t, counts, info = count_pass(pms[r], args.chunk)
                assert (counts == ref).all(), (S, r)
                times[r].append(t)
                row["routes"][r].update({f: info[f] for f in ("aligned_host", "aligned_device", "record_bytes_to_host", "tallied", "bogus")})
        for r in ROUTES:
            row["routes"][r]["pass_s"] = [min(times[r]), max(times[r])]
            pms[r].close()
        row["spread_clear_s"] = max(times["clear"]) - min(times["clear"])
        row["difference_s"] = min(times["align"]) - min(times["clear"])
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(args.out, "w") as f:
        json.dump({"rows": rows, "n": args.n, "runs": args.runs, "chunk": args.chunk}, f, indent=1)


if __name__ == "__main__":
    main()
