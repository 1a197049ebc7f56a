#!/usr/bin/env python3
"""Measure a count pass (`primer_match -c`) two ways on one GPU and write profiles/count_pass.json:

  (A) pm_count_scan over the whole stream + pm_counts: the final hits are re-aligned and tallied in HBM;
  (B) the host route for the same tallies: pm_scan_view per range + pm_align_hits + the tally loop on the host
      (what pm_primer_match runs with PM_GPU_COUNTS=0).

Rows: -K 2 and -k 2 on a uniform synthetic stream (--n, default 3 Gbp), and -K 2 on skewed text (tests/adversarial.py
make_stream style 1 at database size, --skew-n, default 300 Mbp) with the primers cut from the stream -- the hit-dense
case.  100k 20-mers x 2 strands, resident stream, 1 GiB ranges; one warm-up pass per route, then --runs runs each, the two
routes alternating in one process; min - max of the wall time.  The tallies of (A) and (B) must be equal before a
time is reported.  Kernel times come from a separate run under rocprofv3 --kernel-trace --stats (--only a: route A
alone, one run)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sat_amd  # noqa: E402

TABLE = b"ACGT\n"
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_stream(n, seed, skew):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if not skew:
        t = torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda", generator=g)
    else:                                                            # A 0.55, C 0.05, G 0.05, T 0.35
        t = torch.empty(n, dtype=torch.uint8, device="cuda")
        step = 1 << 28
        for a in range(0, n, step):
            u = torch.rand(min(step, n - a), device="cuda", generator=g)
            t[a:a + u.numel()] = (u >= 0.55).to(torch.uint8) + (u >= 0.60).to(torch.uint8) + (u >= 0.65).to(torch.uint8)
    t[0] = 4
    t[-1] = 4
    t[n // 3] = 4
    return t


def primers(dev, rng, count, L, from_stream):
    if not from_stream:
        return [LUT[r].tobytes().decode() for r in rng.integers(0, 4, size=(count, L), dtype=np.uint8)]
    host = dev[: 1 << 26].cpu().numpy()
    out = []
    while len(out) < count:
        a = int(rng.integers(1, host.size - L - 1))
        w = host[a:a + L]
        if not (w > 3).any():
            out.append(LUT[w].tobytes().decode())
    return out


def route_a(pm, n, chunk):
    t0 = time.perf_counter()
    counts, capped, info = pm.count_all(chunk=chunk)
    return time.perf_counter() - t0, counts, info


def route_b(pm, n, chunk, k):
    t0 = time.perf_counter()
    pm.reset()
    counts = np.zeros((pm._npat, k + 1), dtype=np.uint64)
    pos = hits_seen = 0
    while pos < n:
        end = min(n, pos + chunk)
        hits = pm.scan_view(pos, end)
        if hits.size:
            al = pm.align_hits(hits)
            ok = al["editdist"] <= k
            np.add.at(counts, (hits["pid"][ok].astype(np.int64) - 1, al["editdist"][ok].astype(np.int64)), 1)
            hits_seen += int(hits.size)
        pos = end
    return time.perf_counter() - t0, counts, hits_seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000_000)
    ap.add_argument("--skew-n", type=int, default=300_000_000)
    ap.add_argument("--npat", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 30)
    ap.add_argument("--only", choices=["a", "both"], default="both")
    ap.add_argument("--rows", default="K2,k2,K2skew")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "count_pass.json"))
    args = ap.parse_args()
    rows = []
    for name in args.rows.split(","):
        k, indels, skew = 2, name.startswith("k"), name.endswith("skew")
        n = args.skew_n if skew else args.n
        dev = make_stream(n, 7 + int(skew), skew)
        rng = np.random.default_rng(17)
        pats = primers(dev, rng, args.npat, 20, skew)
        allp = pats + [sat_amd.reverse_comp(p) for p in pats]
        pm = sat_amd.PatternMatch(k=k, indels=indels)
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init_device(dev.data_ptr(), n, TABLE, keepalive=dev)
        ta, tb = [], []
        _, ca, info = route_a(pm, n, args.chunk)                     # warm-up passes (buffers grow to their size, tables are built)
        row = {"row": name, "n": n, "patterns": len(allp), "k": k, "indels": indels, "kernel": pm.describe(), "info": info}
        if args.only == "both":
            _, cb, nhits = route_b(pm, n, args.chunk, k)
            assert (ca == cb).all(), "tallies of the two routes differ"
            row["hits"] = nhits
        for _ in range(args.runs):
            t, c, _ = route_a(pm, n, args.chunk)
            assert (c == ca).all()
            ta.append(t)
            if args.only == "both":
                t, c, _ = route_b(pm, n, args.chunk, k)
                assert (c == ca).all()
                tb.append(t)
        row["count_scan_s"] = [min(ta), max(ta)]
        if tb:
            row["host_route_s"] = [min(tb), max(tb)]
            row["faster_by_more_than_spread"] = max(ta) < min(tb) and (min(tb) - max(ta)) > (max(tb) - min(tb))
        print(json.dumps(row), flush=True)
        rows.append(row)
        pm.close()
        del dev
        torch.cuda.empty_cache()
    if args.only == "both":
        with open(args.out, "w") as f:
            json.dump({"rows": rows, "runs": args.runs, "chunk": args.chunk}, f, indent=1)


if __name__ == "__main__":
    main()
