#!/usr/bin/env python3
"""Measure what primers of 16..19 nt cost a -k 2 pass and write profiles/short_class.json.

Workload: the bench's synthetic stream (--n, default 3 Gbp, uniform A,C,G,T), 100k random 20-mers on both strands, plus S
18-mers cut from the stream (a third of them with one, a third with two edits) on both strands, S in --s (default
0,10,1000,20000).  Timed: the end-to-end pass -- pm_scan_view over 1 GiB ranges, final hits landed on the host -- after
one warm-up pass, --runs runs (min - max of the wall time).  Beside it: the device time of the scan stage of the last
pass (pm_last_kernel_time summed over the ranges), the records between the two stages of the scan (pm_scan_stats), and
the hit count and a checksum of the final hits.

The same script runs on the commit before pm_short_edit_scan (PM_GPU_LIB=<that build's libpm_gpu.so>): there the 18-mers
are "patterns the seed plan does not take" and go to the bit-parallel residue kernel.  --merge joins two such outputs
into the table of DESIGN.md 4.7 and checks that hit count and checksum agree at every S.  Kernel times of their own come
from a run under rocprofv3 --kernel-trace --stats (--s 20000 --runs 0).

--indels 0 is the same measurement for -K 2 and pm_short_sub_scan: the 18-mers carry substitutions only (a
third exact, a third with one, a third with two), the output goes to profiles/short_sub_class.json, and on the commit
before (or with PM_SHORT_SUB=off) one 18-mer sends the whole list from the pair plan to the Bloom plan.  For interleaved
runs of the two builds each side of --merge takes several outputs, comma separated: their passes are pooled per S."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sat_amd  # noqa: E402
import synth  # noqa: E402

TABLE = b"ACGT\n"
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_stream(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda", generator=g)
    t[0] = 4
    t[-1] = 4
    t[n // 3] = 4
    return t


def short_primers(dev, rng, count, L, indels=True):
    host = dev[: 1 << 26].cpu().numpy()
    out = []
    while len(out) < count:
        a = int(rng.integers(1, host.size - L - 3))
        w = LUT[host[a:a + L + 2] & 3].tobytes().decode()
        kind = len(out) % 3
        if not indels:
            w = synth.mutate(rng, w[:L], nsub=kind)
        elif kind == 0:
            w = w[:L]
        elif kind == 1:
            w = synth.mutate(rng, w[:L], nsub=int(rng.integers(0, 2)), nins=0, ndel=0) if rng.random() < 0.5 else synth.mutate(rng, w[:L + 1], ndel=1)
        else:
            w = synth.mutate(rng, w[:L], nsub=2) if rng.random() < 0.5 else synth.mutate(rng, w[:L], nsub=1, nins=1, ndel=1)
        if len(w) == L:
            out.append(w)
    return out


def one_pass(pm, n, chunk):
    t0 = time.perf_counter()
    pm.reset()
    pos = nhits = 0
    check = 0
    dev_ms = 0.0
    between = 0
    while pos < n:
        end = min(n, pos + chunk)
        hits = pm.scan_view(pos, end)
        nhits += int(hits.size)
        if hits.size:
            check ^= int(np.bitwise_xor.reduce((hits["end"].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ (hits["pid"].astype(np.uint64) << np.uint64(8)) ^ hits["k"].astype(np.uint64)))
        dev_ms += pm.last_kernel_time()[0]
        between += pm.scan_stats()["between_stages"]
        pos = end
    return time.perf_counter() - t0, nhits, check, dev_ms, between


def pooled(paths):
    """outputs of several runs of one build: per S, the passes of all of them"""
    docs = [json.load(open(p)) for p in paths.split(",")]
    for d in docs[1:]:
        for r0, r in zip(docs[0]["rows"], d["rows"]):
            assert (r0["S"], r0["hits"], r0["checksum"]) == (r["S"], r["hits"], r["checksum"]), (r0, r)
            if r0["pass_s"] and r["pass_s"]:
                r0["pass_s"] = [min(r0["pass_s"][0], r["pass_s"][0]), max(r0["pass_s"][1], r["pass_s"][1])]
    docs[0]["runs"] = sum(d["runs"] for d in docs)
    return docs[0]


def merge(paths, out):
    a, b = (pooled(p) for p in paths)
    rows = []
    for ra in a["rows"]:
        rb = next((r for r in b["rows"] if r["S"] == ra["S"]), None)
        if rb is None:
            continue
        assert (ra["hits"], ra["checksum"]) == (rb["hits"], rb["checksum"]), ("hit count or checksum differ at S = %d" % ra["S"], ra, rb)
        ta, tb = ra["pass_s"] or [ra["warm_s"]] * 2, rb["pass_s"] or [rb["warm_s"]] * 2      # (--runs 0: the one pass there is)
        rows.append({"S": ra["S"], "hits": ra["hits"], "checksum": ra["checksum"], "parent": rb, "this": ra,
                     "faster_by_more_than_parent_spread": bool(max(ta) < min(tb) and min(tb) - max(ta) > max(tb) - min(tb))})
    with open(out, "w") as f:
        json.dump({"rows": rows, "n": a["n"], "runs": a["runs"]}, f, indent=1)
    for r in rows:
        print(r["S"], r["hits"], "this", r["this"]["pass_s"] or r["this"]["warm_s"], "parent", r["parent"]["pass_s"] or r["parent"]["warm_s"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000_000)
    ap.add_argument("--npat", type=int, default=100_000)
    ap.add_argument("--s", default="0,10,1000,20000")
    ap.add_argument("--length", type=int, default=18)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 30)
    ap.add_argument("--indels", type=int, default=1, help="1: -k 2 (pm_short_edit_scan), 0: -K 2 (pm_short_sub_scan)")
    ap.add_argument("--out", default=None, help="default: profiles/short_class.json, with --indels 0 profiles/short_sub_class.json")
    ap.add_argument("--merge", nargs=2, metavar=("THIS", "PARENT"), help="join two outputs of this script into --out")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "short_class.json" if args.indels else "short_sub_class.json")
    if args.merge:
        return merge(args.merge, args.out)
    dev = make_stream(args.n, 7)
    rng = np.random.default_rng(17)
    longs = [LUT[r].tobytes().decode() for r in rng.integers(0, 4, size=(args.npat, 20), dtype=np.uint8)]
    rows = []
    for S in (int(x) for x in args.s.split(",")):
        shorts = short_primers(dev, np.random.default_rng(100 + S), S, args.length, bool(args.indels))
        pats = longs + shorts
        allp = pats + [sat_amd.reverse_comp(p) for p in pats]
        pm = sat_amd.PatternMatch(k=2, indels=bool(args.indels))
        for i, p in enumerate(allp):
            pm.add_pattern(p, i + 1)
        pm.init_device(dev.data_ptr(), args.n, TABLE, keepalive=dev)
        warm, nhits, check, dev_ms, between = one_pass(pm, args.n, args.chunk)     # warm-up pass: buffers grow to their size
        row = {"S": S, "n": args.n, "patterns": len(allp), "kernel": pm.describe(), "hits": nhits, "checksum": check, "warm_s": warm}
        ts = []
        for _ in range(args.runs):
            t, h, c, dev_ms, between = one_pass(pm, args.n, args.chunk)
            assert (h, c) == (nhits, check)
            ts.append(t)
        row.update(pass_s=[min(ts), max(ts)] if ts else None, scan_device_ms=dev_ms, between_stages=between, between_per_base=between / args.n)
        print(json.dumps(row), flush=True)
        rows.append(row)
        pm.close()
    with open(args.out, "w") as f:
        json.dump({"rows": rows, "n": args.n, "runs": args.runs, "chunk": args.chunk}, f, indent=1)


if __name__ == "__main__":
    main()
