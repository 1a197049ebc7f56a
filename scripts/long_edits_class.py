#!/usr/bin/env python3
"""Measure what primers of 33..64 nt cost a -k 2 pass on the two routes and write profiles/long_edits_class.json.

Workload: the bench's synthetic stream (--n, default 3 Gbp, uniform A,C,G,T), 100k random 20-mers on both strands, plus S
40-mers cut from the stream on both strands (a third exact, a third with one edit, a third with two), S in --s (default
0,10,1000), and -- S = "alone" -- a list of 100k such 40-mers with no 20-mer beside them; -k 2: filter_bitvec.  Every list
runs on two handles of one process: the long route (bit 2 of pm_config.long_patterns: the 40-mers on the edit plan's wide
tiles, pm_edits_verify_wide and pm_cluster_dp<64>) and the former route (PM_LONG_EDITS=off while the
handle is created: the 40-mers on the bit-parallel residue kernel).  Timed: the end-to-end pass -- pm_scan_view over 1 GiB
ranges, final hits landed on the host -- after one warm-up pass per handle, --runs runs per handle, the two handles taking
turns (min - max of the wall time).  Beside it: the device time of the scan stage of the last pass, the seed records
handed to the automaton, and the hit count and a checksum of the final hits, which must be equal on the two routes.

The former route costs minutes per pass for the list of 40-mers alone (pm_bitpar_scan<2,true> at 2 x 10^5 patterns):
--off-runs-alone limits the timed passes of that one handle (0, the default: its warm-up pass is its figure).

The same script runs on the commit before the route (PM_GPU_LIB=<that build's libpm_gpu.so>, --parent): one handle per
list, built without the bit; --merge joins the two outputs and checks hit counts and checksums."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import sat_amd  # noqa: E402
from short_class import LUT, TABLE, make_stream, one_pass, short_primers  # noqa: E402


def handle(allp, dev, n, route):
    """route: "long" (the permission given), "off" (given, and PM_LONG_EDITS=off in the environment pm_create reads),
    "parent" (a build without the bit)"""
    if route == "off":
        os.environ["PM_LONG_EDITS"] = "off"
    try:
        pm = sat_amd.PatternMatch(k=2, long_edits=True) if route != "parent" else sat_amd.PatternMatch(k=2)
    finally:
        os.environ.pop("PM_LONG_EDITS", None)
    for i, p in enumerate(allp):
        pm.add_pattern(p, i + 1)
    pm.init_device(dev.data_ptr(), n, TABLE, keepalive=dev)
    return pm


def merge(paths, out):
    a, b = (json.load(open(p)) for p in paths)
    for ra in a["rows"]:
        rb = next((r for r in b["rows"] if r["S"] == ra["S"]), None)
        if rb is None:
            continue
        assert (ra["hits"], ra["checksum"]) == (rb["hits"], rb["checksum"]), ("hit count or checksum differ at S = %s" % ra["S"], ra, rb)
        ra["routes"]["parent"] = rb["routes"]["parent"]
    with open(out, "w") as f:
        json.dump(a, f, indent=1)
    for r in a["rows"]:
        print(r["S"], r["hits"], {k: v["pass_s"] or v["warm_s"] for k, v in r["routes"].items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000_000)
    ap.add_argument("--npat", type=int, default=100_000)
    ap.add_argument("--s", default="0,10,1000,alone")
    ap.add_argument("--length", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--off-runs-alone", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=1 << 30)
    ap.add_argument("--routes", default="long,off", help="the handles of a list (a run on a shorter stream can time the former route of the 40-mer-only list)")
    ap.add_argument("--parent", action="store_true", help="a build without the bit: one handle per list")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_edits_class.json"))
    ap.add_argument("--merge", nargs=2, metavar=("THIS", "PARENT"), help="join two outputs of this script into --out")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    dev = make_stream(args.n, 7)
    rng = np.random.default_rng(17)
    twenty = [LUT[r].tobytes().decode() for r in rng.integers(0, 4, size=(args.npat, 20), dtype=np.uint8)]
    rows = []
    for S in args.s.split(","):
        alone = S == "alone"
        longs = short_primers(dev, np.random.default_rng(500 + (0 if alone else int(S))), args.npat if alone else int(S), args.length)
        pats = longs if alone else twenty + longs
        allp = pats + [sat_amd.reverse_comp(p) for p in pats]
        routes = ["parent"] if args.parent else args.routes.split(",")
        pms = {r: handle(allp, dev, args.n, r) for r in routes}
        row = {"S": S, "n": args.n, "patterns": len(allp), "routes": {}}
        times = {r: [] for r in routes}
        last = {}
        for r in routes:                                             # warm-up pass: buffers grow to their size
            print("S = %s, route %s: warm-up pass" % (S, r), flush=True)
            warm, nhits, check, dev_ms, between = one_pass(pms[r], args.n, args.chunk)
            row["routes"][r] = {"kernel": pms[r].describe(), "warm_s": warm}
            assert (row.setdefault("hits", nhits), row.setdefault("checksum", check)) == (nhits, check), (S, r, nhits, check, row)
            last[r] = (dev_ms, between)
        for i in range(args.runs):                                   # the routes take turns
            for r in routes:
                if alone and r == "off" and i >= args.off_runs_alone:
                    continue
                t, h, c, dev_ms, between = one_pass(pms[r], args.n, args.chunk)
                assert (h, c) == (row["hits"], row["checksum"]), (S, r)
                times[r].append(t)
                last[r] = (dev_ms, between)
        for r in routes:
            row["routes"][r].update(pass_s=[min(times[r]), max(times[r])] if times[r] else None, runs=len(times[r]),
                                    scan_device_ms=last[r][0], seed_records=last[r][1])
            pms[r].close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(args.out, "w") as f:
        json.dump({"rows": rows, "n": args.n, "runs": args.runs, "chunk": args.chunk}, f, indent=1)


if __name__ == "__main__":
    main()
