#!/usr/bin/env python3
"""Measure what long degenerate primers (-w, 33..64 nt, three or more ambiguity letters) cost a pass on the two routes and
write profiles/wild_long_class.json.

Workload: the bench's synthetic stream (--n, default 3 Gbp, uniform A,C,G,T), 100k random 20-mers on both strands, plus S
52-mers cut from the stream, each with four ambiguity letters in its last 20 characters (two two-fold, one three-fold, one
N: 48 concrete variants), on both strands, S in --s (default 0,10,1000), and -- S = "alone" -- the list of 1000 such
52-mers with no 20-mer beside them.  Option sets: -K 2 (filter_bitvec) and k = 0 (shift_and), both with -w.  Every list
and option set runs on two handles of one process: the class route (bits 5 and 7 of pm_config.long_patterns: the 52-mers
on pm_wild_sub_scan + pm_wild_sub_verify_wide) and the former route (the same bits, and PM_WILD_LONG=off
while the handle is created: the 52-mers on the bit-parallel residue kernel).  Timed: the end-to-end pass -- pm_scan_view
over 1 GiB ranges, final hits landed on the host -- after one warm-up pass per handle, --runs runs per handle, the two
handles taking turns (min - max of the wall time).  Beside it: the device time of the scan stage of the last pass, and the
hit count and a checksum of the final hits, which must be equal on the two routes.  The S = 0 pair is the same handle
twice: its two figures give the run-to-run spread.

--append adds the rows to an existing file and does not replace it: the S = 0 pass against another build of the library
(PM_GPU_LIB=<csrc>/libpm_gpu_parent.so PM_GPU_LIB_AB=1 ... --s 0 --append) is recorded that way, under "library"."""
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
import synth  # noqa: E402
from short_class import LUT, TABLE, make_stream, one_pass  # noqa: E402
from wild_class import OPTS, THREE, TWO  # noqa: E402


def degenerate_windows(dev, rng, count, L):
    """windows of the stream's first 2^26 bases with four ambiguity letters in their last 20 characters that hold the
    window's own bases"""
    host = dev[: 1 << 26].cpu().numpy()
    out = []
    while len(out) < count:
        a = int(rng.integers(1, host.size - L - 3))
        w = list(LUT[host[a:a + L] & 3].tobytes().decode())
        i, j, m, q = (L - 20 + rng.choice(20, size=4, replace=False)).tolist()
        w[i], w[j] = str(rng.choice(list(TWO[w[i]]))), str(rng.choice(list(TWO[w[j]])))
        w[m], w[q] = str(rng.choice(list(THREE[w[m]]))), "N"
        out.append("".join(w))
    return out


def handle(allp, dev, n, opt, route, library):
    """route: "class" (both permissions given), "off" (given, and PM_WILD_LONG=off in the environment pm_create reads).
    A library from before the bit existed takes the value without it: both of its handles are the former route."""
    if route == "off":
        os.environ["PM_WILD_LONG"] = "off"
    try:
        if library == "product":
            pm = sat_amd.PatternMatch(wildcards=True, wild_class=True, wild_long=True, **OPTS[opt])
        else:
            pm = sat_amd.PatternMatch(wildcards=True, wild_class=True, **OPTS[opt])
    finally:
        os.environ.pop("PM_WILD_LONG", None)
    for i, p in enumerate(allp):
        pm.add_pattern(p, i + 1)
    pm.init_device(dev.data_ptr(), n, TABLE, keepalive=dev)
    return pm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000_000)
    ap.add_argument("--npat", type=int, default=100_000)
    ap.add_argument("--s", default="0,10,1000,alone")
    ap.add_argument("--opts", default="K2,k0")
    ap.add_argument("--length", type=int, default=52)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--chunk", type=int, default=1 << 30)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wild_long_class.json"))
    args = ap.parse_args()
    library = os.path.basename(os.environ["PM_GPU_LIB"]) if os.environ.get("PM_GPU_LIB_AB") == "1" and os.environ.get("PM_GPU_LIB") else "product"
    rows = []
    if args.append and os.path.exists(args.out):
        with open(args.out) as f:
            rows = json.load(f)["rows"]
    dev = make_stream(args.n, 7)
    rng = np.random.default_rng(17)
    twenty = [LUT[r].tobytes().decode() for r in rng.integers(0, 4, size=(args.npat, 20), dtype=np.uint8)]
    for opt in args.opts.split(","):
        for S in args.s.split(","):
            alone = S == "alone"
            wild = degenerate_windows(dev, np.random.default_rng(500 + (1000 if alone else int(S))), 1000 if alone else int(S), args.length)
            pats = wild if alone else twenty + wild
            allp = pats + [synth.revcomp_iupac(p) for p in pats]
            routes = ["class", "off"]
            pms = {r: handle(allp, dev, args.n, opt, r, library) for r in routes}
            row = {"opt": opt, "S": S, "n": args.n, "patterns": len(allp), "library": library, "routes": {}}
            times = {r: [] for r in routes}
            last = {}
            for r in routes:                                         # warm-up pass: buffers grow to their size
                warm, nhits, check, dev_ms, between = one_pass(pms[r], args.n, args.chunk)
                row["routes"][r] = {"kernel": pms[r].describe(), "warm_s": warm}
                assert (row.setdefault("hits", nhits), row.setdefault("checksum", check)) == (nhits, check), (opt, S, r, nhits, check, row)
                last[r] = (dev_ms, between)
            for i in range(args.runs):                               # the routes take turns
                for r in routes:
                    t, h, c, dev_ms, between = one_pass(pms[r], args.n, args.chunk)
                    assert (h, c) == (row["hits"], row["checksum"]), (opt, S, r)
                    times[r].append(t)
                    last[r] = (dev_ms, between)
            for r in routes:
                row["routes"][r].update(pass_s=[min(times[r]), max(times[r])], runs=len(times[r]), scan_device_ms=last[r][0], between_stages=last[r][1])
                pms[r].close()
            print(json.dumps(row), flush=True)
            rows.append(row)
            with open(args.out, "w") as f:                           # (after every row: a run cut short leaves what it measured)
                json.dump({"rows": rows, "n": args.n, "runs": args.runs, "chunk": args.chunk}, f, indent=1)


if __name__ == "__main__":
    main()
