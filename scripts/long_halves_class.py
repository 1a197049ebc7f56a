#!/usr/bin/env python3
"""Measure what primers of 33..64 nt cost an exact_halves -k 1 pass on the two routes and write
profiles/long_halves_class.json.

Workload: the bench's synthetic stream (--n, default 3 Gbp, uniform A,C,G,T), 100k random 20-mers on both strands under
-k 1 (automatic choice: exact_halves), plus S 40-mers cut from the stream on both strands (half of them exact, half with
one edit), S in --s (default 0,10,1000), and -- S = "alone" -- a list of 100k such 40-mers with no 20-mer beside them.
Every list runs on up to two handles of one process: the long route (bit 3 of pm_config.long_patterns: the list stays on
the halves plan, pm_half_scan<true> + pm_half_verify_wide + pm_seed_extend<32>) and the former route
(PM_LONG_HALVES=off while the handle is created: exact_halves keeps one engine, so the WHOLE list goes to the bit-parallel
kernel).  Timed: the end-to-end pass -- pm_scan_view over 1 GiB ranges, final hits landed on the host -- after one warm-up
pass per handle, --runs runs per handle, the handles taking turns (min - max of the wall time).  Beside it: the device
time of the scan stage of the last pass, the 8-byte records pm_half_scan hands to the verify kernel (pm_scan_stats'
between_stages: the seed records pm_seed_extend gets are at most these times the halves that share a key), and the hit
count and a checksum of the final hits, which must be equal on the routes of a list.

The former route runs the bit-parallel family at 2 x 10^5 patterns over the whole stream: minutes per 3 Gbp pass.  --off-s
names the lists that get that handle at all (default: every list); a run on a shorter stream (--n) times it where the
long stream would not let it.

The same script runs on the commit before the route (PM_GPU_LIB=<that build's libpm_gpu.so>, --parent): one handle per
list, built without the bit; --merge joins outputs of this script (this build's long stream, the parent's, this build's
short stream) into one file and checks hit counts and checksums."""
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


def long_primers(dev, rng, count, L):
    """windows of the stream's first 64 Mi bases: every second one exact, the others with one edit"""
    host = dev[: 1 << 26].cpu().numpy()
    out = []
    while len(out) < count:
        a = int(rng.integers(1, host.size - L - 3))
        w = LUT[host[a:a + L + 2] & 3].tobytes().decode()
        if len(out) % 2 == 0:
            w = w[:L]
        else:
            kind = int(rng.integers(0, 3))
            w = synth.mutate(rng, w[:L], nsub=1) if kind == 0 else synth.mutate(rng, w[:L + 1], ndel=1) if kind == 1 else synth.mutate(rng, w[:L - 1], nins=1)
        w = "".join(w)
        if len(w) == L and set(w) <= set("ACGT"):
            out.append(w)
    return out


def handle(allp, dev, n, route):
    """route: "long" (the permission given), "off" (given, and PM_LONG_HALVES=off in the environment pm_create reads),
    "parent" (a build without the bit)"""
    if route == "off":
        os.environ["PM_LONG_HALVES"] = "off"
    try:
        pm = sat_amd.PatternMatch(k=1, long_halves=True) if route != "parent" else sat_amd.PatternMatch(k=1)
    finally:
        os.environ.pop("PM_LONG_HALVES", None)
    for i, p in enumerate(allp):
        pm.add_pattern(p, i + 1)
    pm.init_device(dev.data_ptr(), n, TABLE, keepalive=dev)
    return pm


def merge(paths, out):
    docs = [json.load(open(p)) for p in paths]
    a = docs[0]
    for b in docs[1:]:
        if b["n"] != a["n"]:                                           # another stream: rows of their own
            a.setdefault("rows_other_streams", []).extend(b["rows"])
            continue
        for rb in b["rows"]:
            ra = next((r for r in a["rows"] if r["S"] == rb["S"]), None)
            if ra is None:
                a["rows"].append(rb)
                continue
            assert (ra["hits"], ra["checksum"]) == (rb["hits"], rb["checksum"]), ("hit count or checksum differ at S = %s" % ra["S"], ra, rb)
            for name, v in rb["routes"].items():
                key = name
                while key in ra["routes"]:
                    key += "'"                                         # a second process of the same build
                ra["routes"][key] = v
    with open(out, "w") as f:
        json.dump(a, f, indent=1)
    for r in a["rows"] + a.get("rows_other_streams", []):
        print(r["S"], r["n"], r["hits"], {k: v["pass_s"] or v["warm_s"] for k, v in r["routes"].items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000_000)
    ap.add_argument("--npat", type=int, default=100_000)
    ap.add_argument("--s", default="0,10,1000,alone")
    ap.add_argument("--off-s", default=None, help="the lists that get the former route's handle (default: all of --s)")
    ap.add_argument("--length", type=int, default=40)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 30)
    ap.add_argument("--parent", action="store_true", help="a build without the bit: one handle per list")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_halves_class.json"))
    ap.add_argument("--merge", nargs="+", metavar="JSON", help="join outputs of this script into --out")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    dev = make_stream(args.n, 7)
    rng = np.random.default_rng(17)
    twenty = [LUT[r].tobytes().decode() for r in rng.integers(0, 4, size=(args.npat, 20), dtype=np.uint8)]
    off_s = (args.off_s if args.off_s is not None else args.s).split(",")
    rows = []
    for S in args.s.split(","):
        alone = S == "alone"
        longs = long_primers(dev, np.random.default_rng(500 + (0 if alone else int(S))), args.npat if alone else int(S), args.length)
        pats = longs if alone else twenty + longs
        allp = pats + [sat_amd.reverse_comp(p) for p in pats]
        routes = ["parent"] if args.parent else ["long"] + (["off"] if S in off_s else [])
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
                t, h, c, dev_ms, between = one_pass(pms[r], args.n, args.chunk)
                assert (h, c) == (row["hits"], row["checksum"]), (S, r)
                times[r].append(t)
                last[r] = (dev_ms, between)
        for r in routes:
            row["routes"][r].update(pass_s=[min(times[r]), max(times[r])] if times[r] else None, runs=len(times[r]),
                                    scan_device_ms=last[r][0], scan_records=last[r][1])
            pms[r].close()
        print(json.dumps(row), flush=True)
        rows.append(row)
    with open(args.out, "w") as f:
        json.dump({"rows": rows, "n": args.n, "runs": args.runs, "chunk": args.chunk}, f, indent=1)


if __name__ == "__main__":
    main()
