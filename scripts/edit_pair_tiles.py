#!/usr/bin/env python3
"""Measure the edit plan's first stage on the pair geometry against the hashed-piece kernel pm_edit_scan where the
PM_EDIT_PAIR bit of pm_config.long_patterns moves it and write profiles/edit_pair_tiles.json.

Workload: the bench's synthetic stream (--n, default 3 Gbp, uniform A,C,G,T) and random 20-mers on both strands.  Lines:
  a  1M 20-mers x 2 strands, -k 2, filter_bitvec            (eight pattern tiles)
  b  100k x 2, -k 1, filter_bitvec                           (pm_pair_edit_scan_k1: two tests per window)
  c  100k x 2, -3 8 -k 2, exact_bases                        (pm_bases_verify behind the pair geometry)
  d  100k x 2, -k 2, filter_bitvec                           (one tile: the same route with and without the bit)
Every line runs on two handles of one process and one library, the bit set ("pair") and clear ("clear"), which take turns:
one warm-up pass each (buffers grow to their size), then --runs timed passes -- pm_scan_view over 1 GiB ranges, final hits
landed on the host.  Recorded per handle: pm_describe, the pass's wall time and the device time of its scan stages (min -
max over the timed passes), seed records and suspects of a pass (per range: the tile with most; summed over the ranges),
launches.  The final hits of the two handles are compared as sorted arrays: a difference ends the script with a non-zero
status.

--parent: one handle per line, built without the bit -- for a run on the commit before this route
(PM_GPU_LIB=<that build's libpm_gpu.so>).  --merge THIS PARENT [PARENT ...] joins the outputs (hit counts and checksums
must agree) into --out and pools the parent runs' spreads."""
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
from short_class import LUT, TABLE, make_stream  # noqa: E402

# line -> (primers per strand, PatternMatch arguments, exact_start_bases / exact_end_bases of every primer)
LINES = {
    "a": (1_000_000, dict(k=2, indels=True, semantics=sat_amd.SEM_FILTER_BITVEC), (0, 0)),
    "b": (100_000, dict(k=1, indels=True, semantics=sat_amd.SEM_FILTER_BITVEC), (0, 0)),
    "c": (100_000, dict(k=2, indels=True, semantics=sat_amd.SEM_EXACT_BASES, kernel=sat_amd.KERNEL_SEED), (0, 8)),
    "d": (100_000, dict(k=2, indels=True, semantics=sat_amd.SEM_FILTER_BITVEC), (0, 0)),
}


def handle(line, allp, dev, n, route):
    _, kw, zone = LINES[line]
    pm = sat_amd.PatternMatch(edit_pair=True, **kw) if route == "pair" else sat_amd.PatternMatch(**kw)
    for i, p in enumerate(allp):
        pm.add_pattern(p, i + 1, zone[0], zone[1])
    pm.init_device(dev.data_ptr(), n, TABLE, keepalive=dev)
    return pm


def one_pass(pm, n, chunk, keep):
    """a pass over the stream; keep: also the hits as sorted keys end << 24 | id << 2 | k"""
    t0 = time.perf_counter()
    pm.reset()
    pos = nhits = launches = 0
    dev_ms, seeds, susp, keys = 0.0, 0, 0, []
    while pos < n:
        end = min(n, pos + chunk)
        hits = pm.scan_view(pos, end)
        nhits += int(hits.size)
        if keep and hits.size:
            assert int(hits["pid"].max()) < (1 << 22)
            keys.append((hits["end"].astype(np.uint64) << np.uint64(24)) | (hits["pid"].astype(np.uint64) << np.uint64(2)) | hits["k"].astype(np.uint64))
        ms, nl = pm.last_kernel_time()
        dev_ms += ms
        launches += nl
        st = pm.scan_stats()
        seeds += st["between_stages"]
        susp += st.get("edit_suspects", 0)
        pos = end
    wall = time.perf_counter() - t0
    return dict(wall_s=wall, hits=nhits, scan_device_ms=dev_ms, seed_records=seeds, suspects=susp, launches=launches), (np.sort(np.concatenate(keys)) if keys else np.zeros(0, np.uint64))


def checksum(keys):
    return int(np.bitwise_xor.reduce(keys * np.uint64(0x9E3779B97F4A7C15))) if keys.size else 0


def merge(paths, out):
    docs = [json.load(open(p)) for p in paths]
    this, parents = docs[0], docs[1:]
    for line, row in this["lines"].items():
        pooled = None
        for p in parents:
            r = p["lines"].get(line)
            if r is None:
                continue
            assert (row["hits"], row["checksum"]) == (r["hits"], r["checksum"]), ("hit count or checksum differ on line " + line, row["hits"], r["hits"])
            q = r["routes"]["parent"]
            if pooled is None:
                pooled = dict(q, processes=1)
            else:
                for f in ("pass_s", "scan_device_ms"):
                    pooled[f] = [min(pooled[f][0], q[f][0]), max(pooled[f][1], q[f][1])]
                pooled["runs"] += q["runs"]
                pooled["processes"] += 1
        if pooled:
            row["routes"]["parent"] = pooled
    with open(out, "w") as f:
        json.dump(this, f, indent=1)
    for line, row in this["lines"].items():
        print(line, row["hits"], {r: (v["pass_s"], v["scan_device_ms"]) for r, v in row["routes"].items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3_000_000_000)
    ap.add_argument("--lines", default="a,b,c,d")
    ap.add_argument("--scale", type=float, default=1.0, help="primers per line, as a fraction (smoke runs)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 30)
    ap.add_argument("--parent", action="store_true", help="a build without the bit: one handle per line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_pair_tiles.json"))
    ap.add_argument("--merge", nargs="+", metavar="JSON", help="THIS PARENT [PARENT ...]: join outputs of this script into --out")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.out)
    dev = make_stream(args.n, 7)
    doc = {"n": args.n, "runs": args.runs, "chunk": args.chunk, "lines": {}}
    for line in args.lines.split(","):
        npat = max(1000, int(LINES[line][0] * args.scale))
        rng = np.random.default_rng(170 + ord(line))
        pats = [LUT[r].tobytes().decode() for r in rng.integers(0, 4, size=(npat, 20), dtype=np.uint8)]
        allp = pats + [sat_amd.reverse_comp(p) for p in pats]
        routes = ["parent"] if args.parent else ["pair", "clear"]
        row = {"patterns": len(allp), "options": {k: int(v) for k, v in LINES[line][1].items()}, "zone": list(LINES[line][2]), "routes": {}}
        pms, passes, ref = {}, {r: [] for r in routes}, None
        for r in routes:
            t0 = time.perf_counter()
            pms[r] = handle(line, allp, dev, args.n, r)
            row["routes"][r] = {"kernel": pms[r].describe(), "init_s": time.perf_counter() - t0}
            print("line %s, %s: %s" % (line, r, row["routes"][r]["kernel"]), flush=True)
            warm, keys = one_pass(pms[r], args.n, args.chunk, True)            # warm-up pass; its hits are the ones compared
            row["routes"][r]["warm_s"] = warm["wall_s"]
            if ref is None:
                ref = keys
                row["hits"], row["checksum"] = int(keys.size), checksum(keys)
            elif not (ref.size == keys.size and np.array_equal(ref, keys)):
                print("line %s: the routes' final hits differ (%d against %d)" % (line, ref.size, keys.size), flush=True)
                sys.exit(1)
        for _ in range(args.runs):                                   # the handles take turns
            for r in routes:
                p, _ = one_pass(pms[r], args.n, args.chunk, False)
                assert p["hits"] == row["hits"], (line, r, p["hits"], row["hits"])
                passes[r].append(p)
        for r in routes:
            ps = passes[r]
            row["routes"][r].update(runs=len(ps), pass_s=[min(p["wall_s"] for p in ps), max(p["wall_s"] for p in ps)],
                                    scan_device_ms=[min(p["scan_device_ms"] for p in ps), max(p["scan_device_ms"] for p in ps)],
                                    seed_records=ps[-1]["seed_records"], suspects=ps[-1]["suspects"], launches=ps[-1]["launches"])
            pms[r].close()
        row["hits_equal"] = len(routes) == 2
        print(json.dumps({line: row}), flush=True)
        doc["lines"][line] = row
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:                               # (after every line: a later line's failure leaves the earlier ones)
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
