#!/usr/bin/env python3
"""A/B of the slot table's overflow markers (csrc/pm_pair.hip, pair_build): bench.py runs with the markers holding their
keys' patterns (the product) interleaved with runs on the empty flagged markers of earlier versions (PM_SEED_DEBUG bit 6),
one fresh process per run, on one GPU.

    python scripts/pair_markers_ab.py --reps 3 --out profiles/x.jsonl -- --steps 20 --warmup 5 --no-cpu
    python scripts/pair_markers_ab.py --reps 1 --rows 11,12 -- --steps 20 --warmup 5 --no-cpu          # PM_PAIR_ROW, product markers only

Everything behind `--` goes to bench.py.  Per run one JSON line: side, PM_PAIR_ROW, value, ms_per_step, roofline.kernel_ms,
config.scan_stats.between_stages, candidates.  The first run that fails or exceeds its time limit ends the script.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(side, row, bench_args, limit):
    env = dict(os.environ)
    env.pop("PM_SEED_DEBUG", None)
    env.pop("PM_PAIR_ROW", None)
    if side == "empty":
        env["PM_SEED_DEBUG"] = "64"
    if row:
        env["PM_PAIR_ROW"] = str(row)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + bench_args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit("bench.py failed (%s, row %s): exit status %d" % (side, row, r.returncode))
    d = json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1])
    return {"side": side, "row": row or None, "args": " ".join(bench_args), "value": d["value"], "ms_per_step": d["ms_per_step"],
            "kernel_ms": d.get("roofline", {}).get("kernel_ms"), "between_stages": d["config"].get("scan_stats", {}).get("between_stages"),
            "candidates": d["config"].get("candidates"), "kernel": d["config"].get("kernel")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", default="", help="comma-separated PM_PAIR_ROW values: product markers only, one run per value and repetition")
    ap.add_argument("--out", default="")
    ap.add_argument("--limit", type=int, default=240, help="seconds per bench.py run")
    ap.add_argument("bench", nargs="*")
    a = ap.parse_args()
    runs = [("filled", int(x)) for x in a.rows.split(",") if x] if a.rows else [("empty", 0), ("filled", 0)]
    for rep in range(a.reps):
        for side, row in runs:
            row_ = one(side, row, a.bench, a.limit)
            row_["rep"] = rep
            line = json.dumps(row_)
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
