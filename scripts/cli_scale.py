#!/usr/bin/env python3
"""End-to-end timing of the command lines at BASELINE.json's sizes (run on the GPU box).

Writes a synthetic database directly in compress_seq's file formats (<db>.sqn/.tbl/.idb/.hdr:
uniform A,C,G,T, 24 entries), a primer list (10 % planted with 0-2 substitutions) and a UniSTS
primer-pair file (10 % planted at amplicon length U[100,1000]), then times
    pm_primer_match -K 2 -r -c          (configs[2]/[3] through the CLI)
    pm_primer_match -k 1 -r -A ...      (alignment output)
    pm_pcr_match    -k 1 -S ... -M 1000 (configs[4])
with -v phase timings, and -- on a bounded sample of the same inputs -- the reference binaries
oracle/_ref/primer_match and oracle/_ref/pcr_match (1 thread) when they are present.
Prints one JSON object.  Usage: python scripts/cli_scale.py --bases 3000000000 --primers 100000 --pairs 100000

--stream-style tandem writes tandem-repeat text instead (the generator of tests/adversarial.py and bench.py --stream-style:
units of 1..39 bases, 1..399 copies, 3 % of the bases drifted) and cuts every primer and every primer pair from it;
--pcr-case K2_pairs times `pm_pcr_match -K 2 -r -P <pairs> -M 1000` (no size bounds: every hit of one primer pairs with every hit
of its partner inside the window, so the candidate pairs grow with the product of a pair's hit counts) instead of the UniSTS case.
"""
import argparse
import json
import os
import resource
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")
REF = os.path.join(ROOT, "oracle", "_ref")
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(b):
    return b.translate(COMP)[::-1]


def write_db(prefix, codes, entries):
    """codes: uint8 array of bases (0..3), split into `entries` equal entries."""
    n = codes.size
    per = n // entries
    bounds = [i * per for i in range(entries)] + [n]
    with open(prefix + ".sqn", "wb") as f:
        f.write(b"\x04")
        for i in range(entries):
            f.write(codes[bounds[i]:bounds[i + 1]].tobytes())
            f.write(b"\x04")
    with open(prefix + ".tbl", "wb") as f:
        f.write(b"ACGT\n")
    hdr = b""
    keys, vals = [], []
    pos = 1
    for i in range(entries):
        keys.append(pos)
        vals.append(len(hdr))
        hdr += ("entry%d synthetic uniform DNA\n" % (i + 1)).encode()
        pos += bounds[i + 1] - bounds[i] + 1
    keys.append(pos + 1)                       # compress_seq counts the final EOS twice
    vals.append(len(hdr))
    with open(prefix + ".hdr", "wb") as f:
        f.write(hdr)
    with open(prefix + ".idb", "wb") as f:
        f.write(struct.pack("<Q", len(keys)))
        for k, v in zip(keys, vals):
            f.write(struct.pack("<qq", k, v))
    return bounds


def tandem_codes(rng, n):
    """tandem repeats of short units with drifting copies (tests/adversarial.py make_stream, style 3) at database size"""
    s = np.empty(n, dtype=np.uint8)
    at = 0
    while at < n:
        unit = rng.integers(0, 4, int(rng.integers(1, 40)), dtype=np.uint8)
        blk = np.tile(unit, int(rng.integers(1, 400)))
        m = rng.random(blk.size) < 0.03
        blk[m] = rng.integers(0, 4, int(m.sum()), dtype=np.uint8)
        blk = blk[: n - at]
        s[at:at + blk.size] = blk
        at += blk.size
    return s


def mutate(rng, w, nsub):
    w = bytearray(w)
    for _ in range(nsub):
        i = int(rng.integers(0, len(w)))
        w[i] = rng.choice([c for c in b"ACGT" if c != w[i]])
    return bytes(w)


LAST_CPU = [0.0, 0.0]


def run_timed(cmd, stdout, env=None):
    """wall seconds, return code and stderr of one process; its user and system CPU seconds (all its threads, up to the
    end of its teardown) are left in LAST_CPU"""
    r0 = resource.getrusage(resource.RUSAGE_CHILDREN)
    t0 = time.time()
    with open(stdout, "wb") as f:
        r = subprocess.run(cmd, stdout=f, stderr=subprocess.PIPE, env=env)
    dt = time.time() - t0
    r1 = resource.getrusage(resource.RUSAGE_CHILDREN)
    LAST_CPU[:] = [r1.ru_utime - r0.ru_utime, r1.ru_stime - r0.ru_stime]
    return dt, r.returncode, r.stderr.decode("latin1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1_000_000_000)
    ap.add_argument("--entries", type=int, default=24)
    ap.add_argument("--primers", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--ref-sample", type=int, default=30_000_000, help="bases for the reference binaries (0 = skip)")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--gpu-counts", choices=["0", "1", "both"], default="0",
                    help="the -c cases with PM_GPU_COUNTS=0 (the host loop, pm_primer_match's default), =1 (the device tally), or both (the host loop's runs are named *_host_tally)")
    ap.add_argument("--counts-only", action="store_true", help="only the two -c cases")
    ap.add_argument("--gpu-pcr", choices=["0", "1", "both"], default="0",
                    help="pm_pcr_match with PM_GPU_PCR=0 (the host loop, its default), =1 (the pairing stage on the device), or both (the device route's runs are named *_gpu_pairing)")
    ap.add_argument("--pcr-only", action="store_true", help="only the pm_pcr_match case")
    ap.add_argument("--pcr-case", choices=["k1_sts", "K2_pairs"], default="k1_sts",
                    help="the pm_pcr_match case: -k 1 -S <UniSTS file> (configs[4]) or -K 2 -r -P <primer pairs>, which has no size bounds (the hit-dense case)")
    ap.add_argument("--pcr-order", choices=["host-first", "device-first"], default="host-first", help="with --gpu-pcr both: which route's processes run first")
    ap.add_argument("--stream-style", choices=["uniform", "tandem"], default="uniform",
                    help="uniform A,C,G,T, or tandem-repeat text with every primer and primer pair cut from it")
    ap.add_argument("--repeat", type=int, default=2, help="processes per command (wall_s is the fastest, all are kept)")
    args = ap.parse_args()
    if args.pcr_only and (args.counts_only or args.gpu_counts == "both"):
        ap.error("--pcr-only runs no -c case: it goes with neither --counts-only nor --gpu-counts both")
    tandem = args.stream_style == "tandem"
    rng = np.random.default_rng(20260101)
    res = {"bases": args.bases, "stream_style": args.stream_style, "entries": args.entries, "primers": args.primers, "pairs": args.pairs, "runs": {}}
    with tempfile.TemporaryDirectory(dir=args.tmp) as d:
        t0 = time.time()
        codes = tandem_codes(rng, args.bases) if tandem else rng.integers(0, 4, size=args.bases, dtype=np.uint8)
        db = os.path.join(d, "db")
        bounds = write_db(db, codes, args.entries)
        lut = np.frombuffer(b"ACGT", dtype=np.uint8)
        head = lut[codes[:min(args.bases, 1 << 26)]].tobytes()           # planted sites come from the first 64 Mbp
        # primers
        prim = []
        for i in range(args.primers):
            if i % 10 == 0 or tandem:
                a = int(rng.integers(0, len(head) - 20))
                prim.append(mutate(rng, head[a:a + 20], i // 10 % 3))
            else:
                prim.append(lut[rng.integers(0, 4, size=20)].tobytes())
        with open(os.path.join(d, "primers.txt"), "wb") as f:
            f.write(b"\n".join(prim) + b"\n")
        # primer pairs (UniSTS lines)
        per = args.bases // args.entries
        with open(os.path.join(d, "pairs.sts"), "wb") as f, open(os.path.join(d, "pairs.txt"), "wb") as fp:
            for i in range(args.pairs):
                if i % 10 == 0 or tandem:
                    amp = int(rng.integers(100, 1001))
                    a = int(rng.integers(0, min(len(head), per) - amp))       # inside the first entry
                    fwd, rev = head[a:a + 20], revcomp(head[a + amp - 20:a + amp])
                    if i % 20 == 0:
                        fwd = mutate(rng, fwd, 1)
                else:
                    amp = 500
                    fwd, rev = lut[rng.integers(0, 4, size=20)].tobytes(), lut[rng.integers(0, 4, size=20)].tobytes()
                f.write(b"STS%d\t%s\t%s\t%d\tACC%d\t1\tALT%d\tsynthetic\n" % (i + 1, fwd, rev, amp, i + 1, i + 1))
                fp.write(fwd + b" " + rev + b"\n")
        res["generate_s"] = time.time() - t0
        del codes

        runs = [
            ("primer_match_K2_counts", [os.path.join(HOST, "pm_primer_match"), "-i", db, "-P", os.path.join(d, "primers.txt"), "-K", "2", "-r", "-c", "-v"]),
            ("primer_match_k2_counts", [os.path.join(HOST, "pm_primer_match"), "-i", db, "-P", os.path.join(d, "primers.txt"), "-k", "2", "-r", "-c", "-v"]),
            ("primer_match_k1_align", [os.path.join(HOST, "pm_primer_match"), "-i", db, "-P", os.path.join(d, "primers.txt"), "-k", "1", "-r", "-A", "%i %r %s %e %d %H\\n", "-v"]),
            ("pcr_match_k1_sts", [os.path.join(HOST, "pm_pcr_match"), "-i", db, "-S", os.path.join(d, "pairs.sts"), "-k", "1", "-M", "1000", "-A", "%I %H %>s %<e %l %>d %<d %r\\n", "-v"]),
        ]
        pcr = "pcr_match_" + args.pcr_case
        if args.pcr_case == "K2_pairs":
            runs[3] = (pcr, [os.path.join(HOST, "pm_pcr_match"), "-i", db, "-P", os.path.join(d, "pairs.txt"), "-K", "2", "-r", "-M", "1000", "-A", "%i %H %>s %<e %l %>d %<d %r\\n", "-v"])
        if args.counts_only:
            runs = runs[:2]
        host_env, dev_env = dict(os.environ, PM_GPU_COUNTS="0"), dict(os.environ, PM_GPU_COUNTS="1")
        envs = {name: (dev_env if args.gpu_counts in ("1", "both") else host_env) for name, _ in runs[:2]}
        if args.gpu_counts == "both":
            extra = [(name + "_host_tally", cmd) for name, cmd in runs[:2]]
            envs.update({name: host_env for name, _ in extra})
            runs = runs[:2] + extra + runs[2:]
        pcr_host, pcr_dev = dict(os.environ, PM_GPU_PCR="0"), dict(os.environ, PM_GPU_PCR="1")
        envs[pcr] = pcr_dev if args.gpu_pcr == "1" else pcr_host
        if args.gpu_pcr == "both" and not args.counts_only:
            envs[pcr + "_gpu_pairing"] = pcr_dev
            dev_run = (pcr + "_gpu_pairing", dict(runs)[pcr])
            runs = runs[:-1] + ([dev_run, runs[-1]] if args.pcr_order == "device-first" else [runs[-1], dev_run])
        if args.pcr_only:                                            # after the -c handling, which counts on runs[:2]
            runs = [r for r in runs if r[0].startswith(pcr)]
        for name, cmd in runs:
            # every command twice, each a new process (HIP start, tables, upload, scan, report: nothing survives between them but the
            # page cache, which holds the database either way -- it was written a moment ago); wall_s is the faster one, both are kept:
            # process start and exit on a shared box vary by 0.1 s from run to run
            walls, errs, cpus = [], [], []
            for _ in range(max(1, args.repeat)):
                dt_i, rc, err_i = run_timed(cmd, os.path.join(d, name + ".out"), envs.get(name))
                walls.append(dt_i)
                cpus.append(list(LAST_CPU))
                errs.append([l for l in err_i.splitlines() if l.startswith("scan")])
                if dt_i == min(walls):
                    dt, err = dt_i, err_i
            with open(os.path.join(d, name + ".out"), "rb") as f:
                nlines = sum(1 for _ in f)
            res["runs"][name] = {"wall_s": dt, "wall_s_runs": walls, "user_sys_cpu_s_runs": cpus, "scan_lines_runs": errs, "rc": rc, "output_lines": nlines, "gbases_per_s_wall": args.bases / dt / 1e9,
                                 "phases": [l for l in err.splitlines() if l.startswith("[") or l.startswith("scan") or l.startswith("counts")]}
            print(name, "%.2f s" % dt, file=sys.stderr, flush=True)

        # the reference binaries on a bounded sample of the same database (same primer files)
        if args.gpu_counts == "both":                                # the two routes print the same lines
            for name, _ in runs[:2]:
                with open(os.path.join(d, name + ".out"), "rb") as fa, open(os.path.join(d, name + "_host_tally.out"), "rb") as fb:
                    res["runs"][name]["same_output_as_host_tally"] = fa.read() == fb.read()
        if args.gpu_pcr == "both" and not args.counts_only:
            with open(os.path.join(d, pcr + ".out"), "rb") as fa, open(os.path.join(d, pcr + "_gpu_pairing.out"), "rb") as fb:
                res["runs"][pcr + "_gpu_pairing"]["same_output_as_host_loop"] = fa.read() == fb.read()
        if args.ref_sample > 0 and not args.counts_only and not args.pcr_only and args.pcr_case == "k1_sts" and os.path.exists(os.path.join(REF, "pcr_match")):
            ns = min(args.ref_sample, args.bases)
            codes = np.fromfile(db + ".sqn", dtype=np.uint8, count=ns + 1)[1:]
            sdb = os.path.join(d, "sample")
            write_db(sdb, codes, 1)
            for name, cmd in [
                ("ref_primer_match_k1_align", [os.path.join(REF, "primer_match"), "-i", sdb, "-P", os.path.join(d, "primers.txt"), "-k", "1", "-r", "-A", "%i %r %s %e %d %H\\n"]),
                ("ref_pcr_match_k1_sts", [os.path.join(REF, "pcr_match"), "-i", sdb, "-S", os.path.join(d, "pairs.sts"), "-k", "1", "-M", "1000", "-A", "%I %H %>s %<e %l %>d %<d %r\\n"]),
            ]:
                dt, rc, err = run_timed(cmd, os.path.join(d, name + ".out"))
                with open(os.path.join(d, name + ".out"), "rb") as f:
                    nlines = sum(1 for _ in f)
                res["runs"][name] = {"wall_s": dt, "rc": rc, "output_lines": nlines, "sample_bases": ns, "gbases_per_s_wall": ns / dt / 1e9,
                                     "stderr_tail": err[-300:]}
                print(name, "%.2f s" % dt, file=sys.stderr, flush=True)
            # same sample through our CLIs: outputs must agree
            for name, exe, ref in [("primer_match_k1_align", "pm_primer_match", "ref_primer_match_k1_align"), ("pcr_match_k1_sts", "pm_pcr_match", "ref_pcr_match_k1_sts")]:
                cmd = [c if c != db else sdb for c in dict(runs)[name]]
                dt, rc, err = run_timed(cmd, os.path.join(d, name + ".sample.out"))
                with open(os.path.join(d, name + ".sample.out"), "rb") as f:
                    got = sorted(f.read().splitlines())
                with open(os.path.join(d, ref + ".out"), "rb") as f:
                    want = sorted(f.read().splitlines())
                res["runs"][ref]["gpu_cli_same_output"] = got == want
                res["runs"][ref]["gpu_cli_wall_s_on_sample"] = dt
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
