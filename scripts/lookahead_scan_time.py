"""How tests/test_gpu_scan_lookahead.py chooses its range length R: on the dense stream ("AC" repeated; the patterns (AC)x10
and (CA)x10, tests/dense_stream.py) the scan-kernel time of one range (pm_last_kernel_time, best of three) against a lower
bound of the time its hit records take to reach the host (16-byte records over a 64 GB/s link), for every pass-through
option set and R = 2^17 .. 2^23; plus the host time of a four-range pm_scan_view walk and pm_scan_stats.

    python scripts/lookahead_scan_time.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch  # noqa: F401
import sat_amd

TABLE = b"ACGT\n"
PATS = ["AC" * 10, "CA" * 10]
SETS = {
    "k0": dict(k=0, indels=True, semantics=sat_amd.SEM_AUTO),
    "sai_K1": dict(k=1, indels=False, semantics=sat_amd.SEM_SHIFT_AND_INEXACT),
    "sai_k1": dict(k=1, indels=True, semantics=sat_amd.SEM_SHIFT_AND_INEXACT),
    "bases_K1": dict(k=1, indels=False, semantics=sat_amd.SEM_EXACT_BASES),
    "bases_K1_seed": dict(k=1, indels=False, semantics=sat_amd.SEM_EXACT_BASES, kernel=sat_amd.KERNEL_SEED),
}
print("library", sat_amd.library_path(), flush=True)
for name, kw in SETS.items():
    for lg in (17, 19, 20, 21, 22, 23):
        R = 1 << lg
        codes = np.tile(np.array([0, 1], dtype=np.uint8), 2 * R)
        pm = sat_amd.PatternMatch(**kw)
        zone = 4 if name.startswith("bases") else 0
        for i, p in enumerate(PATS):
            pm.add_pattern(p, i + 1, zone, 0)
        pm.init(codes, TABLE)
        if lg == 17:
            print(name, "describe:", pm.describe(), "selected", pm.selected(), flush=True)
        best = None
        for rep in range(3):
            n = pm.scan_candidates(R, 2 * R, to_host=False)
            ms, launches = pm.last_kernel_time()
            best = ms if best is None else min(best, ms)
        copy_ms = n * 16 / 64e9 * 1e3
        # one look-ahead walk, timed on the host
        pm.reset()
        t0 = time.perf_counter()
        tot = 0
        for j in range(4):
            tot += pm.scan_view(j * R, (j + 1) * R).size
        t1 = time.perf_counter()
        print("%s R=2^%d records/range=%d scan_ms=%.4f (launches %d) copy_lower_bound_ms=%.4f ratio=%.2f walk4_ms=%.1f hits=%d stats=%s" %
              (name, lg, n, best, launches, copy_ms, copy_ms / best if best else -1, (t1 - t0) * 1e3, tot, pm.scan_stats()), flush=True)
        pm.close()
