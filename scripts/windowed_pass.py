"""Windowed stream (pm_init_windowed) against the resident form on a 3 Gbp synthetic stream, 100k 20-mers (50k and their
reverse complements), -K 2 and -k 2, windows of 256 MiB, 1 GiB and 4 GiB.  Per row: cold init + one full pass, the
steady pass (second pass on the same handle; pm_scan_view in the command lines' 1 GiB ranges), effective upload rate, the fraction of the scan hidden behind the upload,
peak HBM held for the stream, and whether the hits equal the resident form's.  One JSON document on stdout (and to
--out).

  python scripts/windowed_pass.py --out profiles/windowed_pass.json

"hidden" compares three passes: the option set resident (scan only), a windowed pass of a one-primer -K 0 handle with
the same window (upload + a near-free scan) and the option set windowed: 1 - (windowed - upload_only) / resident.
1 = the scan is entirely hidden behind the copies, 0 = the two run one after the other."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch's HIP runtime first, as in __graft_entry__)
import sat_amd  # noqa: E402

TABLE = b"ACGT\n"


def stream(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda", generator=g)
    t[0] = 4
    t[-1] = 4
    t[n // 3] = 4
    return t.cpu().numpy()


def primers(host, rng, count, L=20):
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    while len(out) < count // 20:
        a = int(rng.integers(1, (1 << 24) - L - 1))
        w = host[a:a + L]
        if not (w > 3).any():
            out.append(lut[w].tobytes().decode())
    out += ["".join("ACGT"[x] for x in rng.integers(0, 4, L)) for _ in range(count - len(out))]
    return out + [sat_amd.reverse_comp(p) for p in out]


def one(host, pats, k, indels, window, chunk):
    pm = sat_amd.PatternMatch(k=k, indels=indels)
    for i, p in enumerate(pats):
        pm.add_pattern(p, i + 1)
    def full_pass():                                              # pm_scan_view over the stream in ranges of `chunk` bytes
        pm.reset()
        parts = [pm.scan_view(b, min(host.size, b + chunk)).copy() for b in range(0, host.size, chunk)]
        return np.concatenate(parts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pm.init(host, TABLE, window=window)
    t1 = time.perf_counter()
    hits = full_pass()
    t2 = time.perf_counter()
    up0 = pm.residency()["uploaded"]
    t3 = time.perf_counter()
    again = full_pass()
    t4 = time.perf_counter()
    res = pm.residency()
    pm.close()
    assert again.size == hits.size
    return dict(init_s=t1 - t0, cold_s=t2 - t0, steady_s=t4 - t3, steady_uploaded=res["uploaded"] - up0, res=res), hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3 * 10 ** 9)
    ap.add_argument("--primers", type=int, default=50_000)
    ap.add_argument("--chunk", type=int, default=1 << 30, help="stream bytes per pm_scan call (the command lines' range)")
    ap.add_argument("--windows", default="268435456,1073741824,4294967296")
    ap.add_argument("--out")
    a = ap.parse_args()
    host = stream(a.n, 7)
    rng = np.random.default_rng(7)
    pats = primers(host, rng, a.primers)
    windows = [int(x) for x in a.windows.split(",")]
    rows = []
    upload_only = {}
    for w in windows:                                             # upload + a near-free scan: the copy-bound floor of a pass
        r, _ = one(host, ["ACGTACGTACGTACGTACGT"], 0, False, w, a.chunk)
        upload_only[w] = r["steady_s"]
    for k, indels, name in ((2, False, "-K 2"), (2, True, "-k 2")):
        base, want = one(host, pats, k, indels, None, a.chunk)
        rows.append(dict(option=name, mode="resident", window=0, cold_init_plus_pass_s=round(base["cold_s"], 4), init_s=round(base["init_s"], 4),
                         steady_pass_s=round(base["steady_s"], 4), peak_stream_hbm=base["res"]["peak"], hits=int(want.size)))
        for w in windows:
            r, got = one(host, pats, k, indels, w, a.chunk)
            same = got.size == want.size and bool((got["end"] == want["end"]).all() and (got["pid"] == want["pid"]).all() and (got["k"] == want["k"]).all())
            hidden = 1.0 - (r["steady_s"] - upload_only[w]) / base["steady_s"] if base["steady_s"] > 0 else None
            rows.append(dict(option=name, mode="windowed", window=w, cold_init_plus_pass_s=round(r["cold_s"], 4), init_s=round(r["init_s"], 4),
                             steady_pass_s=round(r["steady_s"], 4), upload_only_pass_s=round(upload_only[w], 4),
                             upload_gb_s=round(r["steady_uploaded"] / r["steady_s"] / 1e9, 2),
                             scan_hidden_fraction=None if hidden is None else round(max(0.0, min(1.0, hidden)), 3),
                             peak_stream_hbm=r["res"]["peak"], loads_per_pass=r["res"]["loads"] // 2, hits=int(got.size), same_hits=same))
            print(json.dumps(rows[-1]), file=sys.stderr)
    doc = dict(what="pm_init_windowed against pm_init, 3 Gbp synthetic stream, %d primers x 2 strands, pm_scan ranges of %d bytes" % (a.primers, a.chunk),
               n=a.n, device=torch.cuda.get_device_name(0), rows=rows)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
