"""The bit-packed route (pm_init_packed: a <db>.sqz crosses PCIe packed and is unpacked in HBM) against the
route through one byte per code, on a synthetic stream of --n bases (default 3 Gbp), table ACGT\\nN (3 bits per code),
--primers 20-mers and their reverse complements.  Every figure is taken --runs times (default 3) after a warm-up and
reported as [min, max]; the two routes alternate inside one process.

  1. kernel    pm_unpack_stream<BITS> alone (HIP events), BITS 3, 1, 2, 5, 8: ms and (BITS/8 + 1.25) * n bytes over that
               time, beside pm_measure_stream_read on the same buffer (reads only: an upper mark, not a target)
  2. cold      init + first full pass, -K 2, resident: pm_init_packed against pm_init on the unpacked codes
  3. windowed  steady pass (pm_scan_view in 1 GiB ranges) in 1 GiB and 256 MiB windows, -K 2 and -k 2, packed against
               unpacked windows, with the bytes uploaded per pass
  4. cli       pm_primer_match -K 2 -r -c on the database as .sqz (default route, PM_GPU_PACKED=0, and with --parent-host a
               build of the parent commit) and as .sqn, wall time and -v phases

  python scripts/packed_init.py --out profiles/packed_init.json [--parts kernel,cold,windowed,cli]"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (torch's HIP runtime first, as in __graft_entry__)
import sat_amd  # noqa: E402

TABLE = b"ACGT\nN"
BITS = 3
HOST = os.path.join(ROOT, "sequence-alignment-tools_amd", "host")


def stream(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda", generator=g)
    t[0] = 4
    t[-1] = 4
    t[n // 3] = 4
    return t.cpu().numpy()


def pack(host, bits):
    n = host.size
    out = np.zeros((n * bits + 7) // 8, dtype=np.uint8)
    step = 1 << 27
    for a in range(0, n, step):
        out[a // 8 * bits:(min(n, a + step) * bits + 7) // 8] = sat_amd.pack_codes(host[a:a + step], bits)
    return out


def primers(host, rng, count, L=20):
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    while len(out) < count // 20:
        a = int(rng.integers(1, min(host.size, 1 << 24) - L - 1))
        w = host[a:a + L]
        if not (w > 3).any():
            out.append(lut[w].tobytes().decode())
    out += ["".join("ACGT"[x] for x in rng.integers(0, 4, L)) for _ in range(count - len(out))]
    return out + [sat_amd.reverse_comp(p) for p in out]


def span(v, digits=4):
    return [round(min(v), digits), round(max(v), digits)]


def kernel_part(n, runs):
    rows = []
    d_text = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    d_words = torch.empty((n + 15) // 16 + 128, dtype=torch.int32, device="cuda")
    read_gbs = [sat_amd.measure_stream_read(d_text.data_ptr(), n // 16 * 16, reps=5) for _ in range(runs)]
    for bits in (3, 1, 2, 5, 8):
        nbytes = (n * bits + 7) // 8
        d_packed = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
        for words in (True, False):
            ms = []
            for i in range(runs + 1):                                     # the first launch is the warm-up
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sat_amd.unpack_device(d_packed.data_ptr(), nbytes, bits, n, d_text.data_ptr(), d_words.data_ptr() if words else 0)
                e1.record()
                e1.synchronize()
                if i:
                    ms.append(e0.elapsed_time(e1))
            moved = (bits / 8 + (1.25 if words else 1.0)) * n
            rows.append(dict(bits=bits, words=words, ms=span(ms, 3), bytes_moved=int(moved), gb_s=span([moved / (t * 1e-3) / 1e9 for t in ms], 1)))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        del d_packed
    return dict(n=n, stream_read_gb_s=span(read_gbs, 1), rows=rows)


def handle(pats, k, indels):
    pm = sat_amd.PatternMatch(k=k, indels=indels)
    for i, p in enumerate(pats):
        pm.add_pattern(p, i + 1)
    return pm


def full_pass(pm, n, chunk):
    pm.reset()
    return sum(pm.scan_view(b, min(n, b + chunk)).size for b in range(0, n, chunk))


def init(pm, form, host, packed, window):
    if form == "packed":
        pm.init_packed(packed, BITS, host.size, TABLE, window=window)
    else:
        pm.init(host, TABLE, window=window)


def cold_part(host, packed, pats, runs, chunk):
    out = {"packed": [], "unpacked": []}
    hits = {}
    for i in range(runs + 1):                                             # the first round is the warm-up
        for form in ("unpacked", "packed"):
            pm = handle(pats, 2, False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            init(pm, form, host, packed, None)
            t1 = time.perf_counter()
            cnt = full_pass(pm, host.size, chunk)
            t2 = time.perf_counter()
            res, unpack_ms = pm.residency(), pm.pack_time()
            pm.close()
            hits[form] = cnt
            if i:
                out[form].append(dict(init_s=t1 - t0, cold_s=t2 - t0, pack_or_unpack_ms=unpack_ms, uploaded=res["uploaded"], peak=res["peak"]))
    assert hits["packed"] == hits["unpacked"], hits
    return {form: dict(init_s=span([r["init_s"] for r in v]), init_plus_first_pass_s=span([r["cold_s"] for r in v]),
                       pack_or_unpack_kernel_ms=span([r["pack_or_unpack_ms"] for r in v], 3), uploaded_bytes=v[0]["uploaded"],
                       peak_stream_hbm=v[0]["peak"], hits=hits[form]) for form, v in out.items()}


def windowed_part(host, packed, pats, runs, chunk, windows):
    rows = []
    for k, indels, name in ((2, False, "-K 2"), (2, True, "-k 2")):
        for w in windows:
            pms = {}
            for form in ("unpacked", "packed"):
                pms[form] = handle(pats, k, indels)
                init(pms[form], form, host, packed, w)
            steady = {f: [] for f in pms}
            upl, hits = {}, {}
            for i in range(runs + 1):                                     # the first pass of either handle is the cold one
                for form, pm in pms.items():
                    up0 = pm.residency()["uploaded"]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    hits[form] = full_pass(pm, host.size, chunk)
                    t1 = time.perf_counter()
                    upl[form] = pm.residency()["uploaded"] - up0
                    if i:
                        steady[form].append(t1 - t0)
            for form, pm in pms.items():
                res = pm.residency()
                pm.close()
                rows.append(dict(option=name, window=w, form=form, steady_pass_s=span(steady[form]), uploaded_per_pass=upl[form],
                                 upload_gb_s=span([upl[form] / t / 1e9 for t in steady[form]], 2), peak_stream_hbm=res["peak"], hits=hits[form]))
                print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            assert hits["packed"] == hits["unpacked"], hits
    return rows


def write_db(prefix, host, packed_form):
    """the database files compress_seq writes, directly: one entry, the stream as it is (it starts and ends with the
    end-of-sequence code), as <db>.sqn + .tbl or, padded with end-of-sequence codes to whole bytes, <db>.sqz + .tbz"""
    n = host.size
    if packed_form:
        fill = np.full((-n) % 8, 4, dtype=np.uint8)
        pack(np.concatenate([host, fill]) if fill.size else host, BITS).tofile(prefix + ".sqz")
    else:
        host.tofile(prefix + ".sqn")
    with open(prefix + (".tbz" if packed_form else ".tbl"), "wb") as f:
        f.write(TABLE)
    hdr = b"entry1 synthetic uniform DNA\n"
    with open(prefix + ".hdr", "wb") as f:
        f.write(hdr)
    with open(prefix + ".idb", "wb") as f:
        f.write(struct.pack("<Q", 2) + struct.pack("<qq", 1, 0) + struct.pack("<qq", n + 1, len(hdr)))


def cli_part(host, pats, runs, tmp, parent_host=None):
    out = {}
    with tempfile.TemporaryDirectory(dir=tmp) as d:
        write_db(os.path.join(d, "dbz"), host, True)
        write_db(os.path.join(d, "dbn"), host, False)
        with open(os.path.join(d, "primers.txt"), "w") as f:
            f.write("\n".join(pats[:len(pats) // 2]) + "\n")
        base = {k: v for k, v in os.environ.items() if k not in ("PM_GPU_PACKED", "PM_GPU_WINDOW")}
        routes = [("sqz_packed", "dbz", base, HOST), ("sqz_unpacked_on_host", "dbz", dict(base, PM_GPU_PACKED="0"), HOST), ("sqn", "dbn", base, HOST)]
        if parent_host:                                                   # the same .sqz database through a build of the parent commit
            routes.append(("sqz_parent_build", "dbz", base, parent_host))
        walls = {r[0]: [] for r in routes}
        last = {}
        for i in range(runs + 1):                                         # the first round warms the page cache
            for name, db, env, exe_dir in routes:
                cmd = [os.path.join(exe_dir, "pm_primer_match"), "-i", os.path.join(d, db), "-P", os.path.join(d, "primers.txt"), "-K", "2", "-r", "-c", "-v"]
                t0 = time.perf_counter()
                r = subprocess.run(cmd, capture_output=True, env=env)
                dt = time.perf_counter() - t0
                assert r.returncode == 0, (name, r.stderr[-500:])
                if i:
                    walls[name].append(dt)
                last[name] = (r.stdout, r.stderr.decode("latin1"))
        want = sorted(last["sqn"][0].splitlines())
        for name, _, _, _ in routes:
            out[name] = dict(wall_s=span(walls[name], 3), same_output_as_sqn=sorted(last[name][0].splitlines()) == want,
                             output_lines=len(last[name][0].splitlines()),
                             phases=[x for x in last[name][1].splitlines() if x.startswith("[") or x.startswith("stream")])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=3 * 10 ** 9)
    ap.add_argument("--primers", type=int, default=50_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=1 << 30, help="stream positions per pm_scan call (the command lines' range)")
    ap.add_argument("--windows", default="1073741824,268435456")
    ap.add_argument("--parts", default="kernel,cold,windowed,cli")
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--parent-host", default=None, help="host/ directory of a build of the parent commit: its pm_primer_match is timed on the .sqz database too")
    ap.add_argument("--out")
    a = ap.parse_args()
    parts = a.parts.split(",")
    import bench
    doc = dict(what="bit-packed stream route (pm_init_packed, %d bits per code) against one byte per code; %d bases, %d primers x 2 strands, "
                    "%d runs each after a warm-up, [min, max]" % (BITS, a.n, a.primers, a.runs),
               n=a.n, device=torch.cuda.get_device_name(0), code_sha=bench.code_sha(), head=None)
    if "kernel" in parts:
        doc["kernel"] = kernel_part(a.n, a.runs)
    if set(parts) & {"cold", "windowed", "cli"}:
        host = stream(a.n, 7)
        rng = np.random.default_rng(7)
        pats = primers(host, rng, a.primers)
        packed = pack(host, BITS)
        if "cold" in parts:
            doc["cold_resident_K2"] = cold_part(host, packed, pats, a.runs, a.chunk)
            print(json.dumps(doc["cold_resident_K2"]), file=sys.stderr, flush=True)
        if "windowed" in parts:
            doc["windowed_steady"] = windowed_part(host, packed, pats, a.runs, a.chunk, [int(x) for x in a.windows.split(",")])
        if "cli" in parts:
            del packed
            doc["cli_primer_match_K2_counts"] = cli_part(host, pats, a.runs, a.tmp, a.parent_host)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
