"""GPU: pm_align_hits_device (csrc/pm_align.hip) -- the caller's per-hit re-alignment for records that lie in HBM.

The input does not depend on the product: the ORACLE's hits of seeds 0 .. 299 of tests/adversarial.small_case (all four
stream styles, k 0 .. 2, -K / -k, exact zones, ambiguity codes, N in the stream, raw and normalized streams, every
engine) are uploaded and re-aligned on the device.  The results must equal (a) the oracle's own re-alignment
(pmoracle.cli_align) on start, end, editdist for every hit and (b) the host's pm_align_hits / pm_align_hits_text on all
four fields, the alignment string and the matching text."""
import numpy as np
import pytest

import sat_amd
import adversarial as A
from oracle import pmoracle as O

pytestmark = pytest.mark.gpu

SEEDS = range(300)
NONE = 2**31 - 1


def hit_array(tuples):
    h = np.zeros(len(tuples), dtype=sat_amd.HIT_DTYPE)
    if tuples:
        a = np.array(tuples, dtype=np.int64)
        h["end"], h["pid"], h["k"] = a[:, 0], a[:, 1], a[:, 2]
    return h


def make_handle(c, init="auto", patterns=None, route=None):
    """the case's handle; init: auto (pm_init for c['host'], else pm_init_device), host, device, packed; route: further
    keyword arguments of PatternMatch (the permission bits of pm_config.long_patterns), None: the default handle"""
    import torch
    with A.knobs(c["env"]):
        pm = sat_amd.PatternMatch(k=c["k"], indels=c["indels"], semantics=c["sem"], wildcards=c["wild"], **(route or {}))
    for i, p in enumerate(patterns or c["patterns"]):
        z = c["zones"][i] if c["zones"] else (0, 0)
        pm.add_pattern(p, i + 1, z[0], z[1])
    if init == "auto":
        init = "host" if c["host"] else "device"
    if init == "host":
        pm.init(c["stream"], c["table"])
    elif init == "device":
        dev = torch.from_numpy(c["stream"]).cuda()
        pm.init_device(dev.data_ptr(), c["n"], c["table"], keepalive=dev)
    else:
        bits = max(1, int(len(c["table"]) - 1).bit_length())
        pm.init_packed(sat_amd.pattern_match.pack_codes(c["stream"], bits), bits, c["n"], c["table"])
    return pm


def oracle_alignments(c, hits):
    text = O.Text(c["stream"], c["table"])
    out = []
    for end, pid, _ in hits:
        z = c["zones"][pid - 1] if c["zones"] else (0, 0)
        _, st, en, ed, val = O.cli_align(text, c["patterns"][pid - 1], end, c["k"], c["indels"], esb=z[0], eeb=z[1], wildcards=c["wild"])
        out.append((st, en, ed, val))
    return out


def check_against_host(pm, hits, al, ops, txt, what):
    """(b): all four fields against pm_align_hits; the strings against pm_align_hits_text for every record that has an
    alignment (the host call has no strings for a record whose DP gave up at a row: the device writes two empty ones)"""
    host = pm.align_hits(hits)
    for f in ("start", "end", "editdist", "value"):
        bad = np.nonzero(host[f] != al[f])[0]
        assert bad.size == 0, (what, f, hits[bad[0]], host[bad[0]], al[bad[0]])
    has = ~((host["editdist"] == NONE) & (host["start"] == 0) & (host["value"] == 0))
    idx = np.nonzero(has)[0]
    _, hops, htxt = pm.align_hits_text(hits[idx])
    for j, i in enumerate(idx.tolist()):
        assert (ops[i], txt[i]) == (hops[j], htxt[j]), (what, hits[i], al[i], ops[i], hops[j], txt[i], htxt[j])
    for i in np.nonzero(~has)[0].tolist():
        assert (ops[i], txt[i]) == ("", ""), (what, hits[i])
    return int(idx.size)


def test_oracle_hits_realigned_on_the_device():
    kinds = dict(ed0=0, ed1=0, ed2=0, longer=0, shorter=0, near_start=0, beyond_end=0, bogus=0, differs=0)
    with_hits = total = 0
    for seed in SEEDS:
        c = A.small_case(seed)
        want_hits = A.oracle_hits(c)
        assert want_hits is not None, "seed %d: the reference rejects the option set" % seed
        if not want_hits:
            continue
        with_hits += 1
        total += len(want_hits)
        hits = hit_array(want_hits)
        pm = make_handle(c)
        try:
            al, ops, txt = pm.align_hits_device_numpy(hits, text=True)
            want = oracle_alignments(c, want_hits)
            for i, (st, en, ed, _) in enumerate(want):                 # (a) the independent check
                assert (int(al["start"][i]), int(al["end"][i]), int(al["editdist"][i])) == (st, en, ed), (A.describe(c), want_hits[i], al[i], want[i])
            check_against_host(pm, hits, al, ops, txt, A.describe(c))
        finally:
            pm.close()
        for (end, pid, hk), (st, en, ed, _) in zip(want_hits, want):
            L = len(c["patterns"][pid - 1])
            if ed > c["k"]:
                kinds["bogus"] += 1
            else:
                kinds["ed%d" % ed] += 1
                kinds["longer"] += en - st > L
                kinds["shorter"] += en - st < L
                kinds["differs"] += ed != hk
            kinds["near_start"] += end <= L + c["k"]
            kinds["beyond_end"] += end > c["n"]
    print("align_device: %d seeds with hits, %d hits, %s" % (with_hits, total, kinds))
    assert with_hits >= 290
    for name, cnt in kinds.items():
        assert cnt > 0, "no hit of kind %s among the seeds" % name


def test_long_pattern_goes_through_the_host():
    """one 40-mer among 20-mers: its records are beyond the device DP and are aligned by the host inside the same call"""
    rng = np.random.default_rng(77)
    s = rng.integers(0, 4, 6000, dtype=np.uint8)
    lut = "ACGT"
    pats = ["".join(lut[x] for x in s[a:a + 20]) for a in range(100, 2100, 100)]
    long_at = 3000
    pats.append("".join(lut[x] for x in s[long_at:long_at + 40]))
    pats[3] = pats[3][:7] + ("A" if pats[3][7] != "A" else "C") + pats[3][8:]      # one substitution
    pats[5] = pats[5][:9] + pats[5][10:] + "G"                                      # one deletion
    c = dict(k=2, indels=True, sem=sat_amd.SEM_AUTO, wild=False, zones=None, env={}, host=True, stream=s, table=b"ACGT\n", n=s.size, patterns=pats)
    pm = make_handle(c)
    try:
        hits = pm.find_all()
        assert any(int(p) == len(pats) for p in hits["pid"]) and hits.size >= len(pats) - 2
        pm.reset()
        al, ops, txt = pm.align_hits_device_numpy(hits, text=True)
        n_long = int((hits["pid"] == len(pats)).sum())
        _, _, info = pm.counts()
        assert info["aligned_host"] == n_long and info["aligned_device"] == hits.size - n_long
        check_against_host(pm, hits, al, ops, txt, "40-mer among 20-mers")
        want = oracle_alignments(c, sat_amd.sorted_tuples(hits))
        got = sorted(zip(hits["end"].tolist(), hits["pid"].tolist(), al["start"].tolist(), al["end"].tolist(), al["editdist"].tolist()))
        assert [(g[2], g[3], g[4]) for g in got] == [w[:3] for w in want]
    finally:
        pm.close()


@pytest.mark.parametrize("init", ["packed", "device", "host"])
def test_every_resident_form(init):
    """pm_init_packed (resident), pm_init_device and pm_init handles give the same re-alignments"""
    done = 0
    for seed in range(300, 330):
        c = A.small_case(seed)
        if c["raw"]:
            continue
        want_hits = A.oracle_hits(c)
        if not want_hits:
            continue
        hits = hit_array(want_hits)
        pm = make_handle(c, init=init)
        try:
            assert pm.residency()["window"] == 0
            al, ops, txt = pm.align_hits_device_numpy(hits, text=True)
            _, _, info = pm.counts()
            assert info["aligned_device"] == hits.size and info["aligned_host"] == 0
            want = oracle_alignments(c, want_hits)
            assert list(zip(al["start"].tolist(), al["end"].tolist(), al["editdist"].tolist())) == [w[:3] for w in want], A.describe(c)
            check_against_host(pm, hits, al, ops, txt, A.describe(c))
            done += 1
        finally:
            pm.close()
    assert done >= 15


def test_windowed_and_host_only_handles_take_the_host_route():
    c = A.small_case(12)
    want_hits = A.oracle_hits(c)
    for seed in range(12, 40):
        c = A.small_case(seed)
        want_hits = A.oracle_hits(c)
        if want_hits and not c["raw"] and c["n"] > 4000:
            break
    hits = hit_array(want_hits)
    want = [w[:3] for w in oracle_alignments(c, want_hits)]
    for form in ("windowed", "host_only"):
        with A.knobs(c["env"]):
            pm = sat_amd.PatternMatch(k=c["k"], indels=c["indels"], semantics=c["sem"], wildcards=c["wild"])
        try:
            for i, p in enumerate(c["patterns"]):
                z = c["zones"][i] if c["zones"] else (0, 0)
                pm.add_pattern(p, i + 1, z[0], z[1])
            if form == "windowed":
                pm.init(c["stream"], c["table"], window=1024)
            else:
                pm.init_host(c["stream"], c["table"])
            al = pm.align_hits_device_numpy(hits)
            assert list(zip(al["start"].tolist(), al["end"].tolist(), al["editdist"].tolist())) == want, (form, A.describe(c))
            _, _, info = pm.counts()
            assert info["aligned_host"] == hits.size and info["aligned_device"] == 0
        finally:
            pm.close()


def test_argument_checks():
    c = A.small_case(3)
    pm = make_handle(c)
    try:
        import torch
        buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
        with pytest.raises(sat_amd.PmError):
            pm.align_hits_device(0, 4, d_out=buf.data_ptr())                            # no records
        with pytest.raises(sat_amd.PmError):
            pm.align_hits_device(buf.data_ptr(), 1, d_out=buf.data_ptr(), d_ops=buf.data_ptr(), d_text=0, stride=8)   # one string without the other
        bad = hit_array([(100, 10**6, 0)])                                              # unknown pattern id
        with pytest.raises(sat_amd.PmError):
            pm.align_hits_device_numpy(bad)
    finally:
        pm.close()
