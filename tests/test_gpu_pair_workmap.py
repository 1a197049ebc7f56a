"""GPU: the pair scan kernels give the same records under every workgroup -> (field pair, chunk) map (csrc/pm_workmap.h):
the superchunk map (the default for ranges of fewer than 1280 chunks and for the edit plan), the XCD superchunk map
(pm_pair_scan's default from 1280 chunks on) and the XCD map, each forced with PM_PAIR_MAP on ranges where the default would take another.  Records are
compared byte for byte, in sorted order (the verify kernel appends them in no fixed order)."""
import numpy as np
import pytest
import torch

import adversarial as A
import sat_amd

pytestmark = pytest.mark.gpu
TABLE = b"ACGT\n"
LUT = np.frombuffer(b"ACGT", dtype=np.uint8)
MAPS = ("superchunk", "xcd-superchunk", "xcd")


def random_db(n, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(0, 4, (n,), dtype=torch.uint8, device="cuda", generator=g)
    t[0] = 4
    t[-1] = 4
    t[n // 3] = 4
    return t


def sampled(host, rng, count, L=20, nsub=0):
    out = []
    while len(out) < count:
        a = int(rng.integers(1, host.size - L - 1))
        w = host[a:a + L].copy()
        if (w > 3).any():
            continue
        for i in rng.choice(L, size=nsub, replace=False):
            w[i] = (w[i] + 1 + int(rng.integers(0, 3))) % 4
        out.append(LUT[w].tobytes().decode())
    return out


def primers(host, rng, n_planted, n_random, L=20):
    pats = [p for d in range(3) for p in sampled(host, rng, n_planted, L, d)]
    pats += ["".join("ACGT"[c] for c in rng.integers(0, 4, L)) for _ in range(n_random)]
    return pats + [sat_amd.reverse_comp(p) for p in pats]


def handle(monkeypatch, schedule, pats, k, indels=False):
    """a handle created with PM_PAIR_MAP=schedule (the library reads its knobs once, in pm_create)"""
    monkeypatch.setenv("PM_PAIR_MAP", schedule)
    pm = sat_amd.PatternMatch(k=k, indels=indels, kernel=sat_amd.KERNEL_SEED)
    monkeypatch.delenv("PM_PAIR_MAP")
    for i, p in enumerate(pats):
        pm.add_pattern(p, i + 1)
    return pm


def canon(recs):
    """records as (n, 2) int64 rows in sorted order: every byte of every record takes part"""
    r = np.ascontiguousarray(recs).view(np.int64).reshape(-1, 2)
    return r[np.lexsort((r[:, 1], r[:, 0]))]


def same(a, b):
    return a.shape == b.shape and bool((a == b).all())


@pytest.mark.parametrize("k", [1, 2])
def test_uniform_256mbp(monkeypatch, k):
    """-K 1 and -K 2 over 256 Mbp of uniform text, 20k primers x 2 strands, a tenth of them cut from the stream: the whole
    range in one launch, and three ranges of it"""
    n = 1 << 28
    dev = random_db(n, 31 + k)
    rng = np.random.default_rng(31 + k)
    pats = primers(dev[: 1 << 24].cpu().numpy(), rng, 700, 17_900)
    got = {}
    for m in MAPS:
        pm = handle(monkeypatch, m, pats, k)
        pm.init_device(dev.data_ptr(), dev.numel(), TABLE, keepalive=dev)
        pm.set_capacity(1 << 23)
        whole = canon(pm.scan_candidates(0, n))
        assert "pm_pair_scan" in pm.describe() and "schedule=%s" % m in pm.describe().split(), pm.describe()
        cuts = [0, (1 << 26) + 4097, n - (3 << 20) - 11, n]
        parts = canon(np.concatenate([pm.scan_candidates(cuts[i], cuts[i + 1]) for i in range(3)]))
        assert same(whole, parts), (m, whole.shape, parts.shape)
        got[m] = whole
        pm.close()
    assert got["superchunk"].shape[0] > 1000
    for m in MAPS[1:]:
        assert same(got[m], got["superchunk"]), (m, got[m].shape, got["superchunk"].shape)


def test_default_schedule_by_range_size(monkeypatch):
    """ranges of >= 1280 chunks take the XCD superchunk map, smaller ones the superchunk map"""
    n = 1 << 28
    dev = random_db(n, 3)
    rng = np.random.default_rng(3)
    pats = primers(dev[: 1 << 24].cpu().numpy(), rng, 100, 2000)
    pm = handle(monkeypatch, "", pats, 1)
    pm.init_device(dev.data_ptr(), dev.numel(), TABLE, keepalive=dev)
    pm.set_capacity(1 << 22)
    pm.scan_candidates(0, n)
    assert "schedule=superchunk" in pm.describe().split(), pm.describe()      # 489 chunks of 512 Ki
    pm.close()
    monkeypatch.setenv("PM_SEED_CHUNK", "131072")                     # 2048 chunks of 128 Ki
    pm = handle(monkeypatch, "", pats, 1)
    monkeypatch.delenv("PM_SEED_CHUNK")
    pm.init_device(dev.data_ptr(), dev.numel(), TABLE, keepalive=dev)
    pm.set_capacity(1 << 22)
    a = canon(pm.scan_candidates(0, n))
    assert "schedule=xcd-superchunk" in pm.describe().split() and "nchunks=2048" in pm.describe(), pm.describe()
    pm.close()
    monkeypatch.setenv("PM_SEED_CHUNK", "131072")
    pm = handle(monkeypatch, "superchunk", pats, 1)
    monkeypatch.delenv("PM_SEED_CHUNK")
    pm.init_device(dev.data_ptr(), dev.numel(), TABLE, keepalive=dev)
    pm.set_capacity(1 << 22)
    b = canon(pm.scan_candidates(0, n))
    pm.close()
    assert a.shape[0] > 200 and same(a, b)


def test_skewed_stream_hit_dense(monkeypatch):
    """-K 2 over 30 Mbp of skewed composition (A .55 C .05 G .05 T .35) with 3000 primers cut from it: key hits and
    suspects many times those of uniform text"""
    rng = np.random.default_rng(77)
    s = A.make_stream(rng, 30_000_000, 1)
    pats = A.make_patterns(rng, s[: 1 << 22], 3000, 20, 24, 2)
    pats = pats + [sat_amd.reverse_comp(p) for p in pats]
    dev = torch.from_numpy(s).to("cuda")
    got = {}
    for m in MAPS:
        pm = handle(monkeypatch, m, pats, 2)
        pm.init_device(dev.data_ptr(), dev.numel(), TABLE, keepalive=dev)
        pm.set_capacity(1 << 25)
        got[m] = canon(pm.scan_candidates(0, s.size))
        assert "pm_pair_scan" in pm.describe() and "schedule=%s" % m in pm.describe().split(), pm.describe()
        pm.close()
    assert got["superchunk"].shape[0] > 3000, got["superchunk"].shape
    for m in MAPS[1:]:
        assert same(got[m], got["superchunk"]), m


def test_edit_plan_k2(monkeypatch):
    """-k 2 (edits) on the pair geometry, pm_pair_edit_scan's 14 tests: final hits over 64 Mbp"""
    n = 1 << 26
    dev = random_db(n, 41)
    rng = np.random.default_rng(41)
    pats = primers(dev[: 1 << 24].cpu().numpy(), rng, 300, 9000)
    got = {}
    for m in MAPS:
        pm = handle(monkeypatch, m, pats, 2, indels=True)
        pm.init_device(dev.data_ptr(), dev.numel(), TABLE, keepalive=dev)
        pm.set_capacity(1 << 24)
        got[m] = canon(pm.find_all())
        assert "pm_pair_edit_scan" in pm.describe() and "schedule=%s" % m in pm.describe().split(), pm.describe()
        pm.close()
    assert got["superchunk"].shape[0] > 900
    for m in MAPS[1:]:
        assert same(got[m], got["superchunk"]), m


@pytest.mark.parametrize("k", [1, 2])
def test_small_pm_scan_ranges(monkeypatch, k):
    """pm_scan in ranges of a few chunks or less (odd lengths), records drained in small batches"""
    n = 24_000_017
    dev = random_db(n, 51 + k)
    rng = np.random.default_rng(51 + k)
    pats = primers(dev[: 1 << 23].cpu().numpy(), rng, 200, 3000)
    got = {}
    for m in MAPS:
        pm = handle(monkeypatch, m, pats, k)
        pm.init_device(dev.data_ptr(), dev.numel(), TABLE, keepalive=dev)
        got[m] = [canon(pm.find_all(chunk=c)) for c in (1_000_003, 4_194_304 + 17)]
        pm.close()
    for m in MAPS[1:]:
        for a, b in zip(got[m], got["superchunk"]):
            assert a.shape[0] > 300 and same(a, b), m
    assert same(got["superchunk"][0], got["superchunk"][1])


def test_windowed_handle(monkeypatch):
    """a windowed handle (stream in host memory, 4 MiB windows in HBM) over 40 Mbp at -K 2"""
    n, window = 40_000_000, 4 << 20
    host = random_db(n, 61).cpu().numpy()
    rng = np.random.default_rng(61)
    pats = primers(host[: 1 << 23], rng, 200, 3000)
    got = {}
    for m in MAPS:
        pm = handle(monkeypatch, m, pats, 2)
        pm.init(host, TABLE, window=window)
        got[m] = canon(pm.find_all(chunk=1 << 30))
        res = pm.residency()
        pm.close()
        assert res["window"] == window and res["loads"] > 1, res
    assert got["superchunk"].shape[0] > 300
    for m in MAPS[1:]:
        assert same(got[m], got["superchunk"]), m
