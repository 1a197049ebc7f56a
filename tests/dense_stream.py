"""The hit-dense stream of tests/test_gpu_scan_lookahead.py and the closed form of its hit lists.

Stream: "AC" * (N / 2), normalized with the table b"ACGT\\n"; patterns "AC" * 10 and "CA" * 10.  Away from its two ends the
stream has period 2, so the hit list of an engine that reports every window on its own (no clustering) has period 2 as well:
expected(N) = the oracle's hits at N = 4,096 cut into head (end <= 64), one period (64 < end <= 66) repeated, and tail (the
last 64 ends, moved).  tests/test_dense_closed_form.py pins it to the oracle on the CPU; the GPU tests use it at sizes where
the oracle's lists would be too slow to build and compare."""
import numpy as np

import sat_amd
from oracle import pmoracle as O

TABLE = b"ACGT\n"
PATTERNS = ["AC" * 10, "CA" * 10]
N0, EDGE = 4096, 64
IDS = [(1, 2), (2, 1), (7, 7)]

# name -> (PatternMatch arguments, oracle engine (None: the automatic choice), exact_start_bases of both patterns)
OPTION_SETS = {
    "k0": (dict(k=0, indels=True), None, 0),
    "inexact_K1": (dict(k=1, indels=False, semantics=sat_amd.SEM_SHIFT_AND_INEXACT), O.SHIFT_AND_INEXACT, 0),
    "inexact_k1": (dict(k=1, indels=True, semantics=sat_amd.SEM_SHIFT_AND_INEXACT), O.SHIFT_AND_INEXACT, 0),
    "bases_K1": (dict(k=1, indels=False, semantics=sat_amd.SEM_EXACT_BASES, kernel=sat_amd.KERNEL_SEED), O.EXACT_BASES_KT, 4),
}

_BASE = {}


def codes(n):
    assert n % 2 == 0
    return np.tile(np.array([0, 1], dtype=np.uint8), n // 2)


def oracle_hits(name, ids, n):
    """the oracle's hits on the stream of n characters: (end, pid, k) as three arrays, in (end, pid, k) order"""
    kw, eng, zone = OPTION_SETS[name]
    text = O.Text(codes(n), TABLE)
    if eng is None:
        eng = O.pick_engine(text, PATTERNS, kw["k"], kw["indels"])
    z = [zone] * len(PATTERNS) if zone else None
    h = O.find_all(text, PATTERNS, engine=eng, k=kw["k"], indels=kw["indels"], ids=list(ids), esb=z)
    end, pid, k = h["end"].astype(np.int64), h["pid"].astype(np.int64), h["k"].astype(np.int64)
    o = np.lexsort((k, pid, end))
    return end[o], pid[o], k[o]


def expected(name, ids, n):
    """closed form of oracle_hits(name, ids, n) for even n >= N0"""
    key = (name, tuple(ids))
    if key not in _BASE:
        _BASE[key] = oracle_hits(name, ids, N0)
    return extend(_BASE[key], n)


def extend(base, n):
    """a list (end, pid, k) of the stream of N0 characters, in (end, pid, k) order and of period 2 between its edges, on the
    stream of n characters (even, >= N0): head, one period repeated, tail"""
    assert n % 2 == 0 and n >= N0
    end, pid, k = base
    head, unit, tail = end <= EDGE, (end > EDGE) & (end <= EDGE + 2), end > N0 - EDGE
    periods = (n - 2 * EDGE) // 2
    shift = 2 * np.arange(periods, dtype=np.int64)[:, None]
    rep = lambda a: np.broadcast_to(a[unit][None, :], (periods, int(unit.sum()))).ravel()
    return (np.concatenate([end[head], (end[unit][None, :] + shift).ravel(), end[tail] + (n - N0)]),
            np.concatenate([pid[head], rep(pid), pid[tail]]),
            np.concatenate([k[head], rep(k), k[tail]]))
