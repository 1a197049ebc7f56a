"""CPU: the closed form of the dense stream's hit lists (tests/dense_stream.py) against the oracle.  The GPU tests of
pm_scan's look-ahead (tests/test_gpu_scan_lookahead.py) compare against that closed form at sizes of 10^6..10^7 hits."""
import numpy as np
import pytest

import dense_stream as D


@pytest.mark.parametrize("ids", D.IDS, ids=lambda t: "ids%d_%d" % t)
@pytest.mark.parametrize("name", list(D.OPTION_SETS))
def test_dense_stream_closed_form_is_the_oracle(name, ids):
    end, pid, k = D.oracle_hits(name, ids, D.N0)
    body = (end > D.EDGE) & (end <= D.N0 - D.EDGE)
    assert body.sum() >= (D.N0 - 2 * D.EDGE) // 2, (name, ids, int(body.sum()))          # dense: a hit at every other end at least
    # period 2: the body moved by two characters is the body again
    a = (end > D.EDGE) & (end <= D.N0 - D.EDGE - 2)
    b = (end > D.EDGE + 2) & (end <= D.N0 - D.EDGE)
    assert a.sum() == b.sum() and a.sum() > 0
    assert np.array_equal(end[a] + 2, end[b]) and np.array_equal(pid[a], pid[b]) and np.array_equal(k[a], k[b]), (name, ids)
    for n in (4096, 6002):
        want = D.oracle_hits(name, ids, n)
        got = D.expected(name, ids, n)
        for w, g, field in zip(want, got, ("end", "pid", "k")):
            assert np.array_equal(w, g), (name, ids, n, field, w.size, g.size)
