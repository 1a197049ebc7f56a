"""CPU: tests/pcr_rule.py -- the pairing rule the pm_pcr_* kernels are held against -- pinned to the reference: on the
pcr_a / pcr_b cases recorded with the one-line format, hits from the oracle's engines and alignments from its
editdist_alignment, the rule must reproduce the recorded lines' %i, %>S %>E %<S %<E, %>d %<d, %l and %N as a multiset,
in one round and with the stream cut into rounds at every 500 positions.  The closed form of the join is also held
against the walk that zeroes keys, on random rounds."""
import numpy as np
import pytest

import pcr_cases as PC
import pcr_rule as R
from oracle import pmoracle as O


def oracle_hits(c):
    text = O.Text(c["codes"], c["table"])
    eng = O.pick_engine(text, c["patterns"], c["k"], c["indels"])
    h = O.find_all(text, c["patterns"], engine=eng, k=c["k"], indels=c["indels"], ids=list(range(1, len(c["patterns"]) + 1)))
    def align(hit):
        _, st, en, ed, _ = O.cli_align(text, c["patterns"][hit[1] - 1], hit[0], c["k"], c["indels"])
        return st, en, ed
    return O.sorted_tuples(h), align


@pytest.mark.parametrize("fixture", ["pcr_a", "pcr_b"])
@pytest.mark.parametrize("case", PC.ONELINE)
def test_rule_reproduces_the_reference(fixture, case):
    c = PC.setup(PC.load(fixture), case)
    hits, align = oracle_hits(c)
    assert c["want"], "the recorded case has no amplicons"
    sv, _, carried = R.round_survivors(c["rule"], hits, c["n_stream"], False, align, c["entry_starts"], c["chars"])
    assert carried == []
    assert sorted(PC.line_of(s) for s in sv) == c["want"]
    sv, log = PC.run_rounds(c["rule"], hits, c["n_stream"], 500, align, c["entry_starts"], c["chars"])
    assert len(log) > 3
    assert sorted(PC.line_of(s) for s in sv) == c["want"]


@pytest.mark.parametrize("seed", range(40))
def test_closed_form_equals_the_walk(seed):
    rng = np.random.default_rng(seed)
    n = 2 * int(rng.integers(1, 4))
    patlen = [0] + [int(rng.integers(5, 30)) for _ in range(2 * n)]
    sizes = None
    if rng.random() < 0.5:
        sizes = [(int(rng.integers(0, 80)), int(rng.integers(0, 120))) for _ in range(n // 2)]
    rule = R.Rule(n, patlen, int(rng.integers(0, 3)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)),
                  int(rng.integers(0, 30)), int(rng.integers(20, 150)), int(rng.integers(-1, 40)), sizes)
    hits = sorted({(int(rng.integers(1, 400)), int(rng.integers(1, 2 * n + 1)), 0) for _ in range(int(rng.integers(0, 120)))})
    for scanned_to, more in ((400, False), (400, True), (250, True), (100, True)):
        a = R.candidates(rule, hits, scanned_to, more)
        b = R.candidates_loop(rule, hits, scanned_to, more)
        assert a == b, (seed, scanned_to, more)
