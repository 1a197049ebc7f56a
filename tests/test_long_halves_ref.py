"""CPU: the oracle's exact_halves -k on primers of 33..64 characters against the real reference's engines
(tests/golden/long_halves_ref.json.gz, recorded from oracle/_ref/ref_harness by tests/golden/make_long_halves_golden.py).
The GPU tests of the halves plan's long route (tests/test_gpu_long_halves.py) take their expected values
from the oracle; this pins the oracle to the reference at these lengths before anything is compared with it."""
import gzip
import json
import os

import numpy as np
import pytest

import synth
from oracle import pmoracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "long_halves_ref.json.gz"), "rt") as f:
        return json.load(f)


def test_one_edit_texts_of_a_33_a_40_and_a_64_mer_under_k1_auto(golden):
    table = golden["table"].encode()
    assert [len(c["pattern"]) for c in golden["one_edit"]] == [33, 40, 64]
    for c in golden["one_edit"]:
        assert c["args"] == ["-k", "1"]
        text = O.Text(synth.normalize(c["stream"].encode(), table), table)
        eng = O.pick_engine(text, [c["pattern"]], 1, True)
        assert O.EXACT_HALVES_KT <= eng <= O.EXACT_HALVES_SA + 1, eng         # select.cc:121-126: exact_halves
        got = O.sorted_tuples(O.find_all(text, [c["pattern"]], engine=eng, k=1, indels=True))
        want = sorted(tuple(h) for h in c["hits"])
        assert got == want, (len(c["pattern"]), len(got), len(want))
        assert len(want) == c["texts"] > 3 * len(c["pattern"])                # one hit per text


def test_mixed_list_under_k2_exact_halves(golden):
    table = golden["table"].encode()
    c = golden["mixed"]
    assert c["args"] == ["-k", "2", "-N", "11"] and 4000 <= len(c["stream"]) <= 4100
    lens = {len(p) for p in c["patterns"]}
    assert lens >= {20, 32, 33, 34, 53, 63, 64} and max(lens) == 64
    text = O.Text(synth.normalize(c["stream"].encode(), table), table)
    want = sorted(tuple(h) for h in c["hits"])
    for eng in (O.EXACT_HALVES_KT, O.EXACT_HALVES_SA):
        got = O.sorted_tuples(O.find_all(text, c["patterns"], engine=eng, k=2, indels=True))
        assert got == want, (eng, len(got), len(want))
    hit_lens = {len(c["patterns"][pid - 1]) for _, pid, _ in want}
    assert any(n > 32 for n in hit_lens) and any(n <= 32 for n in hit_lens)
    assert any(v == 2 for _, pid, v in want if len(c["patterns"][pid - 1]) > 32)
