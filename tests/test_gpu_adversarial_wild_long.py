"""GPU against the ORACLE on the -w cases of the class-mixing adversarial generator (tests/adversarial_classes.py, the fixed
seeds of tests/test_gpu_adversarial_classes.py) with PM_WILD_LONG beside the case's own permission bits: where all seven
bits were on, pm_config.long_patterns is 255.  The degenerate primers of 33..64 nt of those lists -- residue primers there --
then join the class of pm_wild_sub_scan beside narrow and wide main-class tiles, the 16..19 nt classes and the residue,
in one record buffer with the case's knobs, record caps and ways through the library."""
import pytest

import adversarial as A
import adversarial_classes as AC
import sat_amd
from test_gpu_adversarial_classes import SEEDS, case, differ

WIDE_CLASS = "pm_wild_sub_verify_wide"
WILD_SEEDS = [s for s in SEEDS if AC.class_case(s)["wild"]]
NAMED = {}


def test_the_generator_gives_long_degenerate_primers():
    """(CPU) a third of the fixed seeds are -w cases, and at least 40 of them hold a degenerate primer of 33..64 nt beside
    the wild_class bit"""
    assert len(WILD_SEEDS) >= len(SEEDS) // 4
    held = 0
    for s in WILD_SEEDS:
        c = AC.class_case(s)
        held += c["route"]["wild_class"] and any(AC.kind(p) == "degenerate" and 33 <= len(p) <= 64 for p in c["patterns"])
    assert held >= 40, held


@pytest.mark.gpu
@pytest.mark.parametrize("seed", WILD_SEEDS)
def test_class_case_with_bit_seven_vs_oracle(seed):
    c, want = case(seed)
    route = dict(c["route"], wild_long=True)
    try:
        got = A.gpu_hits(c, kernel=sat_amd.KERNEL_AUTO, route=route)
    except sat_amd.PmError as e:
        if want is None and e.code in (-6, -2):
            return                                                    # the reference rejects this option set too
        if e.code != -2 or c["mode"] < 2:
            raise
        got = A.gpu_hits(c, kernel=sat_amd.KERNEL_AUTO, mode=1, route=route)   # (the mode does not take the option set: the resumable scan)
    assert want is not None, ("the oracle rejects what the library accepts", AC.describe(c))
    NAMED[seed] = WIDE_CLASS in c["kernel_desc"]
    assert got == want, differ(c, got, want, " +wild_long")


@pytest.mark.gpu
def test_the_wide_class_did_run():
    """at least 10 handles named the wide class verify, as the sibling file asks of every route (the cases run before this
    test in file order; alone, it runs them itself)"""
    for seed in WILD_SEEDS:
        if seed not in NAMED:
            test_class_case_with_bit_seven_vs_oracle(seed)
    assert sum(NAMED.values()) >= 10, sum(NAMED.values())
