"""CPU: the PM_WILD_LONG permission (bit 7 of pm_config.long_patterns, include/pm_gpu.h) at the C ABI and in
the Python wrapper: the header defines it as 128, pm_create takes 128, 160 and 255, PatternMatch(wild_long=True) sets that
bit and no other, and every older keyword keeps its bit with and without the new one beside it."""
import ctypes as C
import os
import re

import sat_amd
from sat_amd import pattern_match as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OLDER = ("long_patterns", "long_exact", "long_edits", "long_halves", "long_align", "wild_class", "edit_pair")


def create(value):
    L = P.load_library()
    cfg = P._Config()
    cfg.abi_version, cfg.semantics, cfg.kernel, cfg.k, cfg.indels, cfg.eos = 1, sat_amd.SEM_AUTO, sat_amd.KERNEL_AUTO, 1, 0, ord("\n")
    cfg.wildcards = 1
    cfg.long_patterns = value
    h = C.c_void_p()
    rc = L.pm_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        L.pm_destroy(h)
    return rc


def test_the_header_names_bit_seven():
    with open(os.path.join(ROOT, "include", "pm_gpu.h")) as f:
        src = f.read()
    found = re.findall(r"#define\s+PM_WILD_LONG\s+(\d+)", src)
    assert found == ["128"], found
    # one value per permission: no other define of the field's bits has taken 128
    others = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(PM_(?:LONG_[A-Z]+|WILD_CLASS|EDIT_PAIR))\s+(\d+)", src)}
    assert sorted(others.values()) == [1, 2, 4, 8, 16, 32, 64], others


def test_pm_create_takes_the_bit():
    for value in (128, 160, 255):
        assert create(value) == 0, value


def test_the_keyword_sets_bit_seven_and_no_other():
    pm = sat_amd.PatternMatch(k=1, indels=False, wildcards=True, wild_long=True)
    assert pm.long_patterns_bits == 128
    pm.close()
    pm = sat_amd.PatternMatch(k=1, indels=False, wildcards=True)
    assert pm.long_patterns_bits == 0
    pm.close()


def test_every_older_keyword_keeps_its_bit():
    for i, name in enumerate(OLDER):
        for extra in (False, True):
            pm = sat_amd.PatternMatch(k=1, **{name: True, "wild_long": extra})
            assert pm.long_patterns_bits == (1 << i) | (128 if extra else 0), (name, extra)
            pm.close()
    pm = sat_amd.PatternMatch(k=2, wild_long=True, **{name: True for name in OLDER})
    assert pm.long_patterns_bits == 255
    pm.close()
