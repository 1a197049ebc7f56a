"""CPU: the PM_EDIT_PAIR permission (bit 6 of pm_config.long_patterns, include/pm_gpu.h) at the C ABI and in the Python
wrapper: pm_create takes the value, PatternMatch(edit_pair=True) sets that bit and no other, and all seven bits go through."""
import ctypes as C
import os
import re

import sat_amd
from sat_amd import pattern_match as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("long_patterns", "long_exact", "long_edits", "long_halves", "long_align", "wild_class", "edit_pair")


def header_bits():
    with open(os.path.join(ROOT, "include", "pm_gpu.h")) as f:
        src = f.read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+(PM_(?:LONG_[A-Z]+|WILD_CLASS|EDIT_PAIR))\s+(\d+)", src)}


def create(value):
    L = P.load_library()
    cfg = P._Config()
    cfg.abi_version, cfg.semantics, cfg.kernel, cfg.k, cfg.indels, cfg.eos = 1, sat_amd.SEM_AUTO, sat_amd.KERNEL_AUTO, 1, 1, ord("\n")
    cfg.long_patterns = value
    h = C.c_void_p()
    rc = L.pm_create(C.byref(cfg), C.byref(h))
    if rc == 0:
        L.pm_destroy(h)
    return rc


def test_the_header_names_bit_six():
    bits = header_bits()
    assert bits["PM_EDIT_PAIR"] == 64
    assert sorted(bits.values()) == [1, 2, 4, 8, 16, 32, 64], bits


def test_pm_create_takes_the_bit():
    assert create(64) == 0
    assert create(127) == 0


def test_the_keyword_sets_bit_six_and_no_other():
    pm = sat_amd.PatternMatch(k=1, edit_pair=True)
    assert pm.long_patterns_bits == 64
    pm.close()
    pm = sat_amd.PatternMatch(k=1)
    assert pm.long_patterns_bits == 0
    pm.close()
    for i, name in enumerate(FLAGS):                                  # every keyword keeps its bit, with and without the new one beside it
        for extra in (False, True):
            pm = sat_amd.PatternMatch(k=1, **{name: True, "edit_pair": extra or name == "edit_pair"})
            assert pm.long_patterns_bits == (1 << i) | (64 if extra else 0) | (64 if name == "edit_pair" else 0), (name, extra)
            pm.close()


def test_all_seven_bits_round_trip():
    pm = sat_amd.PatternMatch(k=2, **{name: True for name in FLAGS})
    assert pm.long_patterns_bits == 127
    pm.close()
