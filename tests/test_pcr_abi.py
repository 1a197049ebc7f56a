"""CPU: the pm_pcr_* part of the C ABI -- the record layouts on both sides of ctypes and the argument checks of
pm_pcr_setup that need no GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sat_amd
from sat_amd import pattern_match as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PM_E_INVALID = -1


def test_struct_sizes():
    # pm_pcr_amplicon: 2 x pm_hit (16) + 2 x pm_alignment (24) + int64 + 2 x uint32
    assert P.PCR_AMPLICON_DTYPE.itemsize == 96
    assert P.PCR_AMPLICON_DTYPE.fields["al"][1] == 32 and P.PCR_AMPLICON_DTYPE.fields["amplicon_len"][1] == 80
    assert P.PCR_AMPLICON_DTYPE.fields["pair"][1] == 88 and P.PCR_AMPLICON_DTYPE.fields["ncount"][1] == 92
    # pm_pcr_params: 2 x int32, 2 x int64, 2 x int32, 3 pointers, int64
    assert C.sizeof(P._PcrParams) == 64
    assert P._PcrParams.amplicon_min.offset == 8 and P._PcrParams.size_slack.offset == 24 and P._PcrParams.size_lb.offset == 32
    assert P._PcrParams.n_entries.offset == 56
    with open(os.path.join(ROOT, "include", "pm_gpu.h")) as f:
        src = f.read()
    m = re.search(r"typedef struct \{([^}]*)\} pm_pcr_amplicon;", src)
    assert m and [t.split()[-1] for t in m.group(1).split(";") if t.strip()] == ["hit[2]", "al[2]", "amplicon_len", "pair", "ncount"]
    m = re.search(r"typedef struct \{([^}]*)\} pm_pcr_params;", src)
    names = [re.sub(r"/\*.*?\*/", "", t, flags=re.S).split()[-1].lstrip("*") for t in m.group(1).split(";") if re.sub(r"/\*.*?\*/", "", t, flags=re.S).strip()]
    assert names == ["any_orientation", "length_between", "amplicon_min", "amplicon_max", "size_slack", "reserved", "size_ub", "entry_starts", "n_entries"]


def test_struct_sizes_in_c(tmp_path):
    """the other side of ctypes: sizeof and offsetof as a C++ compiler sees include/pm_gpu.h"""
    cxx = next((p for p in map(shutil.which, ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++")) if p), None)
    assert cxx, "no C++ compiler for the layout program"
    src = tmp_path / "layout.cc"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "pm_gpu.h"\n'
                   'int main() { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(pm_pcr_amplicon), offsetof(pm_pcr_amplicon, al), offsetof(pm_pcr_amplicon, amplicon_len),\n'
                   '  offsetof(pm_pcr_amplicon, ncount), sizeof(pm_pcr_params), offsetof(pm_pcr_params, amplicon_min), offsetof(pm_pcr_params, size_lb), offsetof(pm_pcr_params, n_entries)); }\n')
    subprocess.check_call([cxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")])
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, timeout=60).stdout.split()
    t, q = P.PCR_AMPLICON_DTYPE, P._PcrParams
    assert [int(x) for x in out] == [t.itemsize, t.fields["al"][1], t.fields["amplicon_len"][1], t.fields["ncount"][1],
                                     C.sizeof(q), q.amplicon_min.offset, q.size_lb.offset, q.n_entries.offset]


def handle(patterns, ids=None):
    pm = sat_amd.PatternMatch(k=1)
    for i, p in enumerate(patterns):
        pm.add_pattern(p, (i + 1) if ids is None else ids[i])
    return pm


def setup_error(pm, **kw):
    with pytest.raises(sat_amd.PmError) as e:
        pm.pcr_setup(**kw)
    return e.value.code, str(e.value)


PRIMERS = ["ACGTACGTACGTACGTAAAA", "TTGACATTGACATTGACAGG", "TTTTACGTACGTACGTACGT", "CCTGTCAATGTCAATGTCAA"]


def test_setup_before_init_is_invalid():
    code, msg = setup_error(handle(PRIMERS))
    assert code == PM_E_INVALID and "not initialised" in msg


def test_setup_with_an_odd_pattern_count_is_invalid():
    for pats in (PRIMERS[:3], PRIMERS[:2], []):                       # (2n patterns with n odd: no reverse complements)
        code, msg = setup_error(handle(pats))
        assert code == PM_E_INVALID and "2n patterns with n even" in msg


def test_setup_with_ids_out_of_order_is_invalid():
    for ids in ([1, 3, 2, 4], [2, 3, 4, 5], [1, 2, 3, 3]):
        code, msg = setup_error(handle(PRIMERS, ids=ids))
        assert code == PM_E_INVALID and "ids 1..2n in order" in msg


def test_setup_with_a_negative_amplicon_min_is_invalid():
    code, msg = setup_error(handle(PRIMERS), amplicon_min=-1)
    assert code == PM_E_INVALID and "amplicon_min" in msg


def test_feed_and_pair_need_a_setup():
    pm = handle(PRIMERS)
    with pytest.raises(sat_amd.PmError) as e:
        pm.pcr_feed(np.zeros(1, dtype=sat_amd.HIT_DTYPE))
    assert e.value.code == PM_E_INVALID
    with pytest.raises(sat_amd.PmError) as e:
        pm.pcr_pair(0, False)
    assert e.value.code == PM_E_INVALID
