"""The minimum set of (field pair, displacement) tests of the edit plan's first stages, recomputed by
scripts/edit_pair_cover.py for fields of four bases (pm_short_edit_scan, csrc/pm_short.hip) and of five (pm_pair_edit_scan):
the kernels' test tables are these lists."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K2 = [(0, 1, 0), (0, 2, -1), (0, 2, 0), (0, 2, 1), (0, 3, -2), (0, 3, -1), (0, 3, 0), (0, 3, 1), (0, 3, 2), (1, 2, 0), (1, 3, -1), (1, 3, 0), (1, 3, 1), (2, 3, 0)]
K1 = [(0, 1, 0), (2, 3, 0)]


def cover_module():
    spec = importlib.util.spec_from_file_location("edit_pair_cover", os.path.join(ROOT, "scripts", "edit_pair_cover.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cover_with_fields_of_four_bases():
    m = cover_module()
    assert list(m.min_cover(2, 4)[2]) == K2
    assert list(m.min_cover(1, 4)[2]) == K1


def test_cover_with_fields_of_five_bases_is_unchanged():
    m = cover_module()
    assert m.min_cover(2)[:1] == (46,) and list(m.min_cover(2)[2]) == K2
    assert m.min_cover(1)[:1] == (12,) and list(m.min_cover(1)[2]) == K1


def test_the_cover_is_a_cover():
    """every placement of <= k edits on sixteen bases leaves one of the tests' field pairs clean at the test's displacement"""
    import itertools
    m = cover_module()
    for k, tests in ((1, K1), (2, K2)):
        for n in range(k + 1):
            for es in itertools.combinations_with_replacement(m.all_edits(4), n):
                assert m.scenario(es, 4) & set(tests), es
