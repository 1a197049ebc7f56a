#!/usr/bin/env python3
"""Which (field pair, displacement) tests would an edit-distance plan on the PAIR geometry need?  

The last 20 pattern bases are four fields of five.  A text within <= k edits (substitution, insertion, deletion) of
the pattern leaves >= 2 fields clean for k = 2; two clean fields A < B appear in the text displaced by d = net
insertions between them.  A test (A, B, d) -- "field A here and field B 5 (B - A) + d bases further on are the pattern's" --
finds the alignment.  This script enumerates every placement of <= k edits, reduces it to its set of clean pairs with
their displacements, and computes the exact minimum set of tests that hits every scenario (brute force over subsets).

    python scripts/edit_pair_cover.py        ->  k = 1: 2 tests, k = 2: 14 tests

With a field width as its argument the same enumeration runs for fields of that many bases: width 4 is the geometry of
pm_short_edit_scan (the last 16 bases of a 16..19 character pattern), whose minimum cover is the same
list of tests.

    python scripts/edit_pair_cover.py 4
"""
import itertools
import sys

F, L = 4, 5


def all_edits(L):
    return [("s", i) for i in range(F * L)] + [("d", i) for i in range(F * L)] + [("i", i) for i in range(F * L + 1)]


EDITS = all_edits(L)


def scenario(edits, L=L):
    """clean field pairs (a, b, displacement) of the pattern after `edits` (sub at base i / delete base i / insert before base i)"""
    dirty, events = set(), []
    for kind, i in edits:
        if kind == "s":
            dirty.add(i // L)
        elif kind == "d":
            dirty.add(i // L)
            events.append((i + 1, -1))          # every base behind the deleted one moves up
        else:
            if i % L:
                dirty.add(i // L)                # an insertion inside a field splits it; at a field boundary it only shifts
            events.append((i, +1))
    clean = [f for f in range(F) if f not in dirty]
    shift = lambda f: sum(d for pos, d in events if pos <= f * L)
    return frozenset((a, b, shift(b) - shift(a)) for a, b in itertools.combinations(clean, 2))


def min_cover(k, L=L):
    scen = {scenario(es, L) for n in range(k + 1) for es in itertools.combinations_with_replacement(all_edits(L), n)}
    assert all(scen), "a placement without a clean pair"
    tests = sorted(set().union(*scen))
    forced = set().union(*(x for x in scen if len(x) == 1))      # a scenario with one clean pair: its test is in every cover
    left = [x for x in scen if not x & forced]
    free = [t for t in tests if t not in forced]
    for r in range(len(free) + 1):
        for sub in itertools.combinations(free, r):
            s = set(sub)
            if all(x & s for x in left):
                return len(scen), tests, tuple(sorted(forced | s))
    raise AssertionError


if __name__ == "__main__":
    width = int(sys.argv[1]) if len(sys.argv) > 1 else L
    for k in (1, 2):
        n, tests, cover = min_cover(k, width)
        print("k = %d: %d distinct scenarios, %d tests can occur, minimum cover %d: %s" % (k, n, len(tests), len(cover), list(cover)))
