"""CPU: csrc/pm_pcr.h -- the pairing rule as the kernels of pm_pcr.hip compile it -- against tests/pcr_rule.py.

A stand-alone C++ program includes the header, reads random rounds (options, pattern lengths, UniSTS bounds, entry starts,
hits with made-up re-alignments), applies partners / stretch / deferred / survives / pind pair by pair and prints the
candidate and the surviving pairs; they must equal pcr_rule.py's.  The program is built with
-fsanitize=address,undefined -fno-sanitize-recover=undefined and run as a program of its own.  The rounds include
size_lb < size_slack (the wrap of the UniSTS clamp), -b and -a, hits of one pair that overlap each other, and a later hit
that is processed while an earlier partner is deferred (the pair comes out in swapped order)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcr_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "sequence-alignment-tools_amd", "csrc")
NROUNDS = 240

HARNESS = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pm_pcr.h"

struct Hit { long long key; unsigned long long id; long long start, end; int ed; };

int main() {
  int rounds = 0;
  if (scanf("%d", &rounds) != 1) return 2;
  for (int r = 0; r < rounds; ++r) {
    pm::pcr::Rule rule;
    unsigned long long n; long long amin, amax, scanned_to; int any, between, d, has_sizes, k, slack, more, nhits, nentries;
    if (scanf("%llu %d %d %lld %lld %d %d %d %d %lld %d %d %d", &n, &any, &between, &amin, &amax, &d, &has_sizes, &k, &slack, &scanned_to, &more, &nhits, &nentries) != 13) return 2;
    rule.n = n; rule.any_orientation = any; rule.length_between = between; rule.amplicon_min = amin; rule.amplicon_max = amax;
    rule.size_slack = d; rule.has_sizes = has_sizes; rule.k = k; rule.slack = slack;
    // heap blocks of exactly the sizes the rule may index
    std::vector<int32_t> patlen(2 * n + 1, 0);
    for (size_t i = 1; i <= 2 * n; ++i) if (scanf("%d", &patlen[i]) != 1) return 2;
    std::vector<uint64_t> lb(n / 2), ub(n / 2);
    if (has_sizes) for (size_t i = 0; i < n / 2; ++i) { unsigned long long a, b; if (scanf("%llu %llu", &a, &b) != 2) return 2; lb[i] = a; ub[i] = b; }
    std::vector<int64_t> starts(nentries);
    for (int i = 0; i < nentries; ++i) { long long v; if (scanf("%lld", &v) != 1) return 2; starts[i] = v; }
    std::vector<Hit> l(nhits);
    for (Hit &h : l) if (scanf("%lld %llu %lld %lld %d", &h.key, &h.id, &h.start, &h.end, &h.ed) != 5) return 2;
    std::sort(l.begin(), l.end(), [](const Hit &a, const Hit &b) { return a.key != b.key ? a.key < b.key : a.id < b.id; });
    std::vector<int64_t> smin(nhits), smax(nhits);
    std::vector<char> def(nhits);
    for (int i = 0; i < nhits; ++i) {
      const uint64_t pr = pm::pcr::pair_of(rule, l[i].id);
      pm::pcr::stretch(rule, l[i].id, l[i].key, patlen.data(), has_sizes ? lb[pr - 1] : 0, has_sizes ? ub[pr - 1] : 0, &smin[i], &smax[i]);
      def[i] = pm::pcr::deferred(scanned_to, more, smax[i]);
    }
    printf("R %d\n", r);
    for (int i = 0; i < nhits; ++i) {
      if (def[i]) continue;
      uint64_t p[2];
      pm::pcr::partners(rule, l[i].id, &p[0], &p[1]);
      for (int t = 0; t < 2; ++t) {
        if (!p[t]) continue;
        for (int j = 0; j < nhits; ++j) {
          if (l[j].id != p[t] || l[j].key < smin[i] || l[j].key > smax[i] || !(j > i || def[j])) continue;
          printf("C %d %d\n", i, j);
          const uint64_t pi = pm::pcr::pind(rule, l[i].id, l[j].id);
          int64_t alen = 0;
          if (pm::pcr::survives(rule, l[i].start, l[i].end, l[i].ed, l[j].start, l[j].end, l[j].ed, starts.data(), nentries,
                                has_sizes ? lb[pi - 1] : 0, has_sizes ? ub[pi - 1] : 0, &alen))
            printf("S %d %d %lld %llu\n", i, j, (long long)alen, (unsigned long long)pi);
        }
      }
    }
    for (int i = 0; i < nhits; ++i) if (def[i]) printf("D %d\n", i);
  }
  return 0;
}
"""


def compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    pytest.fail("no C++ compiler for the rule harness")


def make_round(rng, r):
    n = 2 * int(rng.integers(1, 4))
    patlen = [0] + [int(rng.integers(5, 30)) for _ in range(2 * n)]
    if r % 3 == 2:
        # partners of very different lengths: the short one's window reaches further, so it is still deferred when the
        # long one behind it is processed -- the pair comes out in swapped order
        patlen = [0] + [int(rng.integers(5, 8)) if i % 2 else int(rng.integers(26, 30)) for i in range(2 * n)]
    slack_d = int(rng.integers(-1, 60))
    sizes = None
    if r % 2 == 0:
        # bounds below -d among them: size_lb - size_slack wraps
        sizes = [(int(rng.integers(0, 90)), int(rng.integers(0, 140))) for _ in range(n // 2)]
    k = int(rng.integers(0, 3))
    indels = bool(rng.integers(0, 2))
    rule = R.Rule(n, patlen, k, indels, any_orientation=r % 3 == 0, length_between=r % 4 == 1, amplicon_min=int(rng.integers(0, 30)),
                  amplicon_max=int(rng.integers(20, 160)), size_slack=slack_d, sizes=sizes)
    nstream = 500
    starts = sorted({1} | {int(rng.integers(1, nstream)) for _ in range(int(rng.integers(0, 3)))})
    scanned_to, more = [(nstream, 0), (nstream, 1), (int(rng.integers(50, nstream)), 1)][r % 3]
    lo, hi = 1, nstream
    if r % 3 == 2:                                      # ... with the hits where windows end around scanned_to
        lo = max(1, scanned_to - rule.amplicon_max - 40)
        hi = min(nstream, lo + 80)
    keys = {}
    for _ in range(int(rng.integers(0, 150))):
        # dense ends: hits of the two primers of a pair overlap each other
        key, pid = int(rng.integers(lo, hi)), int(rng.integers(1, 2 * n + 1))
        L = patlen[pid] + int(rng.integers(-1, 2))
        keys[(key, pid)] = (key - L, key - 1, int(rng.integers(0, k + 2)) if rng.random() < 0.9 else 2 ** 31 - 1)
    hits = [(key, pid) + al for (key, pid), al in sorted(keys.items())]
    return rule, starts, hits, scanned_to, more


def want_lines(r, rule, starts, hits, scanned_to, more, seen):
    l, pairs, carried = R.candidates(rule, [(h[0], h[1], 0) for h in hits], scanned_to, more)
    al = {(h[0], h[1]): h[2:] for h in hits}
    out = ["R %d" % r]
    pos = {h: i for i, h in enumerate(l)}
    for i, j in pairs:
        out.append("C %d %d" % (i, j))
        ok, alen, pi = R.survives(rule, al[l[i][:2]], al[l[j][:2]], l[i][1], l[j][1], starts)
        if ok:
            out.append("S %d %d %d %d" % (i, j, alen, pi))
            seen["survivors"] += 1
        if j < i:
            seen["swapped"] += 1
        if abs(l[i][0] - l[j][0]) < min(rule.patlen[l[i][1]], rule.patlen[l[j][1]]):
            seen["overlap"] += 1
    if rule.sizes is not None and rule.size_slack >= 0 and any(lb < rule.size_slack for lb, _ in rule.sizes):
        seen["wrap"] += 1
    seen["pairs"] += len(pairs)
    seen["deferred"] += len(carried)
    out += ["D %d" % pos[h] for h in carried]
    return out


def test_header_equals_the_python_rule(tmp_path):
    rng = np.random.default_rng(2024)
    seen = dict(pairs=0, survivors=0, swapped=0, overlap=0, wrap=0, deferred=0)
    text, want = ["%d" % NROUNDS], []
    for r in range(NROUNDS):
        rule, starts, hits, scanned_to, more = make_round(rng, r)
        text.append("%d %d %d %d %d %d %d %d %d %d %d %d %d" % (rule.n, rule.any_orientation, rule.length_between, rule.amplicon_min, rule.amplicon_max,
                                                               rule.size_slack, rule.sizes is not None, rule.k, rule.slack, scanned_to, more, len(hits), len(starts)))
        text.append(" ".join(map(str, rule.patlen[1:])))
        if rule.sizes is not None:
            text.append(" ".join("%d %d" % s for s in rule.sizes))
        text.append(" ".join(map(str, starts)))
        text += ["%d %d %d %d %d" % h for h in hits]
        want += want_lines(r, rule, starts, hits, scanned_to, more, seen)
    # the cases the test is about were reached
    assert seen["pairs"] > 2000 and seen["survivors"] > 100 and seen["swapped"] > 20 and seen["overlap"] > 100, seen
    assert seen["wrap"] > 20 and seen["deferred"] > 500, seen
    src = tmp_path / "pcr_rule_check.cc"
    src.write_text(HARNESS)
    exe = tmp_path / "pcr_rule_check"
    subprocess.check_call([compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", HEADER_DIR, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    assert got == want
