"""CPU: the key index of the kernels for patterns of 16..19 characters (csrc/pm_short_tables.h) against a plain restatement.

pm_short_edit_scan and pm_short_sub_scan build their tables with the same header this test compiles: per field pair of the
patterns' last 16 bases a bitmap of the 16-bit keys, an offset table, and the patterns sorted by key.  A small host program
builds the index for tails read from a file and prints it; the properties are checked here, on a few hundred random tails
with duplicates among them, for every field pair:
  * the offset table is non-decreasing, and pair c starts at c * m;
  * the run of key x holds exactly the patterns whose key is x, in increasing pattern index (the sort is stable);
  * a bitmap bit is set exactly where a run is not empty.
"""
import subprocess

import numpy as np

from test_short_sub_host import HEADER_DIR, compiler

PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pm_short_tables.h"

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int npairs = 0;
  if (fscanf(f, "%d", &npairs) != 1 || npairs < 1 || npairs > 6) return 2;
  int fa[6], fb[6];
  for (int c = 0; c < npairs; ++c) if (fscanf(f, "%d %d", &fa[c], &fb[c]) != 2) return 2;
  std::vector<uint32_t> tails;
  unsigned w;
  while (fscanf(f, "%u", &w) == 1) tails.push_back(w);
  fclose(f);
  const pm::ShortKeyIndex x = pm::short_key_index(tails.data(), tails.size(), npairs, fa, fb);
  printf("%zu %zu %zu\n", x.bitmap.size(), x.rows.size(), x.order.size());
  for (uint32_t v : x.bitmap) printf("%u\n", v);
  for (uint32_t v : x.rows) printf("%u\n", v);
  for (uint32_t v : x.order) printf("%u\n", v);
  return 0;
}
"""


def key_of(w, a, b):
    return ((w >> (8 * a)) & 0xFF) | (((w >> (8 * b)) & 0xFF) << 8)


def test_key_index_of_every_field_pair(tmp_path):
    rng = np.random.default_rng(1619)
    tails = [int(x) for x in rng.integers(0, 1 << 32, size=400, dtype=np.uint64)]
    tails += [tails[3], tails[3], tails[120], 0, 0, 0xFFFFFFFF]                       # whole tails twice
    tails += [(tails[7] & 0x0000FFFF) | (int(rng.integers(0, 1 << 16)) << 16) for _ in range(3)]   # equal in fields 0 and 1 only
    tails += [(tails[9] & 0xFF0000FF) | (int(rng.integers(0, 1 << 16)) << 8) for _ in range(3)]    # equal in fields 0 and 3 only
    order = rng.permutation(len(tails))
    tails = [tails[i] for i in order]
    m = len(tails)
    src = tmp_path / "tables_check.cc"
    src.write_text(HARNESS)
    exe = tmp_path / "tables_check"
    subprocess.check_call([compiler(), "-O2", "-std=c++17", "-I", HEADER_DIR, str(src), "-o", str(exe)])
    for pairs in (PAIRS, [(0, 1), (2, 3)]):                          # the plans of k = 2 and of k = 1 substitution
        inp = tmp_path / "tails.txt"
        inp.write_text("%d\n%s\n%s\n" % (len(pairs), " ".join("%d %d" % p for p in pairs), "\n".join(str(t) for t in tails)))
        r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-1000:]
        out = np.array(r.stdout.split(), dtype=np.int64)
        nb, nr, no = (int(x) for x in out[:3])
        assert (nb, nr, no) == (len(pairs) * 2048, len(pairs) * 65537, len(pairs) * m)
        bitmap, rows, runs = out[3:3 + nb], out[3 + nb:3 + nb + nr], out[3 + nb + nr:]
        assert runs.size == no
        for c, (a, b) in enumerate(pairs):
            rw = rows[c * 65537:(c + 1) * 65537]
            assert rw[0] == c * m and rw[-1] == (c + 1) * m, (c, rw[0], rw[-1])
            assert np.all(np.diff(rw) >= 0), c
            want = {}
            for j, t in enumerate(tails):
                want.setdefault(key_of(t, a, b), []).append(j)       # (in increasing pattern index)
            assert any(len(v) > 1 for v in want.values())
            bits = (bitmap[c * 2048:(c + 1) * 2048, None] >> np.arange(32)[None, :]) & 1
            nonempty = np.diff(rw) > 0
            assert np.array_equal(bits.reshape(-1).astype(bool), nonempty), c
            assert set(np.flatnonzero(nonempty).tolist()) == set(want), c
            for x, js in want.items():
                assert runs[rw[x]:rw[x + 1]].tolist() == js, (c, x)
