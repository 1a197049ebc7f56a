"""CPU: the pair scan kernels' workgroup -> (field pair, chunk) maps (csrc/pm_workmap.h) are bijections.

The kernels and this test compile the same header: a small host program includes it, walks every block of every grid
below and reports what does not hold.  Checked for the three maps, chunk counts 1 .. a few thousand, 2 (-K 1), 6 (-K 2)
and 14 (-k 2, the edit plan's tests) field pairs, so grids of every size modulo 8:
  * every block of the grid gets a (combo, chunk) inside the grid, every (combo, chunk) exactly one block; the first
    block past the grid gets none;
  * the XCD map: the blocks of one XCD (equal blockIdx % 8) take their items field pair after field pair, chunks
    ascending inside one, and the XCDs' chunk ranges overlap in at most one chunk;
  * the XCD superchunk map: superchunk after superchunk, and inside one the blocks of an XCD take consecutive items of
    the superchunk's combo-major order.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "sequence-alignment-tools_amd", "csrc")

HARNESS = r"""
#include <cstdio>
#include <vector>
#include "pm_workmap.h"

static int fails = 0;
static void fail(const char *what, int map, int nchunks, int ncombos, int b) {
  if (fails++ < 20) printf("FAIL %s map=%d nchunks=%d ncombos=%d block=%d\n", what, map, nchunks, ncombos, b);
}

static void check(int map, int nchunks, int ncombos, int group) {
  const int G = nchunks * ncombos;
  std::vector<int> seen((size_t)G, 0);
  std::vector<long long> last(pm::PAIR_XCDS, -1);              // XCD map: last item (combo-major key) per XCD
  std::vector<int> lo(pm::PAIR_XCDS, nchunks), hi(pm::PAIR_XCDS, -1);
  std::vector<int> prev_sc(pm::PAIR_XCDS, -1), prev_t(pm::PAIR_XCDS, -1);
  for (int b = 0; b <= G; ++b) {
    int c = -1, j = -1;
    if (map == pm::PAIR_MAP_XCD) pm::pair_xcd_item(b, nchunks, ncombos, &c, &j);
    else if (map == pm::PAIR_MAP_XCD_SUPERCHUNK) pm::pair_xcd_superchunk_item(b, nchunks, ncombos, group, &c, &j);
    else pm::pair_superchunk_item(b, nchunks, ncombos, group, &c, &j);
    if (b == G) {
      if (c < ncombos && j < nchunks) fail("block past the grid got an item", map, nchunks, ncombos, b);
      break;
    }
    if (c < 0 || c >= ncombos || j < 0 || j >= nchunks) { fail("item outside the grid", map, nchunks, ncombos, b); continue; }
    if (seen[(size_t)j * ncombos + c]++) fail("item taken twice", map, nchunks, ncombos, b);
    if (map == pm::PAIR_MAP_XCD_SUPERCHUNK) {
      const int x = b % pm::PAIR_XCDS, sc = j / group, K = nchunks - sc * group < group ? nchunks - sc * group : group;
      const int t = c * K + (j - sc * group);                  // rank inside the superchunk, combo-major
      if (sc < prev_sc[x] || (sc == prev_sc[x] && t != prev_t[x] + 1)) fail("XCD piece of a superchunk not consecutive", map, nchunks, ncombos, b);
      prev_sc[x] = sc; prev_t[x] = t;
    }
    if (map == pm::PAIR_MAP_XCD) {
      const int x = b % pm::PAIR_XCDS;
      const long long key = (long long)c * nchunks + j;
      if (key <= last[x]) fail("XCD does not walk field pair after field pair, chunks ascending", map, nchunks, ncombos, b);
      last[x] = key;
      if (j < lo[x]) lo[x] = j;
      if (j > hi[x]) hi[x] = j;
    }
  }
  for (int i = 0; i < G; ++i) if (seen[(size_t)i] != 1) { fail("item not taken", map, nchunks, ncombos, i); break; }
  if (map == pm::PAIR_MAP_XCD)
    for (int x = 0; x + 1 < pm::PAIR_XCDS; ++x)
      for (int y = x + 1; y < pm::PAIR_XCDS; ++y)
        if (hi[x] >= 0 && hi[y] >= 0 && hi[x] > lo[y]) fail("XCD chunk shares overlap in more than one chunk", map, nchunks, ncombos, x);
}

int main() {
  const int combos[] = {2, 6, 14};
  long long grids = 0;
  for (int ncombos : combos)
    for (int nchunks = 1; nchunks <= 3000; ++nchunks) {
      for (int map = 0; map < 3; ++map) check(map, nchunks, ncombos, 256);
      grids += 3;
    }
  for (int nchunks = 1; nchunks <= 700; nchunks += 3)                 // PM_SEED_GROUP: other run lengths
    for (int group : {1, 3, 37}) { check(0, nchunks, 6, group); check(2, nchunks, 6, group); check(2, nchunks, 14, group); grids += 3; }
  for (int nchunks : {4095, 4096, 4097, 8191, 12345})
    for (int map = 0; map < 3; ++map) { check(map, nchunks, 6, 256); check(map, nchunks, 14, 256); grids += 2; }
  printf("grids %lld fails %d\n", grids, fails);
  return fails ? 1 : 0;
}
"""


def compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    pytest.fail("no C++ compiler for the work-map harness")


def test_pair_work_maps_are_bijections(tmp_path):
    src = tmp_path / "workmap_check.cc"
    src.write_text(HARNESS)
    exe = tmp_path / "workmap_check"
    subprocess.check_call([compiler(), "-O2", "-std=c++17", "-I", HEADER_DIR, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "fails 0" in r.stdout, r.stdout


def test_xcd_maps_keep_each_xcd_on_one_field_pair_per_run(tmp_path):
    """The flagship grid (3 Gbp at -K 2: 1431 chunks x 6 field pairs = 8586 blocks): with 32 workgroups of an XCD in
    flight at a time, a window of 32 consecutive blocks of one XCD holds ONE field pair under both XCD maps in all but
    the windows that straddle a change of field pair; the superchunk map's windows straddle two almost always."""
    src = tmp_path / "workmap_runs.cc"
    src.write_text(r"""
#include <cstdio>
#include "pm_workmap.h"
int main() {
  const int nchunks = 1431, ncombos = 6, G = nchunks * ncombos;
  for (int map = 0; map < 3; ++map) {
    long long windows = 0, mixed = 0;
    for (int x = 0; x < pm::PAIR_XCDS; ++x)
      for (int l0 = 0; 8 * (l0 + 32) + x <= G; ++l0) {
        int c0 = -1, c1 = -1, j;
        if (map == pm::PAIR_MAP_XCD) { pm::pair_xcd_item(8 * l0 + x, nchunks, ncombos, &c0, &j); pm::pair_xcd_item(8 * (l0 + 31) + x, nchunks, ncombos, &c1, &j); }
        else if (map == pm::PAIR_MAP_XCD_SUPERCHUNK) {
          pm::pair_xcd_superchunk_item(8 * l0 + x, nchunks, ncombos, 256, &c0, &j); pm::pair_xcd_superchunk_item(8 * (l0 + 31) + x, nchunks, ncombos, 256, &c1, &j);
        } else { pm::pair_superchunk_item(8 * l0 + x, nchunks, ncombos, 256, &c0, &j); pm::pair_superchunk_item(8 * (l0 + 31) + x, nchunks, ncombos, 256, &c1, &j); }
        ++windows; mixed += c0 != c1;
      }
    printf("%d %lld %lld\n", map, windows, mixed);
  }
  return 0;
}
""")
    exe = tmp_path / "workmap_runs"
    subprocess.check_call([compiler(), "-O2", "-std=c++17", "-I", HEADER_DIR, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True, timeout=120).stdout.split("\n")
    frac = {}
    for line in out:
        if line.strip():
            m, w, x = map(int, line.split())
            frac[m] = x / w
    assert frac[1] < 0.2, frac          # the XCD map: ~31 of ~179 windows per field pair straddle a change
    assert frac[2] < 0.2, frac          # the XCD superchunk map: half the XCDs never change, the others once per superchunk and at its end
    assert frac[0] > 0.9, frac          # the superchunk map: the mix the XCD maps remove
