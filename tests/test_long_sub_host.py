"""CPU: the exact verify on rows of 64 characters (csrc/pm_verify.h, pair_verify<5, 64>: patterns of up to 64 characters
in a wide tile of the pair plan) against a plain restatement.

The kernels and this test compile the same header.  A small host program checks pair_verify<5, 64> for k = 1 and 2, with
and without a violation level, character by character:
  * lengths 20, 32, 33, 47, 63, 64 (L = 64: no shift by the mask's width; L = 33: the first bit beyond a dword; 20 and
    32: short patterns whose rows are padded to 64, so the 64-byte read crosses the stream's end far more often);
  * exact zones at the pattern's start and end, so that zone bits lie on either side of index 32;
  * substitutions, N and end-of-sequence characters at indices below and above 32 (a forced one at a chosen index in
    every trial with a window, beside the random ones);
  * start < 0, start = 0, and windows whose end lies within 64 bytes of the stream's end (the byte-wise read);
  * the clean-half flags, L = 33 (half = 16) and L = 64 (half = 32) among them.
The stream is a heap block of exactly n bytes, so a read past its end -- the byte-wise path of the last windows must stay
inside a.n -- is an error a stand-alone build of the harness under -fsanitize=address,undefined reports.
pair_verify<5, 32> and the default pair_verify<5> go through the same restatement on 20..32 characters: the narrow
instantiation is the one the kernels of tiles without a long pattern keep.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "sequence-alignment-tools_amd", "csrc")

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "pm_verify.h"

static int fails = 0;
static long seen_hit[65], seen_hi_sub = 0, seen_hi_eos = 0, seen_hi_zone = 0, seen_edge = 0, seen_neg = 0;
static unsigned long long rs = 88172645463325252ull;
static unsigned rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (unsigned)(rs >> 11); }

struct Args {                                   // the fields pair_verify reads of a kernel's argument block
  const uint8_t *text; int64_t n; int k, eos_code, ncombos, viol_level; int fa[6], fb[6];
  const uint8_t *pat_len; const uint32_t *pat_id; const uint8_t *pat_codes; const uint32_t *pat_zone;
};

// codes: 0..3 = A,C,G,T, 4 = N, 5 = end of sequence.  CW: characters per row of pat_codes, zone[i]: character i is exact
static bool restated(int CW, const Args &a, const bool *zone, int combo, int64_t p, int *level, int *flags) {
  const int FW = 5, L = a.pat_len[0];
  const int64_t start = p + 1 - L;
  if (start < 0) return false;
  int mism = 0; bool viol = false, left = true, right = true;
  bool dirty[4] = {false, false, false, false};
  for (int i = 0; i < L; ++i) {
    const int t = a.text[start + i], c = a.pat_codes[i];
    if (t == a.eos_code) return false;
    if (t == c) continue;
    ++mism;
    if (zone[i]) viol = true;
    if (i < L / 2) left = false; else right = false;
    const int tail = i - (L - 4 * FW);
    if (tail >= 0) dirty[tail / FW] = true;
  }
  (void)CW;
  if (mism > a.k) return false;
  if (viol && a.viol_level <= 0) return false;
  int first = -1;
  for (int c = 0; c < a.ncombos && first < 0; ++c) if (!dirty[a.fa[c]] && !dirty[a.fb[c]]) first = c;
  if (first != combo) return false;
  *level = viol ? a.viol_level : mism; *flags = (left ? 1 : 0) | (right ? 2 : 0);
  return true;
}

template <int CW, bool DEFAULTED>
static void check_verify(int k, int viol_level, long trials) {
  const int n = 300;
  uint8_t *text = (uint8_t *)malloc(n);            // exactly n bytes: nothing to read behind the stream's end
  uint8_t len[1]; uint32_t id[1] = {77}, zw[2]; bool zone[64];
  alignas(16) uint8_t codes[64];
  Args a; memset(&a, 0, sizeof(a));
  a.text = text; a.n = n; a.k = k; a.eos_code = 5; a.viol_level = viol_level;
  a.ncombos = pm::sub_ncombos(k);
  for (int c = 0; c < a.ncombos; ++c) { a.fa[c] = pm::sub_fa(k, c); a.fb[c] = pm::sub_fb(k, c); }
  a.pat_len = len; a.pat_id = id; a.pat_codes = codes; a.pat_zone = zw;
  static const int wide_len[6] = {20, 32, 33, 47, 63, 64};
  for (long t = 0; t < trials; ++t) {
    const int L = CW == 64 ? wide_len[rnd() % 6] : 20 + (int)(rnd() % 13);
    len[0] = (uint8_t)L;
    memset(codes, 0, 64);
    for (int i = 0; i < L; ++i) codes[i] = (uint8_t)(rnd() % 4);
    // exact zones: up to 9 characters at the start (indices below 32) and at the end (above 32 for L >= 42)
    const int es = rnd() % 3 == 0 ? (int)(rnd() % 10) : 0, ee = rnd() % 3 == 0 ? (int)(rnd() % 10) : 0;
    zw[0] = zw[1] = 0;
    for (int i = 0; i < 64; ++i) zone[i] = false;
    for (int i = 0; i < L; ++i) if (i < es || i >= L - ee) { zone[i] = true; zw[i / 32] |= 1u << (i % 32); }
    for (int i = 0; i < n; ++i) text[i] = (uint8_t)(rnd() % 4);
    // where: the stream's start (start < 0 and start = 0), its end (the CW-byte read does not fit), the middle
    const int where = (int)(rnd() % 4);
    int64_t p = where == 0 ? (int64_t)(rnd() % (L + 2)) : where == 1 ? n - 1 - (int64_t)(rnd() % 50) : L + (int64_t)(rnd() % (n - L));
    if (p >= n) p = n - 1;
    const int64_t start = p + 1 - L;
    if (start < 0) ++seen_neg;
    if (start >= 0) {
      if (start + CW > n) ++seen_edge;
      for (int i = 0; i < L; ++i) text[start + i] = codes[i];
      // behind the window, inside the row's padding: characters that are no part of the verdict, EOS among them
      if (rnd() % 4 == 0) for (int i = L; i < CW && start + i < n; ++i) text[start + i] = 5;
      const int subs = (int)(rnd() % 4);
      for (int s = 0; s < subs; ++s) {
        // half of the trials put their first change at the pattern's highest indices (>= 32 for the long ones)
        const int i = s == 0 && (t & 1) ? L - 1 - (int)(rnd() % (L > 40 ? L - 32 : 8)) : (int)(rnd() % L);
        const int what = (int)(rnd() % 16);
        text[start + i] = what == 0 ? 4 : what == 1 ? 5 : (uint8_t)((codes[i] + 1 + rnd() % 3) % 4);
        if (i >= 32) { ++seen_hi_sub; if (what == 1) ++seen_hi_eos; if (zone[i]) ++seen_hi_zone; }
      }
    }
    for (int combo = 0; combo < a.ncombos; ++combo) {
      pm_hit hh; memset(&hh, 0, sizeof(hh));
      int level = -1, flags = -1;
      const bool got = DEFAULTED ? pm::pair_verify<5>(a, combo, p, 0, &hh) : pm::pair_verify<5, CW>(a, combo, p, 0, &hh);
      const bool want = restated(CW, a, zone, combo, p, &level, &flags);
      bool ok = got == want;
      if (ok && got) { ok = hh.end == p + 1 && hh.pid == 77 && hh.k == level && hh.aux[0] == flags && hh.aux[1] == 0 && hh.aux[2] == 0; ++seen_hit[L]; }
      if (!ok && fails++ < 20) printf("FAIL verify CW=%d k=%d viol=%d L=%d p=%lld combo=%d got=%d want=%d\n", CW, k, viol_level, L, (long long)p, combo, (int)got, (int)want);
    }
  }
  free(text);
}

int main() {
  for (int k = 1; k <= 2; ++k) for (int viol = 0; viol <= 3; viol += 3) {
    check_verify<64, false>(k, viol, 300000);
    check_verify<32, false>(k, viol, 100000);
    check_verify<32, true>(k, viol, 100000);
  }
  // the cases the test is about were reached
  static const int must[6] = {20, 32, 33, 47, 63, 64};
  for (int i = 0; i < 6; ++i) if (seen_hit[must[i]] < 1000) { printf("FAIL coverage: %ld records at L=%d\n", seen_hit[must[i]], must[i]); ++fails; }
  if (seen_hi_sub < 1000 || seen_hi_eos < 100 || seen_hi_zone < 100 || seen_edge < 1000 || seen_neg < 1000) {
    printf("FAIL coverage: %ld %ld %ld %ld %ld\n", seen_hi_sub, seen_hi_eos, seen_hi_zone, seen_edge, seen_neg); ++fails;
  }
  printf("fails %d\n", fails);
  return fails ? 1 : 0;
}
"""


def compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    pytest.fail("no C++ compiler for the verify harness")


def test_verify_on_rows_of_64_characters(tmp_path):
    src = tmp_path / "verify_wide_check.cc"
    src.write_text(HARNESS)
    exe = tmp_path / "verify_wide_check"
    subprocess.check_call([compiler(), "-O2", "-std=c++17", "-I", HEADER_DIR, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "fails 0" in r.stdout, r.stdout
