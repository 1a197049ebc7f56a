"""CPU: the wild class's exact stage (wild_verify<4>, csrc/pm_verify.h) and its table builder (csrc/pm_wild_tables.h)
against plain restatements.

The kernels and this test compile the same headers.  A stand-alone host program, built with -fsanitize=address,undefined
and run as a program of its own, checks
  (a) wild_verify<4> on random windows against a character-by-character restatement: class match and mismatch, N and
      other codes as mismatch, an end-of-sequence character at every index of the window, start < 0, the last 1..31 bytes
      of the stream, zones with and without viol_level, the first-clean-pair rule at k = 1 and k = 2, the registered-pair
      rule at k = 0, the half flags -- on a normalized and on a raw ASCII stream;
  (b) the table builder on 2,000 random primers of 16..32 characters with 3..6 ambiguity letters: every window within k
      class-mismatches of a primer's last 16 characters has a key in some pair's bitmap, that key's run holds an entry of
      the primer whose class word passes the judge count, every entry's class word equals the restated classes, and the
      per-pair cap of 256 keys and the entry cap of 24,000 refuse exactly the lists a restatement refuses.
The restatement has its own table of IUPAC classes, written out by hand; the product takes them from pm_iupac.h.
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
#include <string>
#include <vector>
#include "pm_verify.h"
#include "pm_wild_tables.h"

static int fails = 0;
static unsigned long long rs = 88172645463325252ull;
static unsigned rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (unsigned)(rs >> 11); }
#define FAIL(...) do { if (fails++ < 20) { printf("FAIL " __VA_ARGS__); printf("\n"); } } while (0)

// The restatement's own classes: the A,C,G,T every letter accepts under -w, read off the reference's compatibility sets
// by hand (bit q = "ACGT"[q]): only the A,C,G,T a set names count (T's set names V, the reference's quirk, and no A, C or G).
static int restated_class(char ch) {
  switch (ch) {
    case 'A': return 1; case 'C': return 2; case 'G': return 4; case 'T': return 8;
    case 'R': return 1 | 4; case 'Y': return 2 | 8; case 'K': return 4 | 8; case 'M': return 1 | 2;
    case 'S': return 2 | 4; case 'W': return 1 | 8; case 'B': return 2 | 4 | 8; case 'D': return 1 | 4 | 8;
    case 'H': return 1 | 2 | 8; case 'V': return 1 | 2 | 4; case 'N': return 15;
  }
  return 0;
}
static int pop4(int c) { return (c & 1) + ((c >> 1) & 1) + ((c >> 2) & 1) + ((c >> 3) & 1); }
static const char LETTERS[] = "RYKMSWBDHVN";

struct Args {                                   // the fields wild_verify reads of a kernel's argument block
  const uint8_t *text; int64_t n; int k, eos_code, ascii, ncombos, viol_level; int fa[6], fb[6];
  const uint8_t *pat_len; const uint32_t *pat_id; const uint8_t *pat_class; const uint8_t *pat_reg; const uint32_t *pat_zone;
};

// stream bytes: normalized 0..3 = A,C,G,T, 4 = N, 5 = end of sequence, 6 = another code; raw ASCII: the letters, '\n' = EOS
static bool restated(const Args &a, const std::string &pat, int combo, int64_t p, int *level, int *flags) {
  const int L = (int)pat.size();
  const int64_t start = p + 1 - L;
  if (start < 0) return false;
  int mism = 0; bool viol = false, left = true, right = true;
  bool dirty[4] = {false, false, false, false};
  for (int i = 0; i < L; ++i) {
    const int t = a.text[start + i];
    if (t == a.eos_code) return false;
    int code = -1;
    if (a.ascii) code = t == 'A' ? 0 : t == 'C' ? 1 : t == 'G' ? 2 : t == 'T' ? 3 : -1;
    else if (t < 4) code = t;
    if (code >= 0 && ((restated_class(pat[i]) >> code) & 1)) continue;
    ++mism;
    if ((a.pat_zone[0] >> i) & 1u) viol = true;
    if (i < L / 2) left = false; else right = false;
    const int tail = i - (L - 16);
    if (tail >= 0) dirty[tail / 4] = true;
  }
  if (mism > a.k) return false;
  if (viol && a.viol_level <= 0) return false;
  if (a.k == 0) { if (combo != a.pat_reg[0]) return false; }
  else {
    int first = -1;
    for (int c = 0; c < a.ncombos && first < 0; ++c) if (!dirty[a.fa[c]] && !dirty[a.fb[c]]) first = c;
    if (first != combo) return false;
  }
  *level = viol ? a.viol_level : mism; *flags = (left ? 1 : 0) | (right ? 2 : 0);
  return true;
}

static std::string random_primer(int L, int nletters) {
  std::string s(L, 'A');
  for (int i = 0; i < L; ++i) s[i] = "ACGT"[rnd() % 4];
  for (int j = 0; j < nletters; ++j) s[rnd() % L] = LETTERS[rnd() % 11];
  return s;
}

static void check_verify(int k, int viol_level, bool ascii, long trials) {
  const int kk = k == 2 ? 2 : 1;
  Args a; memset(&a, 0, sizeof(a));
  uint8_t len[1], reg[1]; uint32_t id[1] = {77}, zone[1]; uint8_t cls[16];
  a.k = k; a.eos_code = ascii ? '\n' : 5; a.ascii = ascii ? 1 : 0; a.viol_level = viol_level;
  a.ncombos = pm::sub_ncombos(kk);
  for (int c = 0; c < a.ncombos; ++c) { a.fa[c] = pm::sub_fa(kk, c); a.fb[c] = pm::sub_fb(kk, c); }
  a.pat_len = len; a.pat_id = id; a.pat_class = cls; a.pat_reg = reg; a.pat_zone = zone;
  auto base = [&](int q) -> uint8_t { return ascii ? (uint8_t)"ACGT"[q] : (uint8_t)q; };
  const uint8_t n_byte = ascii ? 'N' : 4, other = ascii ? 'R' : 6;
  for (long t = 0; t < trials; ++t) {
    // a stream of exactly n bytes on the heap: the sanitizer sees any read past n
    const int n = 40 + (int)(rnd() % 60);
    std::vector<uint8_t> text(n);
    a.text = text.data(); a.n = n;
    const int L = 16 + (int)(rnd() % 17);
    const std::string pat = random_primer(L, (int)(rnd() % 7));
    len[0] = (uint8_t)L; reg[0] = (uint8_t)(rnd() % 2);
    memset(cls, 0, 16);
    for (int i = 0; i < L; ++i) cls[i / 2] |= (uint8_t)(pm::wild_class_of((unsigned char)pat[i]) << (4 * (i & 1)));
    const int es = rnd() % 3 == 0 ? (int)(rnd() % 6) : 0, ee = rnd() % 3 == 0 ? (int)(rnd() % 6) : 0;
    zone[0] = 0;
    for (int i = 0; i < L; ++i) if (i < es || i >= L - ee) zone[0] |= 1u << i;
    for (int i = 0; i < n; ++i) text[i] = base(rnd() % 4);
    // where: the stream's start (start < 0 and start = 0), its last 1..31 bytes (the 32-byte read does not fit), the middle
    const int where = (int)(rnd() % 4);
    int64_t p = where == 0 ? (int64_t)(rnd() % (L + 2)) : where == 1 ? n - 1 - (int64_t)(rnd() % 3) : L - 1 + (int64_t)(rnd() % (n - L + 1));
    if (p >= n) p = n - 1;
    const int64_t start = p + 1 - L;
    if (start >= 0) {
      for (int i = 0; i < L; ++i) {                                 // a random concrete variant
        const int c = restated_class(pat[i]);
        int q = (int)(rnd() % 4);
        while (!((c >> q) & 1)) q = (q + 1) % 4;
        text[start + i] = base(q);
      }
      const int subs = (int)(rnd() % 4);
      for (int s = 0; s < subs; ++s) {
        const int i = (int)(rnd() % L), what = (int)(rnd() % 16);
        text[start + i] = what == 0 ? n_byte : what == 1 ? (uint8_t)a.eos_code : what == 2 ? other : base(rnd() % 4);
      }
      if (t % 8 == 0) text[start + (t / 8) % L] = (uint8_t)a.eos_code;   // EOS at every index of the window in turn
    }
    for (int combo = 0; combo < a.ncombos; ++combo) {
      pm_hit hh; memset(&hh, 0, sizeof(hh));
      int level = -1, flags = -1;
      const bool got = pm::wild_verify<4>(a, combo, p, 0, &hh), want = restated(a, pat, combo, p, &level, &flags);
      bool ok = got == want;
      if (ok && got) ok = hh.end == p + 1 && hh.pid == 77 && hh.k == level && hh.aux[0] == flags && hh.aux[1] == 0 && hh.aux[2] == 0;
      if (!ok) FAIL("verify k=%d viol=%d ascii=%d L=%d n=%d p=%lld combo=%d got=%d want=%d pat=%s", k, viol_level, (int)ascii, L, n, (long long)p, combo, (int)got, (int)want, pat.c_str());
    }
  }
}

// the restatement of the caps
static size_t restated_pair_keys(const std::string &s, int fa, int fb) {
  size_t n = 1;
  const int L = (int)s.size();
  for (int i = 0; i < 4; ++i) n *= (size_t)pop4(restated_class(s[L - 16 + 4 * fa + i])) * (size_t)pop4(restated_class(s[L - 16 + 4 * fb + i]));
  return n;
}
static bool restated_fits(const std::string &s, int k) {
  const int kk = k == 2 ? 2 : 1;
  for (char ch : s) if (!restated_class(ch)) return false;
  for (int c = 0; c < pm::sub_ncombos(kk); ++c) if (restated_pair_keys(s, pm::sub_fa(kk, c), pm::sub_fb(kk, c)) > 256) return false;
  return s.size() >= 16 && s.size() <= 32;
}
static bool restated_entries_fit(const std::vector<std::string> &pats, int k) {
  const int kk = k == 2 ? 2 : 1;
  for (int c = 0; c < pm::sub_ncombos(kk); ++c) {
    size_t e = 0;
    for (const std::string &s : pats) {
      if (k == 0) { const int reg = restated_pair_keys(s, 2, 3) < restated_pair_keys(s, 0, 1) ? 1 : 0; if (reg != c) continue; }
      e += restated_pair_keys(s, pm::sub_fa(kk, c), pm::sub_fb(kk, c));
    }
    if (e > 24000) return false;
  }
  return true;
}

static void check_tables(int k, bool ascii) {
  const int kk = k == 2 ? 2 : 1;
  std::vector<std::string> all, pats;
  for (int j = 0; j < 2000; ++j) all.push_back(random_primer(16 + (int)(rnd() % 17), 3 + (int)(rnd() % 4)));
  // a few the per-pair cap has to refuse: five N's in one field pair
  for (int j = 0; j < 20; ++j) { std::string s = random_primer(16 + (int)(rnd() % 17), 0); const int L = (int)s.size(); for (int i = 0; i < 5; ++i) s[L - 16 + i] = 'N'; all.push_back(s); }
  { std::string s = random_primer(20, 0); s[1] = 'X'; all.push_back(s); }   // (X accepts no base)
  // and primers at the per-pair cap -- two N's in every field, 256 keys in every pair -- that carry the list over the entry cap
  for (int j = 0; j < 200; ++j) { std::string s = random_primer(16 + (int)(rnd() % 17), 0); const int L = (int)s.size(); for (int f = 0; f < 4; ++f) { s[L - 16 + 4 * f + (int)(rnd() % 2)] = 'N'; s[L - 16 + 4 * f + 2 + (int)(rnd() % 2)] = 'N'; } all.push_back(s); }
  size_t refused = 0;
  for (const std::string &s : all) {
    const bool got = pm::wild_primer_fits(s, k), want = restated_fits(s, k);
    if (got != want) FAIL("wild_primer_fits k=%d %s got=%d want=%d", k, s.c_str(), (int)got, (int)want);
    if (want) pats.push_back(s); else ++refused;
  }
  if (refused < 21) FAIL("the per-pair cap refused %zu primers", refused);
  // the entry cap: growing prefixes of the list, on either side of 24,000
  std::vector<std::string> kept;
  bool seen_fit = false, seen_refused = false;
  for (size_t m = 50; m <= pats.size(); m += 50) {
    std::vector<std::string> sub(pats.begin(), pats.begin() + m);
    const bool got = pm::wild_entries_fit(sub, k), want = restated_entries_fit(sub, k);
    if (got != want) FAIL("wild_entries_fit k=%d m=%zu got=%d want=%d", k, m, (int)got, (int)want);
    pm::WildIndex probe;
    const bool built = pm::wild_build_index(sub, k, ascii, &probe).empty();
    if (built != want) FAIL("wild_build_index k=%d m=%zu built=%d want=%d", k, m, (int)built, (int)want);
    if (want) { kept = sub; seen_fit = true; } else seen_refused = true;
  }
  if (!seen_fit || !seen_refused) FAIL("entry cap not crossed k=%d fit=%d refused=%d", k, (int)seen_fit, (int)seen_refused);
  pm::WildIndex x;
  if (!pm::wild_build_index(kept, k, ascii, &x).empty()) { FAIL("build of the kept list"); return; }
  auto code_of = [&](int q) { return ascii ? (q == 2 ? 3 : q == 3 ? 2 : q) : q; };   // "ACGT"[q] in the stream's packing
  auto class_bit = [&](char ch, int code) {                         // the restated class accepts the base packed as `code`
    for (int q = 0; q < 4; ++q) if (code_of(q) == code) return (restated_class(ch) >> q) & 1;
    return 0;
  };
  // every entry: its primer, its class word, its key inside the primer's classes; rows in order
  for (int c = 0; c < x.ncombos; ++c) {
    const uint32_t *rows = &x.rows[(size_t)c * pm::SHORT_ROWS];
    for (uint32_t key = 0; key < 65536; ++key) {
      if (rows[key] > rows[key + 1]) { FAIL("rows not monotone"); break; }
      const bool bit = (x.bitmap[(size_t)c * pm::SHORT_BM_WORDS + (key >> 5)] >> (key & 31u)) & 1u;
      if (bit != (rows[key] < rows[key + 1])) FAIL("bitmap and rows disagree c=%d key=%u", c, key);
      for (uint32_t e = rows[key]; e < rows[key + 1]; ++e) {
        const uint32_t j = (uint32_t)x.runs[e], word = (uint32_t)(x.runs[e] >> 32);
        if (j >= kept.size()) { FAIL("entry of no primer"); continue; }
        const std::string &s = kept[j];
        const int L = (int)s.size();
        if (k == 0 && x.reg[j] != c) FAIL("entry under a pair the primer is not registered for");
        int at = 0; uint32_t want = 0;
        for (int f = 0; f < 4; ++f) if (f != x.fa[c] && f != x.fb[c]) for (int i = 0; i < 4; ++i, ++at)
          for (int code = 0; code < 4; ++code) if (class_bit(s[L - 16 + 4 * f + i], code)) want |= 1u << (4 * at + code);
        if (word != want) FAIL("class word c=%d j=%u", c, j);
        for (int i = 0; i < 4; ++i) {
          if (!class_bit(s[L - 16 + 4 * x.fa[c] + i], (key >> (2 * i)) & 3u)) FAIL("key outside the classes c=%d j=%u", c, j);
          if (!class_bit(s[L - 16 + 4 * x.fb[c] + i], (key >> (8 + 2 * i)) & 3u)) FAIL("key outside the classes c=%d j=%u", c, j);
        }
      }
    }
    if (rows[65536] - rows[0] != x.entries[c]) FAIL("entries of pair %d", c);
  }
  // pat_class: one nibble per character
  for (size_t j = 0; j < kept.size(); ++j) for (size_t i = 0; i < kept[j].size(); ++i)
    if (((x.pat_class[j * 16 + i / 2] >> (4 * (i & 1))) & 15) != restated_class(kept[j][i])) FAIL("pat_class j=%zu i=%zu", j, i);
  // cover: windows within k class-mismatches of a primer's tail
  for (size_t j = 0; j < kept.size(); ++j) {
    const std::string &s = kept[j];
    const int L = (int)s.size();
    for (int rep = 0; rep < 6; ++rep) {
      int wb[16];
      for (int i = 0; i < 16; ++i) { int q = (int)(rnd() % 4); while (!((restated_class(s[L - 16 + i]) >> q) & 1)) q = (q + 1) % 4; wb[i] = code_of(q); }
      const int subs = (int)(rnd() % (k + 2));                       // 0 .. k + 1 changed bases (a change may stay inside the class)
      for (int t = 0; t < subs; ++t) wb[rnd() % 16] = (int)(rnd() % 4);
      int dist = 0;
      uint32_t W = 0;
      for (int i = 0; i < 16; ++i) { W |= (uint32_t)wb[i] << (2 * i); dist += !class_bit(s[L - 16 + i], wb[i]); }
      bool found = false;
      for (int c = 0; c < x.ncombos && !found; ++c) {
        const uint32_t key = pm::sub_key(W, x.fa[c], x.fb[c]);
        if (!((x.bitmap[(size_t)c * pm::SHORT_BM_WORDS + (key >> 5)] >> (key & 31u)) & 1u)) continue;
        const uint32_t *rows = &x.rows[(size_t)c * pm::SHORT_ROWS];
        const uint32_t others = pm::wild_others(W, x.fa[c], x.fb[c]);
        for (uint32_t e = rows[key]; e < rows[key + 1] && !found; ++e) {
          if ((uint32_t)x.runs[e] != j) continue;
          int om = 0, at = 0;                                         // the judge's count, restated
          for (int f = 0; f < 4; ++f) if (f != x.fa[c] && f != x.fb[c]) for (int i = 0; i < 4; ++i, ++at) om += !class_bit(s[L - 16 + 4 * f + i], wb[4 * f + i]);
          if (pm::wild_others_mismatches(others, (uint32_t)(x.runs[e] >> 32)) != om) FAIL("judge count j=%zu c=%d", j, c);
          if (pm::wild_others_within(others, (uint32_t)(x.runs[e] >> 32), k)) found = true;
        }
      }
      if (dist <= k && !found) FAIL("cover k=%d dist=%d j=%zu %s", k, dist, j, s.c_str());
    }
  }
}

int main() {
  for (int q = 0; q < 256; ++q) {
    const char *letters = "ACGTRYKMSWBDHVN";
    const bool known = q && strchr(letters, q);
    if (known && (int)pm::wild_class_of((unsigned char)q) != restated_class((char)q)) FAIL("class of %c", q);
  }
  if (pm::wild_class_of('X') != 0) FAIL("class of X");
  for (int ascii = 0; ascii < 2; ++ascii) {
    check_verify(0, 0, ascii, 60000);
    for (int k = 1; k <= 2; ++k) for (int viol = 0; viol <= 3; viol += 3) check_verify(k, viol, ascii, 60000);
  }
  for (int k = 0; k <= 2; ++k) check_tables(k, k == 1);
  check_tables(2, true);
  printf("fails %d\n", fails);
  return fails ? 1 : 0;
}
"""


def compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    pytest.fail("no C++ compiler for the wild class harness")


def test_wild_verify_and_table_builder(tmp_path):
    src = tmp_path / "wild_check.cc"
    src.write_text(HARNESS)
    exe = tmp_path / "wild_check"
    subprocess.check_call([compiler(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", HEADER_DIR, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "fails 0" in r.stdout, r.stdout
