// pm_wild_tables.h -- the key index of the wild class (pm_wild_sub_scan, pm_short.hip): primers of 16..32
// -- 16..64 with PM_WILD_LONG -- characters with IUPAC ambiguity letters, compared by CLASS.  The geometry is pm_short_sub_scan's -- a primer's last 16
// characters as four fields of four, the field pairs of sub_fa / sub_fb (pm_verify.h) -- but a key multiplies over the
// ambiguity letters of its own two fields only, and a run entry carries the classes of the eight bases outside the key.
// Plain C++: tests/test_wild_class_host.py compiles it with the host compiler and checks it against a restatement.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "pm_iupac.h"
#include "pm_short_tables.h"
#include "pm_verify.h"

namespace pm {

constexpr size_t WILD_MAX_PAIR_KEYS = 256;          // keys one primer may have in one field pair (four N's in a pair still fit)
// Run entries (expanded keys) one field pair may hold: SHORT_SUB_MAX_PATTERNS of pm_internal.h, the measured ceiling of
// this skeleton's run tables with a pattern per entry.  Not measured for this class.
constexpr size_t WILD_MAX_ENTRIES = 24000;

// The A,C,G,T a pattern character accepts under -w, bit q = "ACGT"[q] -- from the compatibility table alone (pm_iupac.h:
// its quirks are the reference's).  0: the character accepts no base.
inline uint32_t wild_class_of(unsigned char ch) {
  uint32_t c = 0;
  const char *set = iupac_compatible_set(ch);
  if (!set) return 0;
  for (const char *q = set; *q; ++q) c |= *q == 'A' ? 1u : *q == 'C' ? 2u : *q == 'G' ? 4u : *q == 'T' ? 8u : 0u;
  return c;
}
// the class as the set of the stream's 2-bit codes (pm_seed.hip pack4: A,C,G,T = 0,1,2,3, raw ASCII streams 0,1,3,2)
inline uint32_t wild_code_class(uint32_t acgt, bool ascii) {
  return ascii ? (acgt & 3u) | ((acgt & 4u) << 1) | ((acgt & 8u) >> 1) : acgt;
}
inline int wild_pop4(uint32_t c) { return (int)((c & 1u) + ((c >> 1) & 1u) + ((c >> 2) & 1u) + ((c >> 3) & 1u)); }

// keys of a primer in field pair (a, b): the product of the class sizes over the pair's eight bases (0: some class is empty)
inline size_t wild_pair_keys(const std::string &s, int a, int b) {
  const size_t L = s.size();
  size_t n = 1;
  for (int f : {a, b}) for (int i = 0; i < 4; ++i) n *= (size_t)wild_pop4(wild_class_of((unsigned char)s[L - 16 + 4 * f + i]));
  return n;
}
// A primer the class can hold at all (its number of concrete variants is the routing's business): 16..maxL characters, a
// base accepted at every character, at most WILD_MAX_PAIR_KEYS keys in every field pair of the plan (k = 0: the plan of k = 1).
// maxL: the largest length the caller admits -- 32, or 64 where the class may be verified by wild_verify<4, 64>.
// The keys come from the last 16 characters whatever the length.
inline bool wild_primer_fits(const std::string &s, int k, size_t maxL = 32) {
  if (s.size() < 16 || s.size() > maxL || maxL > 64) return false;
  for (unsigned char ch : s) if (!wild_class_of(ch)) return false;
  const int kk = k == 2 ? 2 : 1;
  for (int c = 0; c < sub_ncombos(kk); ++c) if (wild_pair_keys(s, sub_fa(kk, c), sub_fb(kk, c)) > WILD_MAX_PAIR_KEYS) return false;
  return true;
}
// the field pair a primer is entered under at k = 0: the one of (0,1), (2,3) with fewer keys
inline int wild_registered_pair(const std::string &s) { return wild_pair_keys(s, 2, 3) < wild_pair_keys(s, 0, 1) ? 1 : 0; }

// The class as a whole: no field pair's run entries (the sum of the expanded keys of the primers entered under it) exceed
// WILD_MAX_ENTRIES.  Every primer passes wild_primer_fits(s, k).
inline bool wild_entries_fit(const std::vector<std::string> &pats, int k) {
  const int kk = k == 2 ? 2 : 1;
  for (int c = 0; c < sub_ncombos(kk); ++c) {
    size_t entries = 0;
    for (const std::string &s : pats) if (k != 0 || wild_registered_pair(s) == c) entries += wild_pair_keys(s, sub_fa(kk, c), sub_fb(kk, c));
    if (entries > WILD_MAX_ENTRIES) return false;
  }
  return true;
}

struct WildIndex {
  int k = 0, ncombos = 0;          // ncombos: 6 at k = 2, otherwise (0,1) and (2,3)
  int fa[6] = {}, fb[6] = {};
  bool ascii = false;
  std::vector<uint32_t> bitmap;    // [field pair][SHORT_BM_WORDS]: bit = a key in the cross product of some primer's classes
  std::vector<uint32_t> rows;      // [field pair][SHORT_ROWS]: first entry of the key's run in runs
  std::vector<uint64_t> runs;      // by pair and key: class index of the primer | class word << 32
  std::vector<size_t> entries;     // [field pair] run entries
  std::vector<uint8_t> reg;        // per primer: the pair it is entered under at k = 0 (0xff: under every pair)
  std::vector<uint8_t> pat_class;  // per primer row_bytes bytes: one nibble per character (A,C,G,T = bits 0..3), character i in byte i / 2, even i low
  size_t row_bytes = 16;           // 16, or 32 when the class holds a primer of 33..64 characters (every row of the class is then wide)
};

// The class word of a primer for field pair (a, b): four bits per base -- the set of stream codes the base accepts --
// for the eight bases of the two fields outside the key, lower field first (what wild_others cuts out of a window).
inline uint32_t wild_class_word(const std::string &s, int a, int b, bool ascii) {
  const size_t L = s.size();
  uint32_t w = 0;
  int at = 0;
  for (int f = 0; f < 4; ++f) {
    if (f == a || f == b) continue;
    for (int i = 0; i < 4; ++i, ++at) w |= wild_code_class(wild_class_of((unsigned char)s[L - 16 + 4 * f + i]), ascii) << (4 * at);
  }
  return w;
}

// every key of primer s in field pair (a, b), in the stream's packing
inline void wild_pair_key_list(const std::string &s, int a, int b, bool ascii, std::vector<uint32_t> *keys) {
  const size_t L = s.size();
  keys->assign(1, 0u);
  int at = 0;
  for (int f : {a, b}) for (int i = 0; i < 4; ++i, ++at) {
    const uint32_t cls = wild_code_class(wild_class_of((unsigned char)s[L - 16 + 4 * f + i]), ascii);
    std::vector<uint32_t> next;
    next.reserve(keys->size() * 4);
    for (uint32_t pre : *keys) for (uint32_t code = 0; code < 4; ++code) if ((cls >> code) & 1u) next.push_back(pre | (code << (2 * at)));
    keys->swap(next);
  }
}

// Build the index of primers that all pass wild_primer_fits(s, k, 64).  Returns "" or why the class is refused as a whole
// (some field pair's run entries exceed WILD_MAX_ENTRIES): *out is then unspecified.  The key index -- bitmaps, rows, run
// entries, reg -- does not depend on the primers' lengths; the rows of pat_class are as wide as the class's longest primer
// asks (row_bytes): a class without a primer of 33..64 characters gets the tables it always had.
inline std::string wild_build_index(const std::vector<std::string> &pats, int k, bool ascii, WildIndex *out) {
  WildIndex &x = *out;
  x = WildIndex();
  if (k < 0 || k > 2) return "pm_wild_sub_scan is built for k = 0, 1 and 2";
  const int kk = k == 2 ? 2 : 1;
  x.k = k; x.ncombos = sub_ncombos(kk); x.ascii = ascii;
  for (int c = 0; c < x.ncombos; ++c) { x.fa[c] = sub_fa(kk, c); x.fb[c] = sub_fb(kk, c); }
  const size_t m = pats.size();
  x.reg.assign(m, 0xff);
  for (size_t j = 0; j < m; ++j) {
    if (!wild_primer_fits(pats[j], k, 64)) return "primer the wild class does not take";
    if (pats[j].size() > 32) x.row_bytes = 32;
  }
  x.pat_class.assign(m * x.row_bytes, 0);
  for (size_t j = 0; j < m; ++j) {
    if (k == 0) x.reg[j] = (uint8_t)wild_registered_pair(pats[j]);
    for (size_t i = 0; i < pats[j].size(); ++i) x.pat_class[j * x.row_bytes + i / 2] |= (uint8_t)(wild_class_of((unsigned char)pats[j][i]) << (4 * (i & 1)));
  }
  x.bitmap.assign((size_t)x.ncombos * SHORT_BM_WORDS, 0);
  x.rows.assign((size_t)x.ncombos * SHORT_ROWS, 0);
  x.entries.assign(x.ncombos, 0);
  std::vector<uint32_t> keys;
  for (int c = 0; c < x.ncombos; ++c)
    for (size_t j = 0; j < m; ++j) if (x.reg[j] == 0xff || x.reg[j] == c) x.entries[c] += wild_pair_keys(pats[j], x.fa[c], x.fb[c]);
  size_t total = 0;
  for (int c = 0; c < x.ncombos; ++c) {
    if (x.entries[c] > WILD_MAX_ENTRIES) return "more than " + std::to_string(WILD_MAX_ENTRIES) + " run entries in a field pair of the wild class";
    total += x.entries[c];
  }
  x.runs.assign(total, 0);
  size_t base = 0;
  for (int c = 0; c < x.ncombos; ++c) {
    uint32_t *rows = &x.rows[(size_t)c * SHORT_ROWS];
    for (size_t j = 0; j < m; ++j) {                                 // counting sort by key, as short_key_index
      if (x.reg[j] != 0xff && x.reg[j] != c) continue;
      wild_pair_key_list(pats[j], x.fa[c], x.fb[c], ascii, &keys);
      for (uint32_t key : keys) { x.bitmap[(size_t)c * SHORT_BM_WORDS + (key >> 5)] |= 1u << (key & 31u); ++rows[key + 1]; }
    }
    rows[0] = (uint32_t)base;
    for (int key = 0; key < 65536; ++key) rows[key + 1] += rows[key];
    std::vector<uint32_t> fill(rows, rows + 65536);
    for (size_t j = 0; j < m; ++j) {
      if (x.reg[j] != 0xff && x.reg[j] != c) continue;
      const uint64_t word = wild_class_word(pats[j], x.fa[c], x.fb[c], ascii);
      wild_pair_key_list(pats[j], x.fa[c], x.fb[c], ascii, &keys);
      for (uint32_t key : keys) x.runs[fill[key]++] = (uint64_t)j | (word << 32);
    }
    base += x.entries[c];
  }
  return "";
}

}  // namespace pm
