// pm_short_tables.h -- the key index of the kernels for patterns of 16..19 characters (pm_short.hip): per field pair of
// the patterns' last 16 bases an exact bitmap of the 16-bit keys, and the patterns sorted by key behind an offset table.
// Plain C++: tests/test_short_tables_host.py compiles it with the host compiler and checks it against a restatement.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pm_verify.h"

namespace pm {

constexpr int SHORT_BM_WORDS = 2048;                // 2^16 key bits per field pair
constexpr int SHORT_ROWS = 65536 + 1;               // offset table rows per field pair (+ the end of the last run)

struct ShortKeyIndex {
  std::vector<uint32_t> bitmap;    // [field pair][SHORT_BM_WORDS]: bit = 16-bit key of some pattern
  std::vector<uint32_t> rows;      // [field pair][SHORT_ROWS]: first entry of the key's run in order (pair c starts at c * m)
  std::vector<uint32_t> order;     // [field pair][m]: pattern indices by key, patterns of one key in increasing index
};

// tails: the last 16 bases of m patterns, 2 bits each; field pair c = (fa[c], fb[c]), its key = sub_key
inline ShortKeyIndex short_key_index(const uint32_t *tails, size_t m, int npairs, const int *fa, const int *fb) {
  ShortKeyIndex x;
  x.bitmap.assign((size_t)npairs * SHORT_BM_WORDS, 0);
  x.rows.assign((size_t)npairs * SHORT_ROWS, 0);
  x.order.assign((size_t)npairs * m, 0);
  for (int c = 0; c < npairs; ++c) {
    uint32_t *rows = &x.rows[(size_t)c * SHORT_ROWS];
    for (size_t j = 0; j < m; ++j) {                                 // counting sort by key: rows[key] = first entry of the key's run
      const uint32_t key = sub_key(tails[j], fa[c], fb[c]);
      x.bitmap[(size_t)c * SHORT_BM_WORDS + (key >> 5)] |= 1u << (key & 31u);
      ++rows[key + 1];
    }
    rows[0] = (uint32_t)((size_t)c * m);
    for (int key = 0; key < 65536; ++key) rows[key + 1] += rows[key];
    std::vector<uint32_t> fill(rows, rows + 65536);
    for (size_t j = 0; j < m; ++j) x.order[fill[sub_key(tails[j], fa[c], fb[c])]++] = (uint32_t)j;
  }
  return x;
}

}  // namespace pm
