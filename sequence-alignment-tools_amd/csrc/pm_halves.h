// pm_halves.h -- exact_halves -k with patterns of 33..64 characters: what the halves plan knows of a
// half of 16..32 characters.  The 64-byte record of a wide tile (half_record_fill_wide), the exact test of a whole half on
// the raw stream against it (half_match_wide: pm_half_verify_wide and the HALVES && WIDE instance of pm_seed_scan), and
// the slot of the second kind of pm_half_scan<true> (half_slot_wide / half_slot_test: the half's bases in front of its
// ten-base key, on the packed bases the lane carries).  All of it compiles with a plain C++ compiler as well:
// tests/test_long_halves_host.py checks it against byte loops.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "pm_verify.h"

namespace pm {

namespace {

// Record of a half in a wide tile (a tile that holds a half of a pattern of 33..64 characters; every half of such a
// tile has this record, the short ones too), 64 bytes:
//   [0, 32)  stream codes, right-aligned: the half's last character at byte 31, zeros in front
//   [32, 40) the partner half at 2 bits per base, base i at bits 2i (up to 32 bases)
//   40, 41, 42  L, partner length, side (0 = partner to the right of the seed, 1 = to the left); 43: zero
//   [44, 48) inner id
//   [48, 64) zero
constexpr int HALF_ROW_WIDE = 64, HALF_MAX_WIDE = 32;
inline void half_record_fill_wide(const uint8_t *codes, int L, uint64_t part64, int plen, int side, uint32_t id, uint8_t *rec) {
  memset(rec, 0, HALF_ROW_WIDE);
  memcpy(rec + HALF_MAX_WIDE - L, codes, (size_t)L);
  memcpy(rec + 32, &part64, 8);
  rec[40] = (uint8_t)L; rec[41] = (uint8_t)plen; rec[42] = (uint8_t)side;
  memcpy(rec + 44, &id, 4);
}

struct HalfRecWide { int L, plen, side; uint32_t id; uint64_t part; };
PM_VFN HalfRecWide half_record_info(const uint8_t *rec) {
  uint32_t w[4];
  memcpy(w, rec + 32, 16);
  HalfRecWide r;
  r.part = ((uint64_t)w[1] << 32) | w[0];
  r.L = (int)(w[2] & 0xffu); r.plen = (int)((w[2] >> 8) & 0xffu); r.side = (int)((w[2] >> 16) & 0xffu);
  r.id = w[3];
  return r;
}

// The half of record `rec` (L characters) ends at stream index p: its codes equal text[p + 1 - L, p].  The codes are all
// A,C,G,T, so an N or an end-of-sequence character inside the window rejects by itself; a half that would begin before
// index 0 is no seed.  Reads text[p - 31, p] where that lies inside [0, n), byte by byte elsewhere (the stream's first 31
// characters), and nothing outside [0, n).
PM_VFN bool half_match_wide(const uint8_t *text, int64_t n, const uint8_t *rec, int L, int64_t p) {
  if (p + 1 - L < 0 || p >= n) return false;
  uint64_t t[4] = {0, 0, 0, 0}, c[4];
  if (p >= 31) memcpy(t, text + p - 31, 32);
  else
    for (int i = 0; i <= (int)p; ++i) t[(31 - i) >> 3] |= (uint64_t)text[p - i] << (8 * ((31 - i) & 7));
  memcpy(c, rec, 32);
  uint64_t diff = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int q = 0; q < 4; ++q) {
    // bytes 8q .. 8q+7 of the window; the half covers bytes [32 - L, 32)
    const int first = 32 - L - 8 * q;                                // bytes of this word in front of the half
    const uint64_t m = first <= 0 ? ~0ull : (first >= 8 ? 0ull : (~0ull << (8 * first)));
    diff |= (t[q] ^ c[q]) & m;
  }
  return diff == 0;
}

// Slot of the second kind (pm_half_scan<true>): a half of a pattern of 33..64 characters has 16..32 characters and lies
// inside the 48 bases p-31 .. p+16 a queue entry carries.  slot.x = the bases p-25 .. p-10 of an occurrence that ends at
// p -- the up to 16 in front of the ten-base key -- at 2 bits per base, base p-25+i at bits 2i; the slot's 5-bit field
// holds how many of them belong to the half: cnt = min(L - 10, 16), the LAST cnt of the 16.  code2(ch) = the 2-bit word
// of a pattern character (seed_build's base2).
template <typename Code2>
inline uint32_t half_slot_wide(const char *s, int L, Code2 code2, int *cnt_out) {
  const int cnt = L - 10 < 16 ? L - 10 : 16;
  uint32_t x = 0;
  for (int j = 0; j < cnt; ++j) x |= (uint32_t)code2((unsigned char)s[L - 11 - j]) << (2 * (15 - j));
  *cnt_out = cnt;
  return x;
}
// d0, d1 = the carried bases p-31 .. p-16 and p-15 .. p (base i of a word at bits 2i).  Exact on A,C,G,T; the 2-bit words
// alias an N (or an end-of-sequence character) to a base, so a window that is no occurrence can pass -- an occurrence
// never fails.
PM_VFN bool half_slot_test(uint32_t slotx, int cnt, uint32_t d0, uint32_t d1) {
  const uint32_t x = (d0 >> 12) | (d1 << 20);                        // bases p-25 .. p-10
  const uint32_t mask = cnt >= 16 ? 0xffffffffu : (0xffffffffu << (2 * (16 - cnt)));
  return ((x ^ slotx) & mask) == 0;
}

}  // namespace

}  // namespace pm
