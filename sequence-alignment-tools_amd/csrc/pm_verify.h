// pm_verify.h -- the exact stage of the substitution plans, shared by pm_pair.hip (patterns of 20..32 characters: tail of
// 20 bases, four fields of five) and pm_short.hip (patterns of 16..19 characters: tail of 16 bases, four fields of four),
// the exact stage of the Bloom plan (seed_verify: pm_seed.hip, rows of 32 or 64 characters),
// the window arithmetic of pm_short_sub_scan, the class arithmetic and the exact stage of the wild class (wild_others,
// wild_verify: DESIGN.md 4.13, tests/test_wild_class_host.py), and the way records leave a verify kernel (pair_emit, verify_staged: the
// loop both pm_pair_verify and pm_short_sub_verify are).  All but those two compiles with a plain C++ compiler as well:
// tests/test_short_sub_host.py, tests/test_long_sub_host.py and tests/test_long_exact_host.py check it against plain
// restatements.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/pm_gpu.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PM_VFN __device__ __host__ __forceinline__
#else                                                 // a plain C++ compiler: the host check (tests/test_short_sub_host.py)
#define PM_VFN inline
namespace pm { struct uint4 { uint32_t x, y, z, w; }; }
#endif

namespace pm {

namespace {

PM_VFN int pop32(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(x);
#else
  return __builtin_popcount(x);
#endif
}

// substitutions between two strings of 2-bit symbols
PM_VFN int sym_distance(uint32_t x) { return pop32((x | (x >> 1)) & 0x55555555u); }

// the per-character verdicts of a window of CW characters: one bit each
template <int CW> struct verify_mask { typedef uint32_t type; };
template <> struct verify_mask<64> { typedef uint64_t type; };
PM_VFN int pop_mask(uint32_t x) { return pop32(x); }
PM_VFN int pop_mask(uint64_t x) { return pop32((uint32_t)x) + pop32((uint32_t)(x >> 32)); }

// Exact part of the verify (second kernel): (window ending at p, pattern pi) agree on this combo's key
// and are within k substitutions on the rest of the packed window; count mismatches on the raw stream
// codes over the whole pattern (N = mismatch, EOS = reject) and report -- once: only through the first
// combo of the plan whose two fields are clean.
// FW = bases per field: the plan looks at the pattern's last 4 * FW bases.  CW = characters a pattern's row of pat_codes
// holds, 32 or 64 (a wide tile of the pair plan, patterns of up to 64 characters: DESIGN.md 4.9): the verdicts are CW bits,
// and a row of pat_zone is CW / 32 dwords, low dword first.  Args: the kernel's argument block (text, n, k, eos_code,
// ncombos, fa, fb, pat_len, pat_id, pat_codes, pat_zone, viol_level).
// Returns whether (p, pi) is a candidate this combo reports; *hh is then its record.
template <int FW, int CW = 32, typename Args>
PM_VFN bool pair_verify(const Args &a, int combo, int64_t p, uint32_t pi, pm_hit *hh) {
  static_assert(FW == 4 || FW == 5, "fields of four or five bases");
  static_assert(CW == 32 || CW == 64, "rows of 32 or 64 characters");
  typedef typename verify_mask<CW>::type mask_t;
  constexpr int NW = CW / 4, NV = CW / 16;                          // dwords, 16-byte loads of a row
  const int L = a.pat_len[pi];
  const int64_t start = p + 1 - L;
  if (start < 0) return false;
  // all CW pattern codes and the CW stream bytes from `start` at once (every load independent of the
  // others: this kernel is a chain of dependent loads as it is), per-byte verdicts by SWAR
  const uint4 *pcv = reinterpret_cast<const uint4 *>(a.pat_codes + (size_t)pi * CW);
  uint4 pc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) pc[v] = pcv[v];
  uint32_t tw[NW];
  if (start + CW <= a.n) {
    uint4 t[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) __builtin_memcpy(&t[v], a.text + start + 16 * v, 16);
#pragma unroll
    for (int v = 0; v < NV; ++v) { tw[4 * v] = t[v].x; tw[4 * v + 1] = t[v].y; tw[4 * v + 2] = t[v].z; tw[4 * v + 3] = t[v].w; }
  } else {                                            // the last bytes of the stream (a pattern shorter than its row: often)
#pragma unroll
    for (int d = 0; d < NW; ++d) {
      tw[d] = 0;
      for (int b = 0; b < 4; ++b) { const int64_t q = start + 4 * d + b; if (q < a.n) tw[d] |= (uint32_t)a.text[q] << (8 * b); }
    }
  }
  uint32_t pcw[NW];
#pragma unroll
  for (int v = 0; v < NV; ++v) { pcw[4 * v] = pc[v].x; pcw[4 * v + 1] = pc[v].y; pcw[4 * v + 2] = pc[v].z; pcw[4 * v + 3] = pc[v].w; }
  const uint32_t eb = (uint32_t)(a.eos_code & 0xff) * 0x01010101u;
  mask_t mism = 0, eos = 0;                           // bit i: stream byte i differs from the pattern / is EOS
#pragma unroll
  for (int d = 0; d < NW; ++d) {
    const uint32_t x = tw[d] ^ pcw[d], z = tw[d] ^ eb;
    const uint32_t y = (x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
    const uint32_t e = ~(z | ((z & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
    mism |= (mask_t)(((y >> 7) & 1u) | ((y >> 14) & 2u) | ((y >> 21) & 4u) | ((y >> 28) & 8u)) << (4 * d);
    eos |= (mask_t)(((e >> 7) & 1u) | ((e >> 14) & 2u) | ((e >> 21) & 4u) | ((e >> 28) & 8u)) << (4 * d);
  }
  const mask_t lenmask = L >= CW ? ~(mask_t)0 : (((mask_t)1 << L) - 1u);   // (a shift by the mask's width is undefined)
  mism &= lenmask;
  if (a.eos_code >= 0 && (eos & lenmask)) return false;   // EOS inside the window: never a candidate
  int ham = pop_mask(mism);                           // N (or any other code) = mismatch
  if (ham > a.k) return false;
  // exact-base constraints (pattern_alignment.cc:320-323: a substitution inside an exact zone is a
  // constraint violation, the verify fails)
  mask_t zone = a.pat_zone[(size_t)pi * (CW / 32)];
  if (CW == 64) zone |= (mask_t)((uint64_t)a.pat_zone[(size_t)pi * (CW / 32) + (CW / 32 - 1)] << (CW - 32));
  if (mism & zone) {
    if (a.viol_level <= 0) return false;
    ham = a.viol_level;
  }
  const uint32_t tail = (uint32_t)(mism >> (L - 4 * FW));   // the bases the plan looks at
  uint32_t dirty = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) if ((tail >> (FW * j)) & ((1u << FW) - 1u)) dirty |= 1u << j;
  int first = -1;
  for (int c = 0; c < a.ncombos && first < 0; ++c)
    if (!((dirty >> a.fa[c]) & 1u) && !((dirty >> a.fb[c]) & 1u)) first = c;
  if (first != combo) return false;
  const int half = L / 2;                             // (<= 32 < the width of a 64-bit mask)
  const bool left_clean = (mism & (((mask_t)1 << half) - 1u)) == 0, right_clean = (mism >> half) == 0;
  hh->end = p + 1; hh->pid = a.pat_id[pi]; hh->k = (uint8_t)ham;
  hh->aux[0] = (uint8_t)((left_clean ? 1 : 0) | (right_clean ? 2 : 0)); hh->aux[1] = hh->aux[2] = 0;
  return true;
}

// Exact stage of the Bloom plan (pm_seed.hip: verify_exact, verify_exact_wide): (window ending at p, pattern pi) passed
// the packed-distance test on the pattern's last Lw bases; count mismatches on the raw stream codes over the whole
// pattern (N = mismatch, EOS = reject) and report -- once: only through the combo made of the first r clean pieces
// (mlo, mhi: the caller's combo as window bits, two per base).
// CW = characters a pattern's row of pat_codes holds: 32, or 64 in a wide tile (patterns of up to 64 characters at
// k = 0); the verdicts are CW bits.  Four stream bytes against four pattern codes per step, per-byte
// verdicts by SWAR.  Rolled on purpose: the function must stay small in registers, or the callers' allocation suffers
// (DESIGN.md 4.1).  The stream is read inside [start, min(start + 4 * ceil(L / 4), n)) and nowhere else.
// Args: text, n, k, r, Lw, pb, eos_code, pat_len, pat_id, pat_codes.
// Returns whether (p, pi) is a candidate this combo reports; *ham is then its distance and *flags its clean-half flags
// (seed_record makes the record of them: the kernels do that behind the list's counter, as they always did).
template <int CW = 32, typename Args>
PM_VFN bool seed_verify(const Args &a, uint32_t mlo, uint32_t mhi, int64_t p, uint32_t pi, int *ham_out, uint32_t *flags) {
  static_assert(CW == 32 || CW == 64, "rows of 32 or 64 characters");
  typedef typename verify_mask<CW>::type mask_t;
  const int L = a.pat_len[pi];
  const int64_t start = p + 1 - L;
  if (start < 0) return false;
  const uint32_t *pc = reinterpret_cast<const uint32_t *>(a.pat_codes + (size_t)pi * CW);
  const uint32_t eb = (uint32_t)(a.eos_code & 0xff) * 0x01010101u;
  mask_t mism = 0, eos = 0;                           // bit i: stream byte i differs from the pattern / is EOS
#pragma unroll 1
  for (int d = 0; 4 * d < L; ++d) {
    const int64_t off = start + 4 * d;
    uint32_t tw = 0;
    if (off + 4 <= a.n) __builtin_memcpy(&tw, a.text + off, 4);
    else
      for (int b = 0; off + b < a.n; ++b) tw |= (uint32_t)a.text[off + b] << (8 * b);   // last bytes of the stream
    const uint32_t x = tw ^ pc[d], z = tw ^ eb;
    const uint32_t y = (x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
    const uint32_t e = ~(z | ((z & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
    mism |= (mask_t)(((y >> 7) & 1u) | ((y >> 14) & 2u) | ((y >> 21) & 4u) | ((y >> 28) & 8u)) << (4 * d);
    eos |= (mask_t)(((e >> 7) & 1u) | ((e >> 14) & 2u) | ((e >> 21) & 4u) | ((e >> 28) & 8u)) << (4 * d);
  }
  const mask_t lenmask = L >= CW ? ~(mask_t)0 : (((mask_t)1 << L) - 1u);   // (a shift by the mask's width is undefined)
  mism &= lenmask;
  if (a.eos_code >= 0 && (eos & lenmask)) return false;   // EOS inside the window: never a candidate
  const int ham = pop_mask(mism);                     // N (or any other code) = mismatch
  if (ham > a.k) return false;
  const int half = L / 2, m = a.k + a.r;              // (half <= 32 < the width of a 64-bit mask; 16 at CW = 32)
  const bool left_clean = (mism & (((mask_t)1 << half) - 1u)) == 0, right_clean = (mism >> half) == 0;
  uint32_t dirty = 0;                                 // pieces (of the last Lw bases) with a mismatch
  const uint32_t sm = (uint32_t)(mism >> (L - a.Lw)), pmask = (1u << a.pb) - 1u;
  for (int j = 0; j < m; ++j)
    if ((sm >> (j * a.pb)) & pmask) dirty |= 1u << j;
  // report once: only through the combo made of the first r clean pieces
  uint64_t first = 0;
  const uint64_t field = (1ull << (2 * a.pb)) - 1ull;
  for (int j = 0, t = 0; j < m && t < a.r; ++j)
    if (!(dirty >> j & 1)) { first |= field << (2 * a.pb * j); ++t; }
  if (first != (((uint64_t)mhi << 32) | mlo)) return false;
  *ham_out = ham; *flags = (left_clean ? 1u : 0u) | (right_clean ? 2u : 0u);
  return true;
}
template <typename Args>
PM_VFN pm_hit seed_record(const Args &a, int64_t p, uint32_t pi, int ham, uint32_t flags) {
  pm_hit hh;
  hh.end = p + 1; hh.pid = a.pat_id[pi]; hh.k = (uint8_t)ham;
  hh.aux[0] = (uint8_t)flags; hh.aux[1] = hh.aux[2] = 0;
  return hh;
}

// ---- window arithmetic of pm_short_sub_scan (pm_short.hip) ----------------------------------------
// The plan's field pairs in the order that decides who reports: all six at k = 2, (0,1) and (2,3) at k = 1 (one
// substitution leaves the first two or the last two fields clean) -- the pair plan's.
constexpr int sub_ncombos(int k) { return k == 2 ? 6 : 2; }
constexpr int sub_fa(int k, int c) { return k == 2 ? (c < 3 ? 0 : (c < 5 ? 1 : 2)) : 2 * c; }
constexpr int sub_fb(int k, int c) { return k == 2 ? (c < 3 ? c + 1 : (c < 5 ? c - 1 : 3)) : 2 * c + 1; }
// A lane's 16 windows end at the positions pbase + j, pbase a multiple of 16: window j = the 16 bases up to pbase + j,
// 2 bits each, from the stream words w1 (bases pbase - 16 .. pbase - 1) and w2 (pbase .. pbase + 15).
PM_VFN uint32_t sub_window(uint32_t w1, uint32_t w2, uint32_t j) {
  return (uint32_t)((((uint64_t)w2 << 32) | w1) >> (2u * (j + 1u)));
}
// 16-bit key of field pair (a, b): the fields are the window word's bytes
PM_VFN uint32_t sub_key(uint32_t W, int a, int b) { return ((W >> (8 * a)) & 0xffu) | (((W >> (8 * b)) & 0xffu) << 8); }
// <= k substitutions on the two fields outside the key, P = the pattern's last 16 bases: the key fields of W and P are
// equal (the run was found through the key), so the distance of the whole words is the distance of the other two fields
PM_VFN bool sub_others_within(uint32_t W, uint32_t P, int k) { return sym_distance(W ^ P) <= k; }

// ---- the wild class: pm_wild_sub_scan / pm_wild_sub_verify (pm_short.hip) ---------
// Primers with IUPAC ambiguity letters compared by class.  A window's eight bases outside field pair (a, b), 2 bits each:
// the lower of the two other fields in bits 0..7, the higher in bits 8..15.
PM_VFN uint32_t wild_others(uint32_t W, int a, int b) {
  uint32_t o = 0;
  int at = 0;
#pragma unroll
  for (int f = 0; f < 4; ++f) if (f != a && f != b) { o |= ((W >> (8 * f)) & 0xffu) << (8 * at); ++at; }
  return o;
}
// <= k of those eight bases outside their class: `word` holds four bits per base, bit c = the base accepts stream code c
// (pm_wild_tables.h wild_class_word).  Every code becomes the one bit of its nibble; a base matches when that bit is set.
PM_VFN int wild_others_mismatches(uint32_t others, uint32_t word) {
  uint32_t x = others & 0xffffu;
  x = (x | (x << 8)) & 0x00ff00ffu; x = (x | (x << 4)) & 0x0f0f0f0fu; x = (x | (x << 2)) & 0x33333333u;   // code j in the low bits of nibble j
  const uint32_t lo = x & 0x11111111u, hi = (x >> 1) & 0x11111111u;
  const uint32_t onehot = (~hi & ~lo & 0x11111111u) | ((~hi & lo) << 1) | ((hi & ~lo) << 2) | ((hi & lo) << 3);
  return 8 - pop32(onehot & word);
}
PM_VFN bool wild_others_within(uint32_t others, uint32_t word, int k) { return wild_others_mismatches(others, word) <= k; }

// The exact stage of the wild class: pair_verify with the per-byte verdict replaced -- a stream byte is a mismatch when it
// is no base (code >= 4 after the raw stream's bytes are mapped to 0..3: N, any other letter) or when its bit is not set in
// the primer's class nibble (pat_class: 16 bytes per row of 32 characters, character i in byte i / 2, even i low; bit q =
// "ACGT"[q]).  Everything else is pair_verify's: EOS inside the window and start < 0 reject, the last bytes of the stream
// are read one by one, zones and viol_level, "reported only through the first combo of the plan whose two fields are
// clean", the clean-half flags, the record.  At k = 0 the combo must be the one the primer is entered under (pat_reg).
// Args: text, n, k, eos_code, ascii, ncombos, fa, fb, pat_len, pat_id, pat_class, pat_reg, pat_zone, viol_level.
//
// CW = characters a row holds: 32, or 64 for a class that holds a primer of 33..64 characters -- rows of
// pat_class are then 32 bytes, rows of pat_zone two dwords, low dword first, and the verdicts 64 bits (verify_mask<CW>, as
// pair_verify<5, 64>).  One body for both: the row is judged in groups of 32 characters -- one uint4 of class nibbles and
// two 16-byte stream reads per group, or, where the group's 32 bytes do not fit in front of n, the bytes below n one by one --
// and everything behind the verdicts is written once on the mask type.  The stream is read inside [start, min(start + CW, n)).
template <int FW = 4, int CW = 32, typename Args>
PM_VFN bool wild_verify(const Args &a, int combo, int64_t p, uint32_t pi, pm_hit *hh) {
  static_assert(FW == 4 && (CW == 32 || CW == 64), "fields of four bases, rows of 32 or 64 characters");
  typedef typename verify_mask<CW>::type mask_t;
  const int L = a.pat_len[pi];
  const int64_t start = p + 1 - L;
  if (start < 0) return false;
  const uint4 *pcv = reinterpret_cast<const uint4 *>(a.pat_class + (size_t)pi * (CW / 2));
  mask_t mism = 0, eos = 0;                           // bit i: stream byte i is outside the class of character i / is EOS
#pragma unroll
  for (int g = 0; g < CW / 32; ++g) {
    const uint4 pc = pcv[g];
    const uint32_t pcw[4] = {pc.x, pc.y, pc.z, pc.w};
    const int64_t from = start + 32 * g;
    uint32_t tw[8];
    if (from + 32 <= a.n) {
      uint4 t[2];
#pragma unroll
      for (int v = 0; v < 2; ++v) __builtin_memcpy(&t[v], a.text + from + 16 * v, 16);
#pragma unroll
      for (int v = 0; v < 2; ++v) { tw[4 * v] = t[v].x; tw[4 * v + 1] = t[v].y; tw[4 * v + 2] = t[v].z; tw[4 * v + 3] = t[v].w; }
    } else {                                          // the last bytes of the stream
#pragma unroll
      for (int d = 0; d < 8; ++d) {
        tw[d] = 0;
        for (int b = 0; b < 4; ++b) { const int64_t q = from + 4 * d + b; if (q < a.n) tw[d] |= (uint32_t)a.text[q] << (8 * b); }
      }
    }
    uint32_t m32 = 0, e32 = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const uint32_t ch = (tw[i / 4] >> (8 * (i & 3))) & 0xffu;
      uint32_t code = ch;                             // A,C,G,T = 0..3; anything else >= 4
      if (a.ascii) code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
      const uint32_t cls = (pcw[i / 8] >> (4 * (i & 7))) & 15u;
      if (code >= 4u || !((cls >> code) & 1u)) m32 |= 1u << i;
      if ((int)ch == a.eos_code) e32 |= 1u << i;
    }
    mism |= (mask_t)m32 << (32 * g);
    eos |= (mask_t)e32 << (32 * g);
  }
  const mask_t lenmask = L >= CW ? ~(mask_t)0 : (((mask_t)1 << L) - 1u);   // (a shift by the mask's width is undefined)
  mism &= lenmask;
  if (a.eos_code >= 0 && (eos & lenmask)) return false;   // EOS inside the window: never a candidate
  int ham = pop_mask(mism);
  if (ham > a.k) return false;
  mask_t zone = a.pat_zone[(size_t)pi * (CW / 32)];
  if (CW == 64) zone |= (mask_t)((uint64_t)a.pat_zone[(size_t)pi * (CW / 32) + (CW / 32 - 1)] << (CW - 32));
  if (mism & zone) {                                  // a substitution inside an exact zone (pair_verify)
    if (a.viol_level <= 0) return false;
    ham = a.viol_level;
  }
  if (a.k == 0) {
    if (combo != (int)a.pat_reg[pi]) return false;
  } else {
    const uint32_t tail = (uint32_t)(mism >> (L - 4 * FW));   // the bases the plan looks at (shifted in the mask's width: L - 16 reaches 48)
    uint32_t dirty = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) if ((tail >> (FW * j)) & ((1u << FW) - 1u)) dirty |= 1u << j;
    int first = -1;
    for (int c = 0; c < a.ncombos && first < 0; ++c)
      if (!((dirty >> a.fa[c]) & 1u) && !((dirty >> a.fb[c]) & 1u)) first = c;
    if (first != combo) return false;
  }
  const int half = L / 2;                             // (<= 32 < the width of a 64-bit mask; <= 16 at CW = 32)
  const bool left_clean = (mism & (((mask_t)1 << half) - 1u)) == 0, right_clean = (mism >> half) == 0;
  hh->end = p + 1; hh->pid = a.pat_id[pi]; hh->k = (uint8_t)ham;
  hh->aux[0] = (uint8_t)((left_clean ? 1 : 0) | (right_clean ? 2 : 0)); hh->aux[1] = hh->aux[2] = 0;
  return true;
}

#if defined(__HIPCC__)
// Output of the verify kernels.  The record list's end is ONE counter for the whole grid and same-address atomics
// serialise (~10 ns each under load), so a workgroup collects its records in LDS and appends them in batches: one atomic
// per ~1500 records instead of one per wave and call (hit-dense streams -- tandem repeats, 0.4 candidates per base --
// spent most of this kernel waiting for that counter).  Called by whichever lanes of a wave are executing together.
// Args: out, counter, cap.
constexpr int VSTAGE = 2048;                                        // records a workgroup stages (32 KiB)
struct VerifyStage { pm_hit *rec; uint32_t *fill, *valid; };        // LDS: records, reserved slots, first slot that was refused

template <typename Args>
__device__ __forceinline__ void pair_emit(const Args &a, const VerifyStage &vs, bool ok, const pm_hit &hh) {
  const unsigned long long bal = __ballot(ok);
  if (bal == 0) return;
  const int leader = __ffsll((long long)bal) - 1;
  const int lane = threadIdx.x & 63;
  const uint32_t cnt = (uint32_t)__popcll(bal), mine = (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
  uint32_t pos = 0;
  if (lane == leader) pos = atomicAdd(vs.fill, cnt);
  pos = __builtin_amdgcn_readlane(pos, leader);
  if (pos + cnt <= (uint32_t)VSTAGE) {
    if (ok) vs.rec[pos + mine] = hh;
    return;
  }
  // no room (a workgroup whose suspects give thousands of records in one trip): this batch goes straight to the list;
  // every later reservation of the trip is refused as well (fill stays above VSTAGE), the flush takes the slots in front
  if (lane == leader) atomicMin(vs.valid, pos);
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(a.counter, (unsigned long long)cnt);
  const uint32_t blo = __builtin_amdgcn_readlane((uint32_t)base, leader), bhi = __builtin_amdgcn_readlane((uint32_t)(base >> 32), leader);
  if (ok) {
    const unsigned long long o = (((unsigned long long)bhi << 32) | blo) + (unsigned long long)mine;
    if (o < a.cap) a.out[o] = hh;
  }
}

// The loop of a verify kernel: suspect i of n to thread i of the grid, trip by trip, and the records through the
// workgroup's stage.  body(i, vs, &hh) judges suspect i (i < n) and returns whether hh is a record of it; it may hand
// further records of the same suspect to pair_emit itself.  Called by every thread of the workgroup.
// Args: out, counter, cap.
template <typename Args, typename Body>
__device__ __forceinline__ void verify_staged(const Args &a, unsigned long long n, Body &&body) {
  __shared__ pm_hit s_rec[VSTAGE];
  __shared__ unsigned long long s_base;
  __shared__ uint32_t s_fill, s_valid, s_full;
  const VerifyStage vs = {s_rec, &s_fill, &s_valid};
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  if (threadIdx.x == 0) { s_fill = 0; s_valid = (uint32_t)VSTAGE; }
  __syncthreads();
  // the staged records join the list: one atomic for all of them (block-uniform call)
  auto flush = [&]() __attribute__((always_inline)) {
    const uint32_t cnt = min(s_fill, s_valid);
    __syncthreads();
    if (threadIdx.x == 0) { s_base = cnt ? atomicAdd(a.counter, (unsigned long long)cnt) : 0ull; s_fill = 0; s_valid = (uint32_t)VSTAGE; }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += blockDim.x) if (s_base + i < a.cap) a.out[s_base + i] = s_rec[i];
    __syncthreads();
  };
  for (unsigned long long base = (unsigned long long)blockIdx.x * blockDim.x; base < n; base += stride) {   // block-uniform trip count
    const unsigned long long i = base + threadIdx.x;
    pm_hit hh;
    const bool have = i < n && body(i, vs, &hh);
    pair_emit(a, vs, have, hh);                                       // (every lane is here)
    __syncthreads();
    if (threadIdx.x == 0) s_full = s_fill > (uint32_t)(VSTAGE - 512);   // one thread decides: a wave that runs ahead into the next trip moves s_fill
    __syncthreads();
    if (s_full) flush();
  }
  flush();
}
#endif

}  // namespace

}  // namespace pm
