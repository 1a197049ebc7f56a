// pm_edits.h -- the two exact stages of the edit plan (-k with filter_bitvec / shift_and_inexact), each a template on
// its width: the k-error automaton run per seed record (edits_verify<ROW>: pm_seed.hip's pm_edits_verify on 32-bit rows,
// pm_edits_verify_wide on 64-bit rows) and the banded DP per cluster (device_editdist<MAXL>: pm_cluster.hip's
// pm_cluster_dp for patterns of up to 32 or up to 64 characters).  Both compile with a plain C++ compiler as well:
// tests/test_long_edits_host.py checks them against plain restatements.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "pm_verify.h"

#if defined(__HIPCC__)
#define PM_EFN __device__
#else
#define PM_EFN inline
#endif

namespace pm {

namespace {

// ---- edits (-k with filter_bitvec / shift_and_inexact semantics) --------------------------------
// The candidates of these engines are the end positions at which the Wu-Manber k-error automaton
// (shift_and_inexact.cc:249-352) has the pattern's last bit set.  A seed (3 clean pieces under one
// of the displacement patterns) says "pattern pi ends within +-k of p+1"; the automaton is then
// run for that one pattern over the maxlen+k+4 stream characters in front of p+3, from the empty state
// (its last bit depends on the last L+k characters only), and the ends p-1..p+3 are read off.
// ROW = the automaton's rows: uint32_t for patterns of up to 32 characters, uint64_t for up to 64.
// Record (edit_record_fill): masks of A,C,G,T over the pattern positions (bit i = character i), four ROWs | L | id --
// 32 bytes with 32-bit rows, 64 with 64-bit rows (the rest is padding).
// maxlen: at least the pattern's length, the same on every lane of a wave (the tile's longest pattern, or the wave's).
// Args: text, n, pat_codes (the records), edits (k), ascii, eos_code.
// Returns one nibble per end p-1+d, d = 0..4: level+1, or 0.
template <typename ROW, typename Args>
PM_VFN uint32_t edits_verify(const Args &a, int maxlen, int64_t p, uint32_t pi, uint32_t *pid) {
  static_assert(sizeof(ROW) == 4 || sizeof(ROW) == 8, "rows of 32 or 64 bits");
  const uint4 *rec = reinterpret_cast<const uint4 *>(a.pat_codes + (size_t)pi * (8 * sizeof(ROW)));
  ROW MA, MC, MG, MT;
  int L;
  if constexpr (sizeof(ROW) == 4) {
    const uint4 M = rec[0], r = rec[1];
    MA = M.x; MC = M.y; MG = M.z; MT = M.w;
    L = (int)(r.x & 0xffu); *pid = r.y;
  } else {
    const uint4 m0 = rec[0], m1 = rec[1], r = rec[2];
    MA = (ROW)m0.x | ((ROW)m0.y << 32); MC = (ROW)m0.z | ((ROW)m0.w << 32);
    MG = (ROW)m1.x | ((ROW)m1.y << 32); MT = (ROW)m1.z | ((ROW)m1.w << 32);
    L = (int)(r.x & 0xffu); *pid = r.y;
  }
  const int k = a.edits;
  // characters [base + skip, p+3) are consumed: maxlen+k+4 of them, so that every end p-1..p+3 has
  // its L+k characters; an earlier start only adds true history
  const int nch = (maxlen + k + 4 + 15) >> 4;                     // wave-uniform number of 16-byte pieces
  const int skip = 16 * nch - (maxlen + k + 4);                   // wave-uniform: leading characters of the first piece not needed
  const int64_t base = p + 3 - 16 * (int64_t)nch;
  ROW R0 = 0, R1 = 0, R2 = 0;
  if (base + skip <= 0) { R1 = 1u; R2 = 3u; }                     // true start of the stream: l prefix bits in row l (:162-164)
  const ROW last = (ROW)1 << (L - 1);
  uint32_t res = 0;
#pragma unroll 1
  for (int c = 0; c < nch; ++c) {
    const int64_t off = base + 16 * c;
    uint4 v;
    const bool inside = off >= 0 && off + 16 <= a.n;
    if (inside) __builtin_memcpy(&v, a.text + off, 16);
    else {
      uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const int64_t q = off + b;
        const uint32_t x = (q >= 0 && q < a.n) ? (uint32_t)a.text[q] << (8 * (b & 3)) : 0u;
        if (b < 4) w[0] |= x; else if (b < 8) w[1] |= x; else if (b < 12) w[2] |= x; else w[3] |= x;
      }
      v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
    }
    const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      if (c == 0 && b < skip) continue;                            // wave-uniform
      const uint32_t ch = (vw[b >> 2] >> (8 * (b & 3))) & 0xffu;
      ROW U;
      if (a.ascii) U = ch == 'A' ? MA : ch == 'C' ? MC : ch == 'G' ? MG : ch == 'T' ? MT : (ROW)0;
      else {
        const ROW u01 = (ch & 1u) ? MC : MA, u23 = (ch & 1u) ? MT : MG;
        U = ch > 3u ? (ROW)0 : ((ch & 2u) ? u23 : u01);
      }
      // one character (pm_bitpar.hip step<K, true>): substitution, insertion and deletion terms
      const ROW x0 = (R0 << 1) | 1u, m1 = x0 | R0;
      ROW n0 = x0 & U;
      const ROW x1 = (R1 << 1) | 1u;
      ROW n1 = (x1 & U) | m1 | (n0 << 1) | 1u | n0;
      ROW n2 = 0;
      if (k >= 2) {                                                // wave-uniform
        const ROW m2 = x1 | R1, x2 = (R2 << 1) | 1u;
        n2 = (x2 & U) | m2 | (n1 << 1) | 1u | n1;
      }
      bool live = true;
      if (!inside) { const int64_t t = off + b; live = t >= 0 && t < a.n; }   // only at the stream's ends
      if ((int)ch == a.eos_code) { n0 = 0; n1 = 0; n2 = 0; }      // EOS clears every row
      if (live) { R0 = n0; R1 = n1; R2 = n2; }
      if (c == nch - 1 && b >= 11) {                               // ends p-1 .. p+3 = after the characters p-2 .. p+2
        const uint32_t lvl = (R0 & last) ? 1u : (R1 & last) ? 2u : (R2 & last) ? 3u : 0u;
        if (live) res |= lvl << (4 * (b - 11));
      }
    }
  }
  return res;
}

// ---- filter_bitvec with edits: the banded DP per cluster -------------------------------------------
// editdist_alignment::align (reference pattern_alignment.cc:117-705) as pm_align.cpp restates it,
// on stream codes (the patterns of the seed family are A,C,G,T, so code equality is character
// equality), band cells in thread-private memory as (value, flags) bytes.  Returns true and
// (*end, *value) when the alignment's value is <= k.
// MAXL = the longest pattern the instance takes, 32 or 64 (a handle with patterns of 33..64 characters on the edit plan,
// DESIGN.md 4.11); a cluster spans at most DP_MAXDELTA ends and k <= 3.
constexpr int DP_MAXDELTA = 10, DP_MAXW = DP_MAXDELTA + 2 * 3 + 2;
enum : uint8_t { D_EQ = 2, D_SUB = 8, D_INS = 16, D_DEL = 32, D_VIOL = 64, D_END = 128 };

// The stream window (<= MAXL + 3 + DP_MAXDELTA + 1 characters) and the pattern are copied into LDS first (byte i of
// thread t at i * DP_THREADS + t): read cell by cell from global memory, a dependent byte load per cell, they were
// most of the kernel's time.  dp_win(MAXL): that window, rounded up to 16 (48, 80).
constexpr int DP_THREADS = 256;
constexpr int dp_win(int maxl) { return (maxl + 3 + DP_MAXDELTA + 1 + 15) / 16 * 16; }
template <int MAXL>
PM_EFN bool device_editdist(const uint8_t *text, int64_t n, int64_t end, int64_t end2, const uint8_t *pat, int L,
                            int lconst, int rconst, int k, bool indels, int eos, int64_t *out_end, int *out_value,
                            uint8_t *swin, uint8_t *spat) {
  static_assert(MAXL == 32 || MAXL == 64, "patterns of up to 32 or up to 64 characters");
  constexpr int WIN = dp_win(MAXL);
  uint8_t dp[(MAXL + 1) * DP_MAXW], fl[(MAXL + 1) * DP_MAXW];
  const int viol = 5 * k + 1, b = indels ? k : 0;
  int64_t ws = 0;
  if (end > (int64_t)L + k) ws = end - L - k;                      // :137-139
  const int buflen = (int)(end2 - ws), delta = (int)(end2 - end);
  const int W = delta + 2 * b + 2;
  auto at = [&](int p, int t) { return p * W + (t - (p - b)); };
  for (int i = 0; i <= buflen && i < WIN; ++i) { const int64_t q = ws + i; swin[i * DP_THREADS] = q >= 0 && q < n ? text[q] : (uint8_t)0; }
  for (int i = 0; i < L; ++i) spat[i * DP_THREADS] = pat[i];
  pat = nullptr;
  auto tch = [&](int t) -> int { return (int)swin[(buflen - t) * DP_THREADS]; };   // win[buflen - t]
  int lbexact = 0, rbexact = L + 1;                                // :230-233
  if (lconst > 0) rbexact = L + 1 - lconst;
  if (rconst > 0) lbexact = rconst;
  dp[at(0, 0)] = 0; fl[at(0, 0)] = D_END;
  for (int p = 1, ub = b < L ? b : L; p <= ub; ++p) {              // column 0 (:253-268)
    const int i = at(p, 0);
    if (!indels || p < lbexact || p >= rbexact) { dp[i] = (uint8_t)viol; fl[i] = D_VIOL; }
    else { dp[i] = (uint8_t)(dp[at(p - 1, 0)] + 1); fl[i] = D_DEL; }
  }
  for (int t = 1, ub = buflen < delta + b ? buflen : delta + b; t <= ub; ++t) {   // row 0 (:276-294)
    const int i = at(0, t);
    if (t <= delta) { dp[i] = 0; fl[i] = D_END; }
    else if (!indels || lbexact > 0) { dp[i] = (uint8_t)viol; fl[i] = D_VIOL; }
    else { dp[i] = (uint8_t)(dp[at(0, t - 1)] + 1); fl[i] = D_INS; }
  }
  for (int p = 1; p <= L; ++p) {                                   // :296-437
    const int lb = p - b > 1 ? p - b : 1, ub = buflen < p + delta + b ? buflen : p + delta + b;
    const int pc = spat[(L - p) * DP_THREADS];
    const bool zone_sub = (p <= lbexact || p >= rbexact), zone_ins = (p < lbexact || p >= rbexact);
    int rowmin = viol;
    for (int t = lb; t <= ub; ++t) {
      const int tc = tch(t);
      int v, v1; uint8_t ac;
      if (tc == pc) { v = dp[at(p - 1, t - 1)]; ac = D_EQ; }
      else if (tc == eos || zone_sub) { v = viol; ac = D_VIOL; }
      else { v = dp[at(p - 1, t - 1)] + 1; ac = D_SUB; }
      if (tc == eos || !indels || t <= lb || zone_ins) {
        if (viol < v) { v = viol; ac = D_VIOL; }
      } else {
        v1 = dp[at(p, t - 1)] + 1;
        if (v1 < v) { v = v1; ac = D_INS; } else if (v1 == v) ac |= D_INS;
      }
      if (!indels || t >= ub || zone_sub) {
        if (viol < v) { v = viol; ac = D_VIOL; }
      } else {
        v1 = dp[at(p - 1, t)] + 1;
        if (v1 < v) { v = v1; ac = D_DEL; } else if (v1 == v) ac |= D_DEL;
      }
      const int i = at(p, t);
      dp[i] = (uint8_t)v; fl[i] = ac;
      rowmin = rowmin < v ? rowmin : v;
    }
    if (rowmin > k) return false;                                  // :425-436
  }
  int best = L - b < buflen ? L - b : buflen;                      // :443-475
  if (best < 0) best = 0;
  int bestval = dp[at(L, best)];
  for (int c = best + 1, ub = buflen < L + delta + b ? buflen : L + delta + b; c <= ub; ++c) {
    const int v = dp[at(L, c)];
    if (v < bestval || (v <= bestval && (fl[at(L, c)] & (D_EQ | D_SUB)))) { bestval = v; best = c; }
  }
  int p = L, t = best;
  if (t < p - b || t > p + b + delta) return false;                // :482-490
  int last = 0;                                                    // 0 none, 1 eq, 2 sub, 3 ins, 4 del
  for (int guard = 0; guard < 4 * (MAXL + DP_MAXW); ++guard) {     // traceback (:514-590): only the end column matters here
    const uint8_t ac = fl[at(p, t)];
    if (ac & D_END) break;
    const bool match = ac & (D_EQ | D_SUB), sub = ac & D_SUB, ins = ac & D_INS, del = ac & D_DEL;
    if (match && !((last == 3 && ins) || (last == 4 && del))) {
      --p; --t;
      if ((ac & D_EQ) && !(last == 2 && sub)) last = 1;
      else if (sub) last = 2;
    } else if (del) { --p; last = 4; }
    else if (ins) { --t; last = 3; }
    else if (ac & D_VIOL) { p = 0; t = 0; break; }
    else return false;
  }
  *out_end = end2 - t;                                             // :603-610
  *out_value = bestval;
  return bestval <= k;
}

}  // namespace

}  // namespace pm
