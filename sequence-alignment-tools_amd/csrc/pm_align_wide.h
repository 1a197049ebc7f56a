// pm_align_wide.h -- the per-record computation of pm_align_hits_wide_kernel (pm_align.hip): the caller's
// re-alignment with indels for patterns of 33..64 characters.  It is editdist_alignment::align with end2 == end as
// pm_align.cpp's editdist_align states it -- the banded fill, the row-minimum exit, the best-column rule and the
// traceback with its "do not split an indel run" preference -- on bytes behind a small accessor: columns of the block's
// LDS in the kernel (byte i of lane t at i * 64 + t), plain arrays in a host program.  The kernel and
// tests/test_long_align_host.py compile this text; the narrow kernel (patterns of up to 32 characters) keeps its own.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PM_WFN __host__ __device__ __forceinline__
#else
#define PM_WFN inline
#endif

namespace pm {

constexpr int ALW_MAXL = 64, ALW_MAXK = 3;         // patterns of up to 64 characters, k of up to 3
constexpr int ALW_WIN = ALW_MAXL + ALW_MAXK + 1;   // window characters
constexpr int ALW_LANES = 64;                      // lanes that share an LDS block (the kernel's block is one wave)
constexpr int ALW_NONE = 0x7fffffff;               // INT32_MAX: constraint violation / no alignment
enum : uint8_t { AW_EQ = 2, AW_WEQ = 4, AW_SUB = 8, AW_INS = 16, AW_DEL = 32, AW_VIOL = 64, AW_END = 128 };

// W = band cells per row: 2k + 2 holds the band of k (instances 4, 6, 8 for k = 1, 2, 3)
template <int W> constexpr int alw_lane_bytes() { return ALW_WIN + ALW_MAXL + (ALW_MAXL + 1) * W + 2 * W; }

// storage of one record: window, pattern, traceback flags of the (L + 1) x W band, two rolling rows of values
template <int W>
struct WideLds {                                   // the record's column of a block of alw_lane_bytes<W>() * ALW_LANES bytes
  uint8_t *base;
  PM_WFN WideLds(uint8_t *block, int lane) : base(block + lane) {}
  PM_WFN uint8_t &win(int q) const { return base[q * ALW_LANES]; }
  PM_WFN uint8_t &pat(int q) const { return base[(ALW_WIN + q) * ALW_LANES]; }
  PM_WFN uint8_t &fl(int c) const { return base[(ALW_WIN + ALW_MAXL + c) * ALW_LANES]; }
  PM_WFN uint8_t &row(int c) const { return base[(ALW_WIN + ALW_MAXL + (ALW_MAXL + 1) * W + c) * ALW_LANES]; }
};
template <int W>
struct WideArrays {                                // the same bytes as plain arrays
  uint8_t w[ALW_WIN], p[ALW_MAXL], f[(ALW_MAXL + 1) * W], r[2 * W];
  uint8_t &win(int q) { return w[q]; }
  uint8_t &pat(int q) { return p[q]; }
  uint8_t &fl(int c) { return f[c]; }
  uint8_t &row(int c) { return r[c]; }
};

struct WideOptions { int k, eos, wc, tn; };        // (indels: always)
struct WideAlignment { int64_t start, end; int value, editdist; };

// iupac_compatible(w, c) (reference util.cc:164-183) from the 128 masks of align_tables()
PM_WFN bool wide_iupac_pair(const uint32_t *mask, int w, int c) {
  if (w >= 128 || c == 0) return false;
  const bool upper = w >= 'A' && w <= 'Z', lower = w >= 'a' && w <= 'z';
  if (upper) return c >= 'A' && c <= 'Z' && ((mask[w] >> (c - 'A')) & 1u);
  if (lower) return c >= 'a' && c <= 'z' && ((mask[w] >> (c - 'a')) & 1u);
  return false;
}

// One record: pattern pat[0 .. L), 33 <= L <= ALW_MAXL (any 1 <= L <= ALW_MAXL computes the same), 1 <= o.k and
// 2 * o.k + 2 <= W, exact zones lconst / rconst, the hit's end.  tchar(q) is the character at stream index q >= 0 (beyond
// the stream: that of code 0).  put_op receives the alignment string's characters from the pattern's start on, put_tx the
// matching text.  Returns whether there is an alignment; without one *r is the "none" record (start 0, end, INT32_MAX,
// value 0), put_tx was not called and what put_op received is to be dropped.
template <int W, typename Store, typename TextAt, typename PutOp, typename PutTx>
PM_WFN bool align_wide_record(Store s, const WideOptions &o, const uint32_t *mask, const uint8_t *pat, int L, int lconst, int rconst,
                              int64_t end, TextAt tchar, PutOp put_op, PutTx put_tx, WideAlignment *r) {
  r->start = 0; r->end = end; r->editdist = ALW_NONE; r->value = 0;
  // Row p = last p pattern characters, column t = last t window characters; cell (p, t) of the band at offset t - p + b of row p.
  const int k = o.k, viol = 5 * k + 1, b = k, eos = o.eos;
  const int64_t ws = end > (int64_t)L + k ? end - L - k : 0;        // pattern_alignment.cc:137-139
  int buflen = (int)(end - ws);
  if (buflen < 0) buflen = 0;
  if (buflen > ALW_WIN - 1) buflen = ALW_WIN - 1;
  for (int q = 0; q < buflen; ++q) s.win(q) = (uint8_t)tchar(ws + q);
  for (int q = 0; q < L; ++q) s.pat(q) = pat[q];
  auto fl = [&](int p, int t) -> uint8_t & { return s.fl(p * W + (t - p + b)); };
  auto dp = [&](int p, int t) -> uint8_t & { return s.row((p & 1) * W + (t - p + b)); };
  int lbexact = 0, rbexact = L + 1;                                 // :230-233
  if (lconst > 0) rbexact = L + 1 - lconst;
  if (rconst > 0) lbexact = rconst;
  dp(0, 0) = 0; fl(0, 0) = AW_END;
  for (int t = 1, ub = buflen < b ? buflen : b; t <= ub; ++t) {     // row 0 (:276-294), t > delta == 0
    if (lbexact > 0) { dp(0, t) = (uint8_t)viol; fl(0, t) = AW_VIOL; }
    else { dp(0, t) = (uint8_t)(dp(0, t - 1) + 1); fl(0, t) = AW_INS; }
  }
  for (int p = 1, ub = b < L ? b : L; p <= ub; ++p) {               // column 0 (:253-268); (p, 0) is not in reach of the rows written before row p + 1
    if (p < lbexact || p >= rbexact || s.pat(L - p) == eos) { dp(p, 0) = (uint8_t)viol; fl(p, 0) = AW_VIOL; }
    else { dp(p, 0) = (uint8_t)(dp(p - 1, 0) + 1); fl(p, 0) = AW_DEL; }
  }
  for (int p = 1; p <= L; ++p) {                                    // :296-437
    const int lb = p - b > 1 ? p - b : 1, ub = buflen < p + b ? buflen : p + b;
    const int pc = s.pat(L - p);
    const bool zone_sub = (p <= lbexact || p >= rbexact), zone_ins = (p < lbexact || p >= rbexact);
    int rowmin = viol;
    for (int t = lb; t <= ub; ++t) {
      const int tc = s.win(buflen - t);
      int v, v1; uint8_t ac;
      if (tc == pc) { v = dp(p - 1, t - 1); ac = AW_EQ; }
      else if (o.wc && wide_iupac_pair(mask, pc, tc) && (tc != 'N' || o.tn)) { v = dp(p - 1, t - 1); ac = AW_WEQ; }   // :317-319
      else if (tc == eos || pc == eos || zone_sub) { v = viol; ac = AW_VIOL; }
      else { v = dp(p - 1, t - 1) + 1; ac = AW_SUB; }
      if (tc == eos || pc == eos || t <= lb || zone_ins) {
        if (viol < v) { v = viol; ac = AW_VIOL; }
      } else {
        v1 = dp(p, t - 1) + 1;
        if (v1 < v) { v = v1; ac = AW_INS; } else if (v1 == v) ac |= AW_INS;
      }
      if (pc == eos || t >= ub || zone_sub) {
        if (viol < v) { v = viol; ac = AW_VIOL; }
      } else {
        v1 = dp(p - 1, t) + 1;
        if (v1 < v) { v = v1; ac = AW_DEL; } else if (v1 == v) ac |= AW_DEL;
      }
      dp(p, t) = (uint8_t)v; fl(p, t) = ac;
      rowmin = rowmin < v ? rowmin : v;
    }
    if (rowmin > k) return false;                                   // :425-436
  }
  int best = L - b < buflen ? L - b : buflen;                       // :443-475
  if (best < 0) best = 0;
  int bestval = dp(L, best);
  for (int c = best + 1, ub = buflen < L + b ? buflen : L + b; c <= ub; ++c) {
    const int v = dp(L, c);
    if (v < bestval || (v <= bestval && (fl(L, c) & (AW_EQ | AW_WEQ | AW_SUB)))) { bestval = v; best = c; }
  }
  int p = L, t = best;
  if (t < p - b || t > p + b) return false;                         // :482-490
  int last = 0;                                                     // 0 none, 1 eq, 2 weq, 3 sub, 4 ins, 5 del, 6 viol
  int nsub = 0, nins = 0, ndel = 0, nviol = 0;
  for (int guard = 0; guard < 2 * (ALW_MAXL + W) + 2; ++guard) {    // traceback (:514-590): at most L + buflen steps
    const uint8_t ac = fl(p, t);
    if (ac & AW_END) break;
    const bool match = ac & (AW_EQ | AW_WEQ | AW_SUB), wcf = ac & AW_WEQ, sub = ac & AW_SUB, ins = ac & AW_INS, del = ac & AW_DEL;
    if (match && !((last == 4 && ins) || (last == 5 && del) || (last == 2 && !wcf && (ins || del)))) {
      --p; --t;
      if ((ac & AW_EQ) && !((last == 2 && wcf) || (last == 3 && sub))) last = 1;
      else if (wcf) last = 2;
      else if (sub) last = 3;
      if (last == 3) ++nsub;
    } else if (del) { --p; last = 5; ++ndel; }
    else if (ins) { --t; last = 4; ++nins; }
    else if (ac & AW_VIOL) { p = 0; t = 0; last = 6; ++nviol; }
    else return false;
    put_op(last == 1 ? '|' : last == 2 ? '+' : last == 3 ? '*' : last == 4 ? '^' : last == 5 ? 'v' : '!');
  }
  r->start = end - best;                                            // :603-610
  r->end = end - t;
  r->value = bestval;
  r->editdist = nviol ? ALW_NONE : nsub + nins + ndel;
  for (int64_t q = r->start; q < r->end; ++q) put_tx((char)s.win((int)(q - ws)));
  return true;
}

}  // namespace pm
