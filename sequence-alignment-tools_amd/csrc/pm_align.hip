// pm_align.hip -- the caller's per-hit re-alignment and its tally on the device.
//
// primer_match re-aligns every final hit (reference primer_match.cc:1135-1151): exact_alignment for k == 0,
// exact_wc_alignment for k == 0 with -w/-W, otherwise editdist_alignment(end, end, k, ...) with its traceback
// (pattern_alignment.cc:117-705), and with -c adds one to count[pattern][editdist] until the pattern's total reaches
// -M (primer_match.cc:1123-1247).  pm_align_hits does the first part on host threads, record by record (pm_align.cpp
// editdist_align + pm_api.cpp align_hits_impl); here the same computation runs where the final hits already are:
//
//   pm_align_hits_kernel   one lane per 16-byte hit record: the banded DP on characters (stream codes mapped through
//                          the handle's table, patterns as the caller added them), traceback, pm_alignment and --
//                          optionally -- the alignment string and the matching text, or one 64-bit tally key
//   pm_align_hits_wide_kernel   the same banded DP for patterns of 33..64 characters (PM_LONG_ALIGN), over the list of records
//                          the kernel above left on the device; its per-record code is pm_align_wide.h
//   pm_tally_flags/decide/add   the tally over the sorted keys  pattern index(22) | end(39) | distance code(3)
//
// Everything a lane indexes at run time lives in LDS, byte i of lane t at i * AL_THREADS + t (a runtime-indexed
// per-thread array would go to scratch memory): the window (<= L + k characters), the pattern, the traceback flags of
// the (L + 1) x (2k + 2) band and two rolling rows of values.  No lane reads another lane's bytes, so there is no
// barrier in the kernel.
#include <hipcub/hipcub.hpp>

#include <cstring>

#include "pm_align_wide.h"
#include "pm_internal.h"
#include "pm_iupac.h"

namespace pm {

namespace {

constexpr int AL_W = 2 * AL_MAXK + 2;                 // band cells per row (delta == 0: the end is fixed)
constexpr int AL_WIN = AL_MAXL + AL_MAXK + 1;         // window characters
enum : uint8_t { A_EQ = 2, A_WEQ = 4, A_SUB = 8, A_INS = 16, A_DEL = 32, A_VIOL = 64, A_END = 128 };
constexpr int ED_NONE = 0x7fffffff;                   // INT32_MAX: constraint violation / no alignment

__device__ __forceinline__ unsigned long long wave_slot(unsigned long long *counter) {   // one atomic per wave
  const unsigned long long bal = __ballot(1);
  const int lane = threadIdx.x & 63, leader = __ffsll((long long)bal) - 1;
  unsigned long long base = 0;
  if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(bal));
  base = __shfl(base, leader);
  return base + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
}

// iupac_compatible(w, c) (reference util.cc:164-183) from the mask table align_tables() builds out of pm_iupac.h
__device__ __forceinline__ bool iupac_pair(const uint32_t *mask, int w, int c) {
  if (w >= 128 || c == 0) return false;
  const bool upper = w >= 'A' && w <= 'Z', lower = w >= 'a' && w <= 'z';
  if (upper) return c >= 'A' && c <= 'Z' && ((mask[w] >> (c - 'A')) & 1u);
  if (lower) return c >= 'a' && c <= 'z' && ((mask[w] >> (c - 'a')) & 1u);
  return false;
}

__device__ __forceinline__ uint64_t tally_key(uint32_t idx, int64_t end, int code) {
  return ((uint64_t)idx << 42) | (((uint64_t)end & ((1ull << 39) - 1ull)) << 3) | (uint64_t)code;
}

// ctr[0]: records handed to the host (patterns beyond the device limit), ctr[1]: records with an unknown pattern id,
// ctr[2]: strings that did not fit `stride`
__global__ __launch_bounds__(AL_THREADS) void pm_align_hits_kernel(AlignDevice a, const uint8_t *text, int64_t ntext, const pm_hit *hits,
                                                                   const unsigned long long *d_count, size_t n_upper, pm_alignment *out,
                                                                   char *ops, char *txt, size_t stride, uint64_t *keys,
                                                                   pm_hit *hostq_hits, uint64_t *hostq_idx, unsigned long long *ctr) {
  __shared__ uint8_t swin[AL_WIN * AL_THREADS], spat[AL_MAXL * AL_THREADS], sfl[(AL_MAXL + 1) * AL_W * AL_THREADS], srow[2 * AL_W * AL_THREADS];
  const size_t i = blockIdx.x * (size_t)AL_THREADS + threadIdx.x;
  size_t n = n_upper;
  if (d_count && (size_t)*d_count < n) n = (size_t)*d_count;
  if (i >= n) return;
  const int lane = threadIdx.x;
  const pm_hit h = hits[i];
  const uint8_t *ch = a.tab;
  const uint32_t *mask = (const uint32_t *)(a.tab + 256);
  const int k = a.k;
  pm_alignment r;
  r.start = 0; r.end = h.end; r.editdist = ED_NONE; r.value = 0;
  int nops = 0, ntxt = 0;
  bool fits = true;
  char *myops = ops ? ops + i * stride : nullptr, *mytxt = ops ? txt + i * stride : nullptr;
  auto put_op = [&](char c) { if (myops) { if ((size_t)nops + 1 < stride) myops[nops] = c; else fits = false; ++nops; } };
  auto put_tx = [&](char c) { if (mytxt) { if ((size_t)ntxt + 1 < stride) mytxt[ntxt] = c; else fits = false; ++ntxt; } };
  auto tchar = [&](int64_t q) -> int { return (int)ch[q < ntext ? text[q] : (uint8_t)0]; };   // q >= 0; beyond the stream: code 0

  uint32_t lo = 0, hi = a.npat;                                     // first rank with ids_sorted[rank] >= pid
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a.ids_sorted[mid] < h.pid) lo = mid + 1; else hi = mid; }
  bool done = false, to_host = false;
  uint32_t idx = 0;
  if (lo >= a.npat || a.ids_sorted[lo] != h.pid) { atomicAdd(ctr + 1, 1ull); done = true; }
  else idx = a.perm[lo];
  const uint8_t *pat = a.pchars + (done ? 0 : a.poff[idx]);
  const int L = done ? 0 : (int)(a.poff[idx + 1] - a.poff[idx]);

  if (!done && k == 0 && !a.wc) {                                   // exact_alignment (pattern_alignment.cc:29-43): no text read
    r.start = h.end - L; r.editdist = 0;
    for (int q = 0; q < L; ++q) { put_op('|'); put_tx((char)pat[q]); }
    done = true;
  } else if (!done && k == 0) {                                     // exact_wc_alignment (pattern_alignment.cc:70-93)
    const int64_t st = h.end - L;
    int subs = 0;
    for (int q = 0; q < L; ++q) {
      const int64_t tp = st + q;
      const int tc = tp >= 0 ? tchar(tp) : 0, pc = pat[q];
      char op;
      if (tc == pc) op = '|';
      else if (pc && iupac_pair(mask, tc, pc) && (a.tn || tc != 'N')) op = '+';
      else { op = '*'; ++subs; }
      put_op(op); put_tx((char)tc);
    }
    r.start = st; r.editdist = subs;
    done = true;
  } else if (!done && !a.indels && k <= AL_MAXK && L > AL_MAXL && L <= AL_MAXL_SUB) {
    // Substitutions only (-K) and a pattern of 33..64 characters: the band has width zero (b = 0 below), the DP is the one
    // diagonal (p, p), and this lane walks it without the LDS arrays of the banded DP -- the cell rules of the loop below
    // with !indels: equal, wildcard-equal, violation (end of sequence, a substitution in an exact zone), substitution; a
    // row above k ends the DP with no alignment at all, and so does a window that does not fit in front of the hit's end.
    const int viol = 5 * k + 1, eos = a.eos;
    const int lconst = a.esb[idx], rconst = a.eeb[idx];
    int lbexact = 0, rbexact = L + 1;
    if (lconst > 0) rbexact = L + 1 - lconst;
    if (rconst > 0) lbexact = rconst;
    const int64_t st = h.end - L;
    bool alive = st >= 0;                                           // (buflen < L: row buflen + 1 has no cell)
    int v = 0;
    for (int p = 1; p <= L && alive; ++p) {                         // row p = the last p pattern characters, as in the banded DP
      const int tc = tchar(h.end - p), pc = pat[L - p];
      const bool zone_sub = (p <= lbexact || p >= rbexact);
      if (tc == pc) {}
      else if (a.wc && iupac_pair(mask, pc, tc) && (tc != 'N' || a.tn)) {}
      else if (tc == eos || pc == eos || zone_sub) v = viol;
      else v = v + 1;
      if (viol < v) v = viol;
      if (v > k) alive = false;
    }
    if (alive) {
      int nsub = 0;
      for (int q = 0; q < L; ++q) {                                 // the traceback runs from the pattern's first character on
        const int tc = tchar(st + q), pc = pat[q];
        char op;
        if (tc == pc) op = '|';
        else if (a.wc && iupac_pair(mask, pc, tc) && (tc != 'N' || a.tn)) op = '+';
        else { op = '*'; ++nsub; }
        put_op(op); put_tx((char)tc);
      }
      r.start = st; r.end = h.end; r.value = v; r.editdist = nsub;
    }
    done = true;
  } else if (!done && (L > AL_MAXL || k > AL_MAXK || L == 0)) {     // beyond the device limit: the host aligns this record
    to_host = true; done = true;
  }

  if (!done) {
    // editdist_alignment::align as pm_align.cpp editdist_align restates it, end2 == end (delta 0).  Row p = last p pattern
    // characters, column t = last t window characters; cell (p, t) of the band at offset t - p + b of row p.
    const int viol = 5 * k + 1, b = a.indels ? k : 0, eos = a.eos;
    const bool indels = a.indels != 0;
    const int64_t ws = h.end > (int64_t)L + k ? h.end - L - k : 0;  // :137-139
    int buflen = (int)(h.end - ws);
    if (buflen < 0) buflen = 0;
    if (buflen > AL_WIN - 1) buflen = AL_WIN - 1;
    const int lconst = a.esb[idx], rconst = a.eeb[idx];
    for (int q = 0; q < buflen; ++q) swin[q * AL_THREADS + lane] = (uint8_t)tchar(ws + q);
    for (int q = 0; q < L; ++q) spat[q * AL_THREADS + lane] = pat[q];
    auto fl = [&](int p, int t) -> uint8_t & { return sfl[(p * AL_W + (t - p + b)) * AL_THREADS + lane]; };
    auto dp = [&](int p, int t) -> uint8_t & { return srow[((p & 1) * AL_W + (t - p + b)) * AL_THREADS + lane]; };
    int lbexact = 0, rbexact = L + 1;                               // :230-233
    if (lconst > 0) rbexact = L + 1 - lconst;
    if (rconst > 0) lbexact = rconst;
    dp(0, 0) = 0; fl(0, 0) = A_END;
    for (int t = 1, ub = buflen < b ? buflen : b; t <= ub; ++t) {   // row 0 (:276-294), t > delta == 0
      if (!indels || lbexact > 0) { dp(0, t) = (uint8_t)viol; fl(0, t) = A_VIOL; }
      else { dp(0, t) = (uint8_t)(dp(0, t - 1) + 1); fl(0, t) = A_INS; }
    }
    for (int p = 1, ub = b < L ? b : L; p <= ub; ++p) {             // column 0 (:253-268); (p, 0) is not in reach of the rows written before row p + 1
      if (!indels || p < lbexact || p >= rbexact || spat[(L - p) * AL_THREADS + lane] == eos) { dp(p, 0) = (uint8_t)viol; fl(p, 0) = A_VIOL; }
      else { dp(p, 0) = (uint8_t)(dp(p - 1, 0) + 1); fl(p, 0) = A_DEL; }
    }
    bool alive = true;
    for (int p = 1; p <= L && alive; ++p) {                         // :296-437
      const int lb = p - b > 1 ? p - b : 1, ub = buflen < p + b ? buflen : p + b;
      const int pc = spat[(L - p) * AL_THREADS + lane];
      const bool zone_sub = (p <= lbexact || p >= rbexact), zone_ins = (p < lbexact || p >= rbexact);
      int rowmin = viol;
      for (int t = lb; t <= ub; ++t) {
        const int tc = swin[(buflen - t) * AL_THREADS + lane];
        int v, v1; uint8_t ac;
        if (tc == pc) { v = dp(p - 1, t - 1); ac = A_EQ; }
        else if (a.wc && iupac_pair(mask, pc, tc) && (tc != 'N' || a.tn)) { v = dp(p - 1, t - 1); ac = A_WEQ; }   // :317-319
        else if (tc == eos || pc == eos || zone_sub) { v = viol; ac = A_VIOL; }
        else { v = dp(p - 1, t - 1) + 1; ac = A_SUB; }
        if (tc == eos || pc == eos || !indels || t <= lb || zone_ins) {
          if (viol < v) { v = viol; ac = A_VIOL; }
        } else {
          v1 = dp(p, t - 1) + 1;
          if (v1 < v) { v = v1; ac = A_INS; } else if (v1 == v) ac |= A_INS;
        }
        if (!indels || pc == eos || t >= ub || zone_sub) {
          if (viol < v) { v = viol; ac = A_VIOL; }
        } else {
          v1 = dp(p - 1, t) + 1;
          if (v1 < v) { v = v1; ac = A_DEL; } else if (v1 == v) ac |= A_DEL;
        }
        dp(p, t) = (uint8_t)v; fl(p, t) = ac;
        rowmin = rowmin < v ? rowmin : v;
      }
      if (rowmin > k) alive = false;                                // :425-436
    }
    if (alive) {
      int best = L - b < buflen ? L - b : buflen;                   // :443-475
      if (best < 0) best = 0;
      int bestval = dp(L, best);
      for (int c = best + 1, ub = buflen < L + b ? buflen : L + b; c <= ub; ++c) {
        const int v = dp(L, c);
        if (v < bestval || (v <= bestval && (fl(L, c) & (A_EQ | A_WEQ | A_SUB)))) { bestval = v; best = c; }
      }
      int p = L, t = best;
      if (!(t < p - b || t > p + b)) {                              // :482-490
        int last = 0;                                               // 0 none, 1 eq, 2 weq, 3 sub, 4 ins, 5 del, 6 viol
        int nsub = 0, nins = 0, ndel = 0, nviol = 0;
        bool broken = false;
        for (int guard = 0; guard < 2 * (AL_MAXL + AL_W) + 2; ++guard) {   // traceback (:514-590)
          const uint8_t ac = fl(p, t);
          if (ac & A_END) break;
          const bool match = ac & (A_EQ | A_WEQ | A_SUB), wcf = ac & A_WEQ, sub = ac & A_SUB, ins = ac & A_INS, del = ac & A_DEL;
          if (match && !((last == 4 && ins) || (last == 5 && del) || (last == 2 && !wcf && (ins || del)))) {
            --p; --t;
            if ((ac & A_EQ) && !((last == 2 && wcf) || (last == 3 && sub))) last = 1;
            else if (wcf) last = 2;
            else if (sub) last = 3;
            if (last == 3) ++nsub;
          } else if (del) { --p; last = 5; ++ndel; }
          else if (ins) { --t; last = 4; ++nins; }
          else if (ac & A_VIOL) { p = 0; t = 0; last = 6; ++nviol; }
          else { broken = true; break; }
          put_op(last == 1 ? '|' : last == 2 ? '+' : last == 3 ? '*' : last == 4 ? '^' : last == 5 ? 'v' : '!');
        }
        if (!broken) {
          r.start = h.end - best;                                   // :603-610
          r.end = h.end - t;
          r.value = bestval;
          r.editdist = nviol ? ED_NONE : nsub + nins + ndel;
          for (int64_t q = r.start; q < r.end; ++q) put_tx((char)swin[(int)(q - ws) * AL_THREADS + lane]);
        } else nops = 0;
      }
    }
  }

  if (to_host) {
    const unsigned long long o = wave_slot(ctr);
    if (hostq_hits) hostq_hits[o] = h;
    if (hostq_idx) hostq_idx[o] = (uint64_t)i;
  }
  if (out && !to_host) out[i] = r;
  if (myops && !to_host) {
    myops[(size_t)nops + 1 <= stride ? nops : 0] = 0;
    mytxt[(size_t)ntxt + 1 <= stride ? ntxt : 0] = 0;
    if (!fits) atomicAdd(ctr + 2, 1ull);
  }
  if (keys) {
    const bool known = !(lo >= a.npat || a.ids_sorted[lo] != h.pid);
    keys[i] = (to_host || !known) ? TALLY_INVALID : tally_key(idx, h.end, (r.editdist < 0 || r.editdist > k) ? TALLY_BOGUS : r.editdist);
  }
}

// The banded DP for patterns of 33..64 characters (PM_LONG_ALIGN; a.indels != 0, 1 <= a.k and 2 * a.k + 2 <= W): one lane
// per record of the list pm_align_hits_kernel left on the device -- side_hits[j], the record's place side_idx[j] in the
// caller's arrays, ctr[0] of them -- through align_wide_record (pm_align_wide.h), on the lane's column of the block's
// LDS.  One instance per band width: W = 4, 6, 8 hold 25,600 / 34,176 / 42,752 bytes per block.  Results
// go where the narrow kernel would have put them; what this kernel cannot take either (more than 64 characters, an empty
// pattern) is compacted into rest_hits / rest_idx and counted in ctr[3].
static_assert(ALW_LANES == AL_THREADS && ALW_MAXL == AL_MAXL_WIDE && ALW_MAXK == AL_MAXK, "pm_align_wide.h and pm_internal.h disagree");
template <int W>
__global__ __launch_bounds__(AL_THREADS) void pm_align_hits_wide_kernel(AlignDevice a, const uint8_t *text, int64_t ntext, const pm_hit *side_hits,
                                                                        const uint64_t *side_idx, size_t n_upper, pm_alignment *out, char *ops, char *txt,
                                                                        size_t stride, uint64_t *keys, pm_hit *rest_hits, uint64_t *rest_idx,
                                                                        unsigned long long *ctr) {
  __shared__ uint8_t lds[alw_lane_bytes<W>() * AL_THREADS];
  const size_t j = blockIdx.x * (size_t)AL_THREADS + threadIdx.x;
  size_t n = n_upper;
  if ((size_t)ctr[0] < n) n = (size_t)ctr[0];
  if (j >= n) return;
  const pm_hit h = side_hits[j];
  const size_t i = (size_t)side_idx[j];
  const uint8_t *ch = a.tab;
  const uint32_t *mask = (const uint32_t *)(a.tab + 256);
  const int k = a.k;
  int nops = 0, ntxt = 0;
  bool fits = true;
  char *myops = ops ? ops + i * stride : nullptr, *mytxt = ops ? txt + i * stride : nullptr;
  auto put_op = [&](char c) { if (myops) { if ((size_t)nops + 1 < stride) myops[nops] = c; else fits = false; ++nops; } };
  auto put_tx = [&](char c) { if (mytxt) { if ((size_t)ntxt + 1 < stride) mytxt[ntxt] = c; else fits = false; ++ntxt; } };
  auto tchar = [&](int64_t q) -> int { return (int)ch[q < ntext ? text[q] : (uint8_t)0]; };   // q >= 0; beyond the stream: code 0

  uint32_t lo = 0, hi = a.npat;                                     // first rank with ids_sorted[rank] >= pid (the narrow kernel found it)
  while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a.ids_sorted[mid] < h.pid) lo = mid + 1; else hi = mid; }
  const bool known = lo < a.npat && a.ids_sorted[lo] == h.pid;
  const uint32_t idx = known ? a.perm[lo] : 0;
  const int L = known ? (int)(a.poff[idx + 1] - a.poff[idx]) : 0;
  if (L <= AL_MAXL || L > AL_MAXL_WIDE) {                           // not this kernel's either: the host aligns the record
    const unsigned long long o = wave_slot(ctr + 3);
    if (rest_hits) rest_hits[o] = h;
    if (rest_idx) rest_idx[o] = (uint64_t)i;
    return;
  }
  WideOptions opt;
  opt.k = k; opt.eos = a.eos; opt.wc = a.wc; opt.tn = a.tn;
  WideAlignment w;
  if (!align_wide_record<W>(WideLds<W>(lds, (int)threadIdx.x), opt, mask, a.pchars + a.poff[idx], L, a.esb[idx], a.eeb[idx], h.end, tchar, put_op, put_tx, &w))
    nops = 0;
  if (out) { pm_alignment r; r.start = w.start; r.end = w.end; r.editdist = w.editdist; r.value = w.value; out[i] = r; }
  if (myops) {
    myops[(size_t)nops + 1 <= stride ? nops : 0] = 0;
    mytxt[(size_t)ntxt + 1 <= stride ? ntxt : 0] = 0;
    if (!fits) atomicAdd(ctr + 2, 1ull);
  }
  if (keys) keys[i] = tally_key(idx, h.end, (w.editdist < 0 || w.editdist > k) ? TALLY_BOGUS : w.editdist);
}

// ---- the tally -------------------------------------------------------------------------------------------------
// Sorted keys put every pattern's hits of the range side by side in order of stream end.  The cap needs, per hit, the
// pattern's total so far (the sum of its tallies of the earlier ranges) plus the number of tallied hits before it in its
// run: a segmented inclusive sum (head flag in bit 63) over "this hit is not bogus".
constexpr uint64_t SEG_HEAD = 1ull << 63;
struct SegSum {
  __host__ __device__ __forceinline__ uint64_t operator()(uint64_t x, uint64_t y) const {
    return (y & SEG_HEAD) ? y : ((x & SEG_HEAD) | ((x + y) & ~SEG_HEAD));
  }
};

__global__ void pm_tally_flags(const uint64_t *keys, size_t n, uint64_t *v) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  const bool head = i == 0 || (keys[i - 1] >> 42) != (key >> 42);
  v[i] = (head ? SEG_HEAD : 0ull) | ((key != TALLY_INVALID && (int)(key & 7u) < TALLY_BOGUS) ? 1ull : 0ull);
}

// v[i]: the segmented sum on entry, the decision on return: 0 .. 3 tally under that distance, 4 bogus, 5 behind the cap, 6 no record
__global__ void pm_tally_decide(const uint64_t *keys, size_t n, uint64_t *v, int k, uint64_t max_count, const unsigned long long *counts) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t key = keys[i];
  if (key == TALLY_INVALID) { v[i] = 6; return; }
  const int code = (int)(key & 7u);
  uint64_t dec = (uint64_t)code;
  if (max_count) {
    const uint32_t idx = (uint32_t)(key >> 42);
    uint64_t rank = (v[i] & ~SEG_HEAD) - (code < TALLY_BOGUS ? 1u : 0u);
    for (int d = 0; d <= k; ++d) rank += counts[(size_t)idx * (k + 1) + d];
    if (rank >= max_count) dec = 5;
  }
  v[i] = dec;
}

// One block adds TALLY_ITEMS * 256 consecutive sorted keys: their (pattern, distance) pairs go into an LDS table that
// covers the first TALLY_SPAN patterns from the block's first one (a tandem repeat gives one pattern whole blocks of
// keys; uniform text gives a block hundreds of patterns with a few keys each, and what lies beyond the table are adds
// to as many different addresses), then one global add per nonzero table entry and per info counter.
constexpr int TALLY_ITEMS = 4, TALLY_SPAN = 256;
__global__ __launch_bounds__(256) void pm_tally_add(const uint64_t *keys, const uint64_t *dec, size_t n, int k, const uint32_t *idrank,
                                                    unsigned long long *counts, unsigned long long *info) {
  __shared__ uint32_t s_tab[TALLY_SPAN * 4];
  __shared__ uint32_t s_info[3];
  __shared__ unsigned long long s_first;
  const size_t base = blockIdx.x * (size_t)(TALLY_ITEMS * 256);
  for (int t = threadIdx.x; t < TALLY_SPAN * 4; t += 256) s_tab[t] = 0;
  if (threadIdx.x < 3) s_info[threadIdx.x] = 0;
  if (threadIdx.x == 0) s_first = ~0ull;
  __syncthreads();
  const uint32_t idx0 = (uint32_t)(keys[base] >> 42);               // (base < n: the grid is sized by n)
  for (int j = 0; j < TALLY_ITEMS; ++j) {
    const size_t i = base + (size_t)j * 256 + threadIdx.x;
    if (i >= n) break;
    const int d = (int)dec[i];
    if (d > 5) continue;
    const uint64_t key = keys[i];
    const uint32_t idx = (uint32_t)(key >> 42);
    if (d < TALLY_BOGUS) {
      const uint32_t off = idx - idx0;
      if (off < (uint32_t)TALLY_SPAN) atomicAdd(&s_tab[off * 4 + d], 1u);
      else atomicAdd(&counts[(size_t)idx * (k + 1) + d], 1ull);
      atomicAdd(&s_info[0], 1u);
    } else if (d == 5) atomicAdd(&s_info[1], 1u);
    else {
      atomicAdd(&s_info[2], 1u);
      const unsigned long long f = (((key >> 3) & ((1ull << 39) - 1ull)) << 22) | idrank[idx];   // smallest (end, id)
      atomicMin(&s_first, f);
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < TALLY_SPAN * 4; t += 256) {
    const uint32_t c = s_tab[t];
    if (c) atomicAdd(&counts[(size_t)(idx0 + (t >> 2)) * (k + 1) + (t & 3)], (unsigned long long)c);
  }
  if (threadIdx.x < 3 && s_info[threadIdx.x]) atomicAdd(&info[threadIdx.x], (unsigned long long)s_info[threadIdx.x]);
  if (threadIdx.x == 3 && s_first != ~0ull) atomicMin(&info[3], s_first);
}

// results the host computed for the records idx[0 .. m) -> their places in the caller's arrays
__global__ void pm_align_scatter(const uint64_t *idx, size_t m, const pm_alignment *src, const char *src_ops, const char *src_txt, size_t stride,
                                 pm_alignment *out, char *ops, char *txt) {
  const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (j >= m) return;
  const size_t i = (size_t)idx[j];
  out[i] = src[j];
  if (ops)
    for (size_t q = 0; q < stride; ++q) { ops[i * stride + q] = src_ops[j * stride + q]; txt[i * stride + q] = src_txt[j * stride + q]; }
}

}  // namespace

hipError_t align_scatter_device(const uint64_t *d_idx, size_t m, const pm_alignment *d_src, const char *d_src_ops, const char *d_src_txt, size_t stride,
                                pm_alignment *d_out, char *d_ops, char *d_txt, hipStream_t st) {
  if (m == 0) return hipSuccess;
  hipLaunchKernelGGL(pm_align_scatter, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_idx, m, d_src, d_src_ops, d_src_txt, stride, d_out, d_ops, d_txt);
  return hipGetLastError();
}

// d_tab: 256 characters by stream code, then 128 masks of 'A'..'Z' / 'a'..'z' by pattern character
void align_tables(const Alphabet &alpha, uint8_t *tab) {
  memcpy(tab, alpha.ch, 256);
  uint32_t mask[128];
  for (int w = 0; w < 128; ++w) {
    mask[w] = 0;
    const char *set = iupac_compatible_set((unsigned char)w);
    if (!set) continue;
    const bool upper = w >= 'A' && w <= 'Z';
    for (const char *c = set; *c; ++c) mask[w] |= 1u << (*c - (upper ? 'A' : 'a'));
  }
  memcpy(tab + 256, mask, sizeof(mask));
}

hipError_t align_hits_device(const AlignDevice &a, const uint8_t *d_text, int64_t ntext, const pm_hit *d_hits, const unsigned long long *d_count,
                             size_t n_upper, pm_alignment *d_out, char *d_ops, char *d_txt, size_t stride, uint64_t *d_keys,
                             pm_hit *d_hostq_hits, uint64_t *d_hostq_idx, unsigned long long *d_ctr, hipStream_t st) {
  hipError_t e = hipMemsetAsync(d_ctr, 0, 3 * sizeof(unsigned long long), st);
  if (e != hipSuccess || n_upper == 0) return e;
  const unsigned blocks = (unsigned)((n_upper + AL_THREADS - 1) / AL_THREADS);
  hipLaunchKernelGGL(pm_align_hits_kernel, dim3(blocks), dim3(AL_THREADS), 0, st, a, d_text, ntext, d_hits, d_count, n_upper, d_out, d_ops, d_txt,
                     stride, d_keys, d_hostq_hits, d_hostq_idx, d_ctr);
  return hipGetLastError();
}

hipError_t align_hits_wide_device(const AlignDevice &a, const uint8_t *d_text, int64_t ntext, const pm_hit *d_side_hits, const uint64_t *d_side_idx,
                                  size_t n_upper, pm_alignment *d_out, char *d_ops, char *d_txt, size_t stride, uint64_t *d_keys,
                                  pm_hit *d_rest_hits, uint64_t *d_rest_idx, unsigned long long *d_ctr, hipStream_t st) {
  if (!a.indels || a.k < 1 || a.k > AL_MAXK || !d_side_hits || !d_side_idx) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(d_ctr + 3, 0, sizeof(unsigned long long), st);
  if (e != hipSuccess || n_upper == 0) return e;
  // the grid covers the most the list can hold; blocks beyond its count exit at once
  const dim3 blocks((unsigned)((n_upper + AL_THREADS - 1) / AL_THREADS)), threads(AL_THREADS);
#define PM_WIDE_LAUNCH(W)                                                                                                                        \
  hipLaunchKernelGGL(pm_align_hits_wide_kernel<W>, blocks, threads, 0, st, a, d_text, ntext, d_side_hits, d_side_idx, n_upper, d_out, d_ops, d_txt, \
                     stride, d_keys, d_rest_hits, d_rest_idx, d_ctr)
  if (a.k == 1) PM_WIDE_LAUNCH(4);
  else if (a.k == 2) PM_WIDE_LAUNCH(6);
  else PM_WIDE_LAUNCH(8);
#undef PM_WIDE_LAUNCH
  return hipGetLastError();
}

size_t tally_temp_bytes(size_t n) {
  size_t sort_bytes = 0, scan_bytes = 0;
  uint64_t *p = nullptr;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, p, p, (int)n);
  (void)hipcub::DeviceScan::InclusiveScan(nullptr, scan_bytes, p, p, SegSum(), (int)n);
  return sort_bytes > scan_bytes ? sort_bytes : scan_bytes;
}

// n keys at d_keys (any order) -> d_counts[index * (k + 1) + distance] and d_info[0..3] (tallied, skipped behind the cap,
// bogus, smallest end << 22 | id rank of a bogus hit).  d_keys_alt and d_scan are workspaces of n keys each.
hipError_t tally_device(const AlignDevice &a, uint64_t *d_keys, uint64_t *d_keys_alt, uint64_t *d_scan, size_t n, void *d_temp, size_t temp_bytes,
                        uint64_t max_count, unsigned long long *d_counts, unsigned long long *d_info, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipError_t e;
  const unsigned blocks = (unsigned)((n + 255) / 256);
  if ((e = hipcub::DeviceRadixSort::SortKeys(d_temp, temp_bytes, d_keys, d_keys_alt, (int)n, 0, 64, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(pm_tally_flags, dim3(blocks), dim3(256), 0, st, d_keys_alt, n, d_scan);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::InclusiveScan(d_temp, temp_bytes, d_scan, d_keys, SegSum(), (int)n, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(pm_tally_decide, dim3(blocks), dim3(256), 0, st, d_keys_alt, n, d_keys, a.k, max_count, d_counts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const unsigned ablocks = (unsigned)((n + TALLY_ITEMS * 256 - 1) / (TALLY_ITEMS * 256));
  hipLaunchKernelGGL(pm_tally_add, dim3(ablocks), dim3(256), 0, st, d_keys_alt, d_keys, n, a.k, a.idrank, d_counts, d_info);
  return hipGetLastError();
}

}  // namespace pm
