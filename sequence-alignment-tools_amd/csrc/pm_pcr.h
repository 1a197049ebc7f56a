// pm_pcr.h -- the pairing rule of pcr_match as closed forms.
//
// One round of the reference's pairing stage (pcr_match.cc:948-1259, restated by host/pm_pcr_match.cc) walks the held
// hits in (key, id) order and zeroes the key of every hit it has processed.  What that loop decides depends on nothing but
// the two hits of a pair: the functions below say it per hit and per pair, so that the kernels of pm_pcr.hip, the host
// code of the library and a plain C++ test program share one copy.  No HIP types: a host compiler can include this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PM_PCR_HD __host__ __device__ inline
#else
#define PM_PCR_HD inline
#endif

namespace pm {
namespace pcr {

// The options of a run (pcr_match's -a, -b, -m, -M, -d, -k / -K) and n, the number of primers: ids 1..n are the primers as
// given (2j-1 forward, 2j reverse), n+1..2n their reverse complements.
struct Rule {
  uint64_t n;
  int32_t any_orientation, length_between;
  int64_t amplicon_min, amplicon_max;
  int32_t size_slack;               // -d (< 0: none)
  int32_t has_sizes;                // the primers carry UniSTS size bounds (-S)
  int32_t k, slack;                 // -k / -K value; slack = k with indels, 1 without
};

// partner ids of a hit of pattern pid (0: none), pcr_match.cc:1003-1029
PM_PCR_HD void partners(const Rule &r, uint64_t pid, uint64_t *pid1, uint64_t *pid2) {
  const uint64_t n = r.n;
  uint64_t p1 = 0, p2 = 0;
  if (pid <= n && pid % 2 == 1) p1 = pid + 1;
  else if (pid > n && (pid - n) % 2 == 0) p1 = pid - 1;
  if (r.any_orientation) {
    if (pid <= n) {
      if (pid % 2 == 1) p2 = pid + n + 1;
      else { p1 = pid - 1; p2 = pid + n - 1; }
    } else {
      if (pid % 2 == 0) p2 = pid - n - 1;
      else { p1 = pid + 1; p2 = pid - n + 1; }
    }
  }
  *pid1 = p1; *pid2 = p2;
}

// primer pair (1-based) a pattern id belongs to
PM_PCR_HD uint64_t pair_of(const Rule &r, uint64_t pid) { return (pid - (pid > r.n ? r.n : 0) + 1) / 2; }

// The window of partner keys of a hit at stream position pos (pcr_match.cc:1031-1052).  patlen[id] for id = 1..2n;
// size_lb / size_ub are the pair's UniSTS bounds (read only when has_sizes and size_slack >= 0).  The clamp compares as
// unsigned 64-bit values and size_lb - size_slack wraps, as in the reference.
PM_PCR_HD void stretch(const Rule &r, uint64_t pid, int64_t pos, const int32_t *patlen, uint64_t size_lb, uint64_t size_ub,
                       int64_t *stretch_min, int64_t *stretch_max) {
  uint64_t pid1, pid2;
  partners(r, pid, &pid1, &pid2);
  int64_t smax = r.amplicon_max, smin = r.amplicon_min;
  if (r.length_between) {
    int64_t plen = 0;
    if (pid1 != 0) plen = patlen[pid1];
    if (pid2 != 0 && patlen[pid2] > plen) plen = patlen[pid2];
    smax += plen + patlen[pid];
  }
  if (r.has_sizes && r.size_slack >= 0) {
    const uint64_t ub = size_ub + (uint64_t)(int64_t)r.size_slack;
    const uint64_t lb = size_lb - (uint64_t)(int64_t)r.size_slack;
    if ((uint64_t)smax > ub) smax = (int64_t)ub;
    if ((uint64_t)smin < lb) smin = (int64_t)lb;
  }
  *stretch_max = smax + pos - patlen[pid] + r.slack;
  *stretch_min = smin + pos - patlen[pid] - r.slack;
}

// a hit whose window is not scanned yet waits for the next round (pcr_match.cc:1054)
PM_PCR_HD bool deferred(int64_t scanned_to, int more, int64_t stretch_max) { return more && scanned_to < stretch_max; }

// SeqDb::locate: index of the last entry whose start is <= pos - 1 (an upper_bound over the entry starts), -1: none
PM_PCR_HD int64_t locate(const int64_t *starts, int64_t n_entries, int64_t pos) {
  int64_t lo = 0, hi = n_entries;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (starts[mid] <= pos - 1) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}
PM_PCR_HD bool is_subseq(const int64_t *starts, int64_t n_entries, int64_t start, int64_t end) {
  const int64_t a = locate(starts, n_entries, start + 1), b = locate(starts, n_entries, end);
  return a >= 0 && b >= 0 && a == b;
}

// pind: the primer pair of a candidate pair of hits (pcr_match.cc:1131-1135)
PM_PCR_HD uint64_t pind(const Rule &r, uint64_t pid, uint64_t pid1) {
  const uint64_t ind = pid - (pid > r.n ? r.n : 0), ind1 = pid1 - (pid1 > r.n ? r.n : 0);
  return ind < ind1 ? ind / 2 + 1 : ind1 / 2 + 1;
}

// The filter of pcr_match.cc:1116-1160 on the two re-alignments (start, end, editdist of the first and the second hit
// of the candidate pair).  size_lb / size_ub: the bounds of pair pind.  *amplicon_len is written either way.
PM_PCR_HD bool survives(const Rule &r, int64_t start, int64_t end, int32_t editdist, int64_t start1, int64_t end1, int32_t editdist1,
                        const int64_t *entry_starts, int64_t n_entries, uint64_t size_lb, uint64_t size_ub, int64_t *amplicon_len) {
  const int64_t ps = start, pe = end, ps1 = start1, pe1 = end1;
  const long alen = !r.length_between ? (long)(pe1 - ps) : (long)(ps1 - pe);
  *amplicon_len = alen;
  if (editdist < 0 || editdist > r.k || editdist1 < 0 || editdist1 > r.k) return false;
  if (!is_subseq(entry_starts, n_entries, ps, pe1)) return false;
  if (!(alen <= r.amplicon_max && alen >= r.amplicon_min)) return false;
  if (r.has_sizes && r.size_slack >= 0) {
    if (!(((unsigned long)(alen + r.size_slack) >= size_lb) && (alen <= (long)((int)size_ub) + r.size_slack))) return false;
  }
  return true;
}

}  // namespace pcr
}  // namespace pm
