// pm_pcr.hip -- pcr_match's pairing stage in HBM: join the held primer hits with their partners' hits
// inside the amplicon window, filter the re-aligned pairs and count the N's of the survivors.  The rule itself is
// pm_pcr.h; nothing here looks at the stream's 2-bit words (N's are not in them).
//
// Orders: `sorted` is the held list in (key, id, k) order, position = index there.  `gkeys` / `gpos` are the same hits grouped
// by id, in key order inside an id: gkeys[j] = id << endbits | key, gpos[j] = position.  Inside one id's segment both the
// positions and the deferred flags grow with j, so the partners that are alive for a hit -- those behind it or deferred --
// are a suffix of its window: the count pass finds that suffix with binary searches, the write pass copies it.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "pm_internal.h"

namespace pm {
namespace {

constexpr int PCR_THREADS = 256;
constexpr uint32_t PCR_LANE_MAX = 4;   // partners a lane writes itself; a longer window is written by the whole wave

inline unsigned blocks_for(size_t n) { return (unsigned)((n + PCR_THREADS - 1) / PCR_THREADS); }

__global__ __launch_bounds__(PCR_THREADS) void pm_pcr_keys(const pm_hit *held, uint32_t n, int idbits, int kbits, uint64_t *keys) {
  const uint32_t i = blockIdx.x * PCR_THREADS + threadIdx.x;
  if (i >= n) return;
  const pm_hit h = held[i];
  keys[i] = ((uint64_t)h.end << (idbits + kbits)) | ((uint64_t)h.pid << kbits) | (uint64_t)h.k;
}

// sorted keys -> records, the grouping keys, and who is deferred
__global__ __launch_bounds__(PCR_THREADS) void pm_pcr_unpack(const uint64_t *keys, uint32_t n, PcrDevice d, int64_t scanned_to, int more,
                                                            pm_hit *sorted, uint64_t *gkeys, uint32_t *gpos, uint32_t *def) {
  const uint32_t i = blockIdx.x * PCR_THREADS + threadIdx.x;
  if (i > n) return;
  if (i == n) { def[n] = 0; return; }                               // (the scans run over n + 1 items: the last offset is the total)
  const uint64_t key = keys[i];
  pm_hit h;
  h.k = (uint8_t)(key & ((1ull << d.kbits) - 1ull));
  h.pid = (uint32_t)((key >> d.kbits) & ((1ull << d.idbits) - 1ull));
  h.end = (int64_t)(key >> (d.idbits + d.kbits));
  h.aux[0] = h.aux[1] = h.aux[2] = 0;
  sorted[i] = h;
  gkeys[i] = ((uint64_t)h.pid << d.endbits) | (uint64_t)h.end;
  gpos[i] = i;
  const uint64_t pr = pcr::pair_of(d.rule, h.pid);
  int64_t smin, smax;
  pcr::stretch(d.rule, h.pid, h.end, d.patlen, d.size_lb ? d.size_lb[pr - 1] : 0, d.size_ub ? d.size_ub[pr - 1] : 0, &smin, &smax);
  def[i] = pcr::deferred(scanned_to, more, smax) ? 1u : 0u;
}

__device__ inline uint32_t lower_bound_key(const uint64_t *a, uint32_t n, uint64_t v) {   // first j with a[j] >= v
  uint32_t lo = 0, hi = n;
  while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (a[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}

// count pass: the alive suffix [wlo, whi) of each of the hit's two windows in the id-grouped order, and their total length
__global__ __launch_bounds__(PCR_THREADS) void pm_pcr_count(const pm_hit *sorted, uint32_t n, PcrDevice d, const uint64_t *gkeys, const uint32_t *gpos,
                                                           const uint32_t *def, uint32_t *wlo, uint32_t *whi, unsigned long long *cnt) {
  const uint32_t i = blockIdx.x * PCR_THREADS + threadIdx.x;
  if (i > n) return;
  if (i == n) { cnt[n] = 0; return; }
  unsigned long long total = 0;
  uint32_t lo2[2] = {0, 0}, hi2[2] = {0, 0};
  if (!def[i]) {
    const pm_hit h = sorted[i];
    const uint64_t pr = pcr::pair_of(d.rule, h.pid);
    int64_t smin, smax;
    pcr::stretch(d.rule, h.pid, h.end, d.patlen, d.size_lb ? d.size_lb[pr - 1] : 0, d.size_ub ? d.size_ub[pr - 1] : 0, &smin, &smax);
    uint64_t pid[2];
    pcr::partners(d.rule, h.pid, &pid[0], &pid[1]);
    const int64_t maxend = (int64_t)((1ull << d.endbits) - 1ull);
    if (smax >= 0 && smin <= maxend) {
      const uint64_t kmin = (uint64_t)(smin < 0 ? 0 : smin), kmax = (uint64_t)(smax > maxend ? maxend : smax);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        if (pid[p] == 0) continue;
        const uint64_t base = pid[p] << d.endbits;
        uint32_t lo = lower_bound_key(gkeys, n, base | kmin);
        const uint32_t hi = lower_bound_key(gkeys, n, (base | kmax) + 1);
        // the first partner behind this hit, and the first deferred one: whichever comes first starts the alive suffix
        uint32_t a = lo, b = hi;
        while (a < b) { const uint32_t mid = a + (b - a) / 2; if (gpos[mid] > i || def[gpos[mid]]) b = mid; else a = mid + 1; }
        lo = a;
        lo2[p] = lo; hi2[p] = hi;
        total += hi - lo;
      }
    }
  }
  wlo[2 * i] = lo2[0]; whi[2 * i] = hi2[0];
  wlo[2 * i + 1] = lo2[1]; whi[2 * i + 1] = hi2[1];
  cnt[i] = total;
}

// write pass: the pairs of hit i at off[i], pid1's before pid2's, each in key order.  Windows of more than PCR_LANE_MAX
// partners are handed to the wave: ballot, then the 64 lanes write one window after the other together.
__global__ __launch_bounds__(PCR_THREADS) void pm_pcr_write(uint32_t n, const uint32_t *wlo, const uint32_t *whi, const unsigned long long *off,
                                                           const uint32_t *gpos, uint2 *pairs, uint32_t *flag) {
  const uint32_t i = blockIdx.x * PCR_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool on = i < n;
  unsigned long long o = on ? off[i] : 0;
  bool any = false;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const uint32_t s = on ? wlo[2 * i + p] : 0, e = on ? whi[2 * i + p] : 0;
    const uint32_t len = e - s;
    any = any || len != 0;
    if (len <= PCR_LANE_MAX)
      for (uint32_t t = 0; t < len; ++t) { const uint32_t j = gpos[s + t]; pairs[o + t] = make_uint2(i, j); flag[j] = 1; }
    unsigned long long wide = __ballot(len > PCR_LANE_MAX);
    while (wide) {
      const int src = __builtin_ctzll(wide);
      wide &= wide - 1;
      const uint32_t ws = __shfl(s, src), wlen = __shfl(len, src), wi = __shfl(i, src);
      const unsigned long long wo = __shfl(o, src);
      for (uint32_t t = lane; t < wlen; t += 64) { const uint32_t j = gpos[ws + t]; pairs[wo + t] = make_uint2(wi, j); flag[j] = 1; }
    }
    o += len;
  }
  if (any) flag[i] = 1;
}

// flagged hits -> the list that is re-aligned (slot = exclusive scan of the flags)
__global__ __launch_bounds__(PCR_THREADS) void pm_pcr_gather(const pm_hit *sorted, uint32_t n, const uint32_t *flag, const uint32_t *slot, pm_hit *out) {
  const uint32_t i = blockIdx.x * PCR_THREADS + threadIdx.x;
  if (i < n && flag[i]) out[slot[i]] = sorted[i];
}

// filter pass, one lane per candidate pair
__global__ __launch_bounds__(PCR_THREADS) void pm_pcr_filter(const uint2 *pairs, uint32_t npairs, const pm_hit *sorted, const uint32_t *slot, const pm_alignment *al,
                                                            PcrDevice d, uint32_t *keep) {
  const uint32_t p = blockIdx.x * PCR_THREADS + threadIdx.x;
  if (p > npairs) return;
  if (p == npairs) { keep[p] = 0; return; }
  const uint2 ij = pairs[p];
  const pm_alignment a = al[slot[ij.x]], b = al[slot[ij.y]];
  const uint64_t pi = pcr::pind(d.rule, sorted[ij.x].pid, sorted[ij.y].pid);
  int64_t alen;
  keep[p] = pcr::survives(d.rule, a.start, a.end, a.editdist, b.start, b.end, b.editdist, d.entry_starts, d.n_entries,
                          d.size_lb ? d.size_lb[pi - 1] : 0, d.size_ub ? d.size_ub[pi - 1] : 0, &alen) ? 1u : 0u;
}

// survivors, in the order of the pairs (kof = exclusive scan of keep), with the strings of both ends when asked: the wave
// copies the 2 x 2 x stride bytes of one survivor after the other together, lane by lane along the bytes
__global__ __launch_bounds__(PCR_THREADS) void pm_pcr_emit(const uint2 *pairs, uint32_t npairs, const uint32_t *keep, const uint32_t *kof, const pm_hit *sorted,
                                                          const uint32_t *slot, const pm_alignment *al, const char *ops, const char *txt, size_t stride,
                                                          PcrDevice d, pm_pcr_amplicon *out, char *out_ops, char *out_txt) {
  const uint32_t p = blockIdx.x * PCR_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool kept = p < npairs && keep[p];
  uint32_t sa = 0, sb = 0, q = 0;
  if (kept) {
    const uint2 ij = pairs[p];
    sa = slot[ij.x]; sb = slot[ij.y]; q = kof[p];
    pm_pcr_amplicon r;
    r.hit[0] = sorted[ij.x]; r.hit[1] = sorted[ij.y];
    r.al[0] = al[sa]; r.al[1] = al[sb];
    r.amplicon_len = !d.rule.length_between ? r.al[1].end - r.al[0].start : r.al[1].start - r.al[0].end;
    r.pair = (uint32_t)pcr::pind(d.rule, r.hit[0].pid, r.hit[1].pid);
    r.ncount = 0;
    out[q] = r;
  }
  if (!ops) return;                                                   // (the same for every lane)
  unsigned long long todo = __ballot(kept);
  while (todo) {
    const int src = __builtin_ctzll(todo);
    todo &= todo - 1;
    const size_t wa = __shfl(sa, src), wb = __shfl(sb, src), wq = __shfl(q, src);
    for (size_t c = lane; c < 2 * stride; c += 64) {                 // strings 2q and 2q + 1 lie side by side
      const size_t from = c < stride ? wa * stride + c : wb * stride + (c - stride);
      out_ops[2 * wq * stride + c] = ops[from];
      out_txt[2 * wq * stride + c] = txt[from];
    }
  }
}

struct NMask { uint32_t w[8]; };

// N count, one wave per surviving amplicon: stream positions start .. start + amplicon_len - 1 that lie in [0, ntext).  The
// bytes up to the first 16-byte boundary and behind the last one are read one by one; nothing outside the range is loaded.
// (Alignments lie inside the stream and an amplicon ends at one's end, so the two clamps never cut: they guard the loads.)
__global__ __launch_bounds__(PCR_THREADS) void pm_pcr_ncount(pm_pcr_amplicon *out, uint32_t nsurv, const uint8_t *text, int64_t ntext, NMask mask) {
  __shared__ uint32_t m[8];
  if (threadIdx.x < 8) m[threadIdx.x] = mask.w[threadIdx.x];
  __syncthreads();
  const uint32_t q = blockIdx.x * (PCR_THREADS / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  if (q >= nsurv) return;
  int64_t lo = out[q].al[0].start, hi = lo + out[q].amplicon_len;
  if (lo < 0) lo = 0;
  if (hi > ntext) hi = ntext;
  uint32_t c = 0;
  if (hi > lo) {
    const uint8_t *b = text + lo, *e = text + hi;
    const uint8_t *body = (const uint8_t *)(((uintptr_t)b + 15) & ~(uintptr_t)15);
    if (body > e) body = e;
    const size_t chunks = (size_t)(e - body) / 16;
    const uint8_t *tail = body + chunks * 16;
    auto isn = [&](uint32_t ch) { return (m[ch >> 5] >> (ch & 31)) & 1u; };
    for (const uint8_t *x = b + lane; x < body; x += 64) c += isn(*x);
    for (size_t ch = lane; ch < chunks; ch += 64) {
      const uint4 v = ((const uint4 *)body)[ch];
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int t = 0; t < 4; ++t) c += isn(w[t] & 255) + isn((w[t] >> 8) & 255) + isn((w[t] >> 16) & 255) + isn(w[t] >> 24);
    }
    for (const uint8_t *x = tail + lane; x < e; x += 64) c += isn(*x);
  }
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if (lane == 0) out[q].ncount = c;
}

// deferred hits to the front of the held list (dof = exclusive scan of def)
__global__ __launch_bounds__(PCR_THREADS) void pm_pcr_carry(const pm_hit *sorted, uint32_t n, const uint32_t *def, const uint32_t *dof, pm_hit *held) {
  const uint32_t i = blockIdx.x * PCR_THREADS + threadIdx.x;
  if (i < n && def[i]) held[dof[i]] = sorted[i];
}

}  // namespace

size_t pcr_temp_bytes(size_t n) {
  size_t a = 0, b = 0, c = 0, e = 0;
  uint64_t *k = nullptr; uint32_t *v = nullptr; unsigned long long *s = nullptr;
  (void)hipcub::DeviceRadixSort::SortKeys(nullptr, a, k, k, (int)n);
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, k, k, v, v, (int)n);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, c, s, s, (int)n);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, e, v, v, (int)n);
  return std::max(std::max(a, b), std::max(c, e));
}

hipError_t pcr_scan_u32(const uint32_t *d_in, uint32_t *d_out, size_t n, void *d_temp, size_t temp_bytes, hipStream_t st) {
  return hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, d_in, d_out, (int)n, st);
}

hipError_t pcr_join_device(const PcrDevice &d, const pm_hit *d_held, size_t n, int64_t scanned_to, int more, const PcrRound &w, hipStream_t st) {
  hipError_t e;
  const uint32_t m = (uint32_t)n;
  size_t tb = w.temp_bytes;
  hipLaunchKernelGGL(pm_pcr_keys, dim3(blocks_for(n)), dim3(PCR_THREADS), 0, st, d_held, m, d.idbits, d.kbits, w.keys);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipcub::DeviceRadixSort::SortKeys(w.temp, tb, w.keys, w.keys_alt, (int)n, 0, d.endbits + d.idbits + d.kbits, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(pm_pcr_unpack, dim3(blocks_for(n + 1)), dim3(PCR_THREADS), 0, st, w.keys_alt, m, d, scanned_to, more, w.sorted, w.keys, w.gpos_in, w.def);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipcub::DeviceRadixSort::SortPairs(w.temp, tb, w.keys, w.keys_alt, w.gpos_in, w.gpos, (int)n, 0, d.endbits + d.idbits, st)) != hipSuccess) return e;
  hipLaunchKernelGGL(pm_pcr_count, dim3(blocks_for(n + 1)), dim3(PCR_THREADS), 0, st, w.sorted, m, d, w.keys_alt, w.gpos, w.def, w.wlo, w.whi, w.cnt);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(w.temp, tb, w.cnt, w.off, (int)(n + 1), st)) != hipSuccess) return e;
  return hipMemsetAsync(w.flag, 0, (n + 1) * sizeof(uint32_t), st);
}

hipError_t pcr_write_device(size_t n, const PcrRound &w, uint2 *d_pairs, hipStream_t st) {
  hipError_t e;
  hipLaunchKernelGGL(pm_pcr_write, dim3(blocks_for(n)), dim3(PCR_THREADS), 0, st, (uint32_t)n, w.wlo, w.whi, w.off, w.gpos, d_pairs, w.flag);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return pcr_scan_u32(w.flag, w.slot, n + 1, w.temp, w.temp_bytes, st);
}

hipError_t pcr_gather_device(size_t n, const PcrRound &w, pm_hit *d_out, hipStream_t st) {
  hipLaunchKernelGGL(pm_pcr_gather, dim3(blocks_for(n)), dim3(PCR_THREADS), 0, st, w.sorted, (uint32_t)n, w.flag, w.slot, d_out);
  return hipGetLastError();
}

hipError_t pcr_filter_device(const PcrDevice &d, const PcrRound &w, const uint2 *d_pairs, size_t npairs, const pm_alignment *d_al, uint32_t *d_keep, uint32_t *d_kof, hipStream_t st) {
  hipError_t e;
  hipLaunchKernelGGL(pm_pcr_filter, dim3(blocks_for(npairs + 1)), dim3(PCR_THREADS), 0, st, d_pairs, (uint32_t)npairs, w.sorted, w.slot, d_al, d, d_keep);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return pcr_scan_u32(d_keep, d_kof, npairs + 1, w.temp, w.temp_bytes, st);
}

hipError_t pcr_emit_device(const PcrDevice &d, const PcrRound &w, const uint2 *d_pairs, size_t npairs, const uint32_t *d_keep, const uint32_t *d_kof, size_t nsurv,
                           const pm_alignment *d_al, const char *d_ops, const char *d_txt, size_t stride, const uint8_t *d_text, int64_t ntext,
                           const uint32_t nmask[8], pm_pcr_amplicon *d_out, char *d_out_ops, char *d_out_txt, hipStream_t st) {
  if (nsurv == 0) return hipSuccess;
  hipLaunchKernelGGL(pm_pcr_emit, dim3(blocks_for(npairs)), dim3(PCR_THREADS), 0, st, d_pairs, (uint32_t)npairs, d_keep, d_kof, w.sorted, w.slot, d_al, d_ops, d_txt, stride,
                     d, d_out, d_out_ops, d_out_txt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  NMask mk;
  for (int i = 0; i < 8; ++i) mk.w[i] = nmask[i];
  const unsigned per = PCR_THREADS / 64;
  hipLaunchKernelGGL(pm_pcr_ncount, dim3((unsigned)((nsurv + per - 1) / per)), dim3(PCR_THREADS), 0, st, d_out, (uint32_t)nsurv, d_text, ntext, mk);
  return hipGetLastError();
}

hipError_t pcr_carry_device(size_t n, const PcrRound &w, pm_hit *d_held, hipStream_t st) {
  hipError_t e = pcr_scan_u32(w.def, w.slot, n + 1, w.temp, w.temp_bytes, st);   // (slot is free again: the round's records are out)
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(pm_pcr_carry, dim3(blocks_for(n)), dim3(PCR_THREADS), 0, st, w.sorted, (uint32_t)n, w.def, w.slot, d_held);
  return hipGetLastError();
}

}  // namespace pm
