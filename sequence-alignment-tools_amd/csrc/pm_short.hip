// pm_short.hip -- patterns of 16..19 characters: the first stage of the edit-distance plan and, further
// down, the substitution class beside the pair plan (pm_short_sub_scan).
//
// The edit plan of pm_seed.hip / pm_pair.hip seeds on the last 20 pattern bases, so a primer of 16..19 bases used to go
// to the bit-parallel residue kernel.  Here the last SIXTEEN bases are four fields of four -- the four bytes of the 2-bit
// packed word -- and the geometry is the pair-edit plan's: <= 2 edits leave two fields A < B untouched,
// which sit in the text 4 (B - A) + d bases apart, d = net insertions between them; 14 tests (A, B, d) cover every
// placement of two edits, two tests every placement of one (scripts/edit_pair_cover.py 4).
//
//   pm_short_edit_scan   reads the stream's 2-bit words; per window (position p = its last base) and test the 16-bit key
//                        "field A taken d bases early | field B" is looked up in the exact key bitmap of the field pair
//                        (six bitmaps of 2^16 bits = 48 KiB of LDS).  Key hits go through a queue of the wave in LDS and
//                        are then resolved with every lane busy: the key's run of patterns (offset table + pattern
//                        indices, L2 resident), a q-gram count over the pattern's 16 bases as a necessary condition, and
//                        what passes leaves as a seed record "pattern i, position p" in reserved blocks of the seed list.
//   pm_edits_verify      (pm_seed.hip) runs the k-error automaton for every seed record and reads off the ends p-1 .. p+3:
//                        with field B in place, the edits behind B move the end by at most +-k.
//
// N, end-of-sequence and positions outside the stream pack to arbitrary bases: a window that holds one can only gain key
// hits (the automaton decides on the real characters), and it cannot lose a true one -- a text character that is not the
// pattern's is an edit of the alignment, and both the cover and the q-gram count argue about the bases no edit touches.
#include "pm_internal.h"
#include "pm_seed.h"
#include "pm_verify.h"

#include <algorithm>
#include <cstring>
#include <utility>

namespace pm {

namespace {

constexpr int SHORT_THREADS = 256;                  // 4 waves share the bitmaps; 48 KiB + 16 KiB of queues: two workgroups per CU
constexpr int SHORT_WAVES = SHORT_THREADS / 64;
constexpr int SHORT_PAIRS = 6;
constexpr int SHORT_BM_WORDS = 2048;                // 2^16 key bits per field pair
constexpr int SHORT_ROWS = 65536 + 1;               // offset table rows per field pair (+ the end of the last run)
constexpr int SHORT_QCAP = 2048;                    // 2-byte key-hit entries per wave: two tests of a block (2 x 1024 windows) fit behind a drain
constexpr int SHORT_OUT_BLOCK = 256;                // seed list slots a wave reserves per atomic

// the tests in table order (the pair-edit plan's): (0,1,0); (0,2,-1..1); (0,3,-2..2); (1,2,0); (1,3,-1..1); (2,3,0)
constexpr int t_a(int v) { const int t[SHORT_NTESTS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2}; return t[v]; }
constexpr int t_b(int v) { const int t[SHORT_NTESTS] = {1, 2, 2, 2, 3, 3, 3, 3, 3, 2, 3, 3, 3, 3}; return t[v]; }
constexpr int t_d(int v) { const int t[SHORT_NTESTS] = {0, -1, 0, 1, -2, -1, 0, 1, 2, 0, -1, 0, 1, 0}; return t[v]; }
constexpr int pair_of(int a, int b) { return a == 0 ? b - 1 : (a == 1 ? b + 1 : 5); }   // (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
// A window's text: 20 bases from p - 17 on, base t at bits 2t of a 40-bit string; window base i (0..15) = t = i + 2.
constexpr int off_a(int v) { return 4 + 8 * t_a(v) - 2 * t_d(v); }   // field A, d bases early
constexpr int off_b(int v) { return 4 + 8 * t_b(v); }
constexpr uint32_t test_word(int v) { return (uint32_t)off_a(v) | ((uint32_t)off_b(v) << 8) | ((uint32_t)pair_of(t_a(v), t_b(v)) << 16); }
__constant__ uint32_t SHORT_TEST[16] = {test_word(0), test_word(1), test_word(2), test_word(3), test_word(4), test_word(5), test_word(6),
                                        test_word(7), test_word(8), test_word(9), test_word(10), test_word(11), test_word(12), test_word(13), 0, 0};

struct ShortArgs {
  const uint32_t *packed;               // the stream, 2 bits per base, 16 bases per dword
  int64_t npacked;
  int64_t p_lo, p_hi;                   // window positions lo <= p < hi
  int64_t chunk0, chunk_len;            // first chunk (absolute, chunk_len aligned); positions per workgroup, a multiple of 1024 * SHORT_WAVES
  const uint32_t *bitmap;               // [pair][SHORT_BM_WORDS]
  const uint32_t *rows;                 // [pair][SHORT_ROWS]: first entry of the key's run in runs
  const uint32_t *runs;                 // pattern indices (inside the tile) by pair and key
  const uint32_t *pat16;                // the patterns' last 16 bases, 2 bits each
  uint32_t tile_base;                   // index of the tile's first pattern in the class (seed records carry class indices)
  uint64_t *seed_out;
  unsigned long long *seed_count;
  unsigned long long seed_cap;
};

__device__ __forceinline__ uint32_t load_words(const uint32_t *packed, int64_t npacked, int64_t pos) {
  const int64_t i = pos >> 4;
  return (pos < 0 || i >= npacked) ? 0u : packed[i];
}

template <int... Is, typename F>
__device__ __forceinline__ void static_each(std::integer_sequence<int, Is...>, F &&f) { (f(std::integral_constant<int, Is>()), ...); }

// 32 bits from bit O (compile time) of the 128-bit string w0 : w1 : w2 : w3 (bit 0 = bit 0 of w0)
template <int O>
__device__ __forceinline__ uint32_t bits128(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
  static_assert(O >= 0 && O < 128, "offset");
  if constexpr (O == 0) return w0;
  else if constexpr (O < 32) return __builtin_amdgcn_alignbit(w1, w0, O);
  else if constexpr (O == 32) return w1;
  else if constexpr (O < 64) return __builtin_amdgcn_alignbit(w2, w1, O - 32);
  else if constexpr (O == 64) return w2;
  else if constexpr (O < 96) return __builtin_amdgcn_alignbit(w3, w2, O - 64);
  else return w3 >> (O - 96);
}

// q-gram lemma with positions over the pattern's last 16 bases P (base i at bits 2i), field B in place: an edit touches at
// most four of the 13 four-base words and three of the 14 three-base words; every untouched word sits in the text within
// k bases of where the frame expects it.  xlo : xhi = the window's 40 text bits (base i of the window at bits 2 (i + 2)).
template <int K>
__device__ __forceinline__ bool short_plausible(uint32_t P, uint32_t xlo, uint32_t xhi) {
  uint32_t n4 = ~0u, n3 = ~0u;                                      // bit 2i clear: the four / three bases from i on are equal at some displacement
#pragma unroll
  for (int s = -K; s <= K; ++s) {
    const int c = 2 * (2 + s);
    const uint32_t x = P ^ (c ? __builtin_amdgcn_alignbit(xhi, xlo, c) : xlo);
    const uint32_t z3 = x | (x >> 2) | (x >> 4), z4 = z3 | (x >> 6);
    n3 &= z3 | (z3 >> 1); n4 &= z4 | (z4 >> 1);
  }
  return __popc(~n4 & 0x1555555u) >= 13 - 4 * K && __popc(~n3 & 0x5555555u) >= 14 - 3 * K;
}

template <int K>
__global__ __launch_bounds__(SHORT_THREADS) void pm_short_edit_scan(ShortArgs a) {
  __shared__ uint32_t s_bm[SHORT_PAIRS * SHORT_BM_WORDS];
  __shared__ uint16_t s_q[SHORT_WAVES][SHORT_QCAP];
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(a.bitmap);
    uint4 *dst = reinterpret_cast<uint4 *>(s_bm);
    for (int i = threadIdx.x; i < SHORT_PAIRS * SHORT_BM_WORDS / 4; i += SHORT_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t sub = a.chunk_len / SHORT_WAVES;
  const int64_t ws = (a.chunk0 + (int64_t)blockIdx.x) * a.chunk_len + (int64_t)wave * sub;   // a multiple of 1024
  const int64_t lo = ws > a.p_lo ? ws : a.p_lo, hi = ws + sub < a.p_hi ? ws + sub : a.p_hi;
  if (lo >= hi) return;
  uint16_t *q = s_q[wave];
  int qn = 0;                                                       // wave-uniform: key hits queued
  unsigned long long ob_next = 0;                                   // wave-uniform: next free slot of the wave's reserved run of the seed list
  int ob_left = 0;

  // every queued key hit of block bb: its run of patterns, the q-gram count, seed records
  auto drain = [&](int64_t bb) __attribute__((always_inline)) {
    for (int base = 0; base < qn; base += 64) {
      const bool valid = base + lane < qn;
      const uint32_t e = valid ? (uint32_t)q[base + lane] : 0u;
      const uint32_t win = (e >> 4) & 15u, tw = SHORT_TEST[e & 15u];
      const int64_t pb = bb + 16 * (int64_t)(e >> 8);
      const uint32_t w0 = load_words(a.packed, a.npacked, pb - 32), w1 = load_words(a.packed, a.npacked, pb - 16);
      const uint32_t w2 = load_words(a.packed, a.npacked, pb), w3 = load_words(a.packed, a.npacked, pb + 16);
      // the window's 40 bits start at bit 30 + 2 win of w0 : w1 : w2 : w3
      const bool up = win != 0;                                      // (bit 30 + 2 win >= 32)
      const uint32_t sh = (30u + 2u * win) & 31u;
      const uint32_t b0 = up ? w1 : w0, b1 = up ? w2 : w1, b2 = up ? w3 : w2;
      const uint32_t xlo = __builtin_amdgcn_alignbit(b1, b0, sh), xhi = __builtin_amdgcn_alignbit(b2, b1, sh);
      const uint32_t ka = __builtin_amdgcn_alignbit(xhi, xlo, tw & 31u) & 0xffu, kb = __builtin_amdgcn_alignbit(xhi, xlo, (tw >> 8) & 31u) & 0xffu;
      const uint32_t row = (tw >> 16) * (uint32_t)SHORT_ROWS + (ka | (kb << 8));
      uint32_t cur = 0, stop = 0;
      if (valid) { cur = a.rows[row]; stop = a.rows[row + 1]; }
      const int64_t p = pb + (int64_t)win;
      while (__ballot(cur < stop)) {
        bool pass = false;
        uint32_t pi = 0;
        if (cur < stop) {
          pi = a.runs[cur];
          pass = short_plausible<K>(a.pat16[pi], xlo, xhi);
          ++cur;
        }
        const unsigned long long bal = __ballot(pass);
        if (bal == 0) continue;
        const int c = __popcll(bal);
        if (c > ob_left) {                                           // a fresh run of slots; what is left of the old one is marked unused
          for (int u = lane; u < ob_left; u += 64) if (ob_next + u < a.seed_cap) a.seed_out[ob_next + u] = ~0ull;
          unsigned long long got = 0;
          if (lane == 0) got = atomicAdd(a.seed_count, (unsigned long long)SHORT_OUT_BLOCK);
          ob_next = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(got >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)got);
          ob_left = SHORT_OUT_BLOCK;
        }
        if (pass) {
          const unsigned long long slot = ob_next + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
          if (slot < a.seed_cap) a.seed_out[slot] = ((uint64_t)(a.tile_base + pi) << 40) | ((uint64_t)p & 0xffffffffffull);
        }
        ob_next += c; ob_left -= c;
      }
    }
    qn = 0;
  };

  for (int64_t bb = ws + (lo - ws) / 1024 * 1024; bb < hi; bb += 1024) {
    const int64_t pbase = bb + 16 * lane;                            // this lane's windows: p = pbase .. pbase + 15
    uint32_t own = 0xffffu;
    {
      const int64_t l = lo - pbase, h = hi - pbase;
      const uint32_t lb = l <= 0 ? 0u : (l >= 16 ? 16u : (uint32_t)l), hb = h <= 0 ? 0u : (h >= 16 ? 16u : (uint32_t)h);
      own = ((1u << hb) - 1u) & ~((1u << lb) - 1u);
    }
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    if (own) {                                                       // (lanes outside the range read nothing: the range's halo bounds every load)
      w0 = load_words(a.packed, a.npacked, pbase - 32); w1 = load_words(a.packed, a.npacked, pbase - 16);
      w2 = load_words(a.packed, a.npacked, pbase); w3 = load_words(a.packed, a.npacked, pbase + 16);
    }
    // two tests per round: bit j of the low / high half = window j has the key of test v / v + 1 in the pair's bitmap
    static_each(std::make_integer_sequence<int, (K == 2 ? SHORT_NTESTS : 2) / 2>(), [&](auto R) __attribute__((always_inline)) {
      constexpr int r = decltype(R)::value;
      constexpr int V0 = K == 2 ? 2 * r : 0, V1 = K == 2 ? 2 * r + 1 : SHORT_NTESTS - 1;   // (k = 1: the tests (0,1,0) and (2,3,0))
      uint32_t m = 0;
      static_each(std::make_integer_sequence<int, 16>(), [&](auto J) __attribute__((always_inline)) {
        constexpr int j = decltype(J)::value, O = 30 + 2 * j;
        auto hit = [&](auto VV) __attribute__((always_inline)) -> uint32_t {
          constexpr int v = decltype(VV)::value, OA = O + off_a(v), OB = O + off_b(v), BM = pair_of(t_a(v), t_b(v)) * SHORT_BM_WORDS;
          const uint32_t key = (bits128<OA>(w0, w1, w2, w3) & 0xffu) | ((bits128<OB>(w0, w1, w2, w3) & 0xffu) << 8);
          return (s_bm[BM + (key >> 5)] >> (key & 31u)) & 1u;
        };
        m |= hit(std::integral_constant<int, V0>()) << j;
        m |= hit(std::integral_constant<int, V1>()) << (16 + j);
      });
      m &= own | (own << 16);
      const int cnt = __popc(m);
      if (__ballot(cnt != 0)) {
        int x = cnt;                                                 // inclusive prefix sum over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
        const int total = __shfl(x, 63);
        if (qn + total > SHORT_QCAP) drain(bb);                      // (total <= SHORT_QCAP)
        int at = qn + x - cnt;
        while (m) {
          const int b = __builtin_ctz(m);
          m &= m - 1u;
          q[at++] = (uint16_t)(((uint32_t)lane << 8) | ((uint32_t)(b & 15) << 4) | (uint32_t)(b < 16 ? V0 : V1));
        }
        qn += total;
      }
    });
    if (qn) drain(bb);
  }
  for (int u = lane; u < ob_left; u += 64) if (ob_next + u < a.seed_cap) a.seed_out[ob_next + u] = ~0ull;
}

// ---- substitutions only: patterns of 16..19 characters beside a main class on the pair plan ------------
//
//   pm_short_sub_scan    <= 2 substitutions leave two of the four fields clean and in place: no displacement, so a test is a
//                        field pair -- the pair plan's combos, six at k = 2, (0,1) and (2,3) at k = 1 -- and a window is the
//                        16 bases that end at p.  Key hits go through the wave's queue as above; a key's run holds 8-byte
//                        entries {pattern index, the pattern's last 16 bases}, so ONE read behind the offset table settles a
//                        key hit: XOR + popcount against the window (the key fields are equal, what differs lies in the
//                        other two).  What is within k leaves as an 8-byte suspect "combo, pattern, position".
//   pm_short_sub_verify  pair_verify<4> of pm_verify.h per suspect -- the pair plan's exact stage on fields of four bases:
//                        raw stream bytes (N = mismatch, EOS = reject), exact zones, "reported once, by the first clean field
//                        pair of the plan", clean-half flags -- into the record list of the main class.
//
// As above, N, end-of-sequence and positions outside the stream pack to arbitrary bases: such a window can only gain
// suspects.  It cannot lose a candidate either: a text character that is not the pattern's is one of its <= k mismatches,
// and the two fields no mismatch touches are clean on the packed bases as well.
constexpr int SUB_OUT_BLOCK = 64;                   // suspect slots a wave reserves per atomic
constexpr int SUB_VERIFY_BLOCKS = 4096;
constexpr uint64_t SUB_POS_MASK = 0xffffffffffull;  // suspect: combo << 61 | class index of the pattern (21 bits) << 40 | position
constexpr size_t SUB_MAX_PATTERNS = (size_t)1 << 21;


struct SubArgs {
  const uint8_t *text;
  int64_t n;
  const uint32_t *packed;               // the stream, 2 bits per base, 16 bases per dword
  int64_t npacked;
  int64_t p_lo, p_hi;                   // window positions lo <= p < hi (hit ends p + 1)
  int64_t chunk0, chunk_len;            // as ShortArgs
  int k, eos_code, ncombos, viol_level;
  int fa[SUB_MAX_COMBOS], fb[SUB_MAX_COMBOS];
  const uint32_t *bitmap;               // the tile's: [combo][SHORT_BM_WORDS]
  const uint32_t *rows;                 //             [combo][SHORT_ROWS]: first entry of the key's run in runs
  const uint2 *runs;                    //             {pattern index inside the tile, its last 16 bases} by combo and key
  uint32_t tile_base;
  const uint8_t *pat_len;               // the class's (pair_verify)
  const uint32_t *pat_id;
  const uint8_t *pat_codes;
  const uint32_t *pat_zone;
  uint64_t *susp;
  unsigned long long *susp_count;
  unsigned long long susp_cap;
  pm_hit *out;
  unsigned long long *counter;
  unsigned long long cap;
};

template <int K>
__global__ __launch_bounds__(SHORT_THREADS) void pm_short_sub_scan(SubArgs a) {
  constexpr int NC = sub_ncombos(K);
  __shared__ uint32_t s_bm[NC * SHORT_BM_WORDS];
  __shared__ uint16_t s_q[SHORT_WAVES][SHORT_QCAP];
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(a.bitmap);
    uint4 *dst = reinterpret_cast<uint4 *>(s_bm);
    for (int i = threadIdx.x; i < NC * SHORT_BM_WORDS / 4; i += SHORT_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t sub = a.chunk_len / SHORT_WAVES;
  const int64_t ws = (a.chunk0 + (int64_t)blockIdx.x) * a.chunk_len + (int64_t)wave * sub;   // a multiple of 1024
  const int64_t lo = ws > a.p_lo ? ws : a.p_lo, hi = ws + sub < a.p_hi ? ws + sub : a.p_hi;
  if (lo >= hi) return;
  uint16_t *q = s_q[wave];
  int qn = 0;                                                       // wave-uniform: key hits queued
  unsigned long long ob_next = 0;                                   // wave-uniform: next free slot of the wave's reserved run of the suspect list
  int ob_left = 0;
  uint32_t w1 = 0, w2 = 0;                                          // this lane's stream words of the block (sub_window)

  // every queued key hit of block bb: the key's run of {pattern, last 16 bases}, the other two fields, suspects
  auto drain = [&](int64_t bb) __attribute__((always_inline)) {
    for (int base = 0; base < qn; base += 64) {
      const bool valid = base + lane < qn;
      const uint32_t e = valid ? (uint32_t)q[base + lane] : 0u;
      const uint32_t win = (e >> 4) & 15u, c = e & 15u, from = e >> 8;
      const uint32_t W = sub_window((uint32_t)__shfl((int)w1, (int)from), (uint32_t)__shfl((int)w2, (int)from), win);
      // the combo's fields, a nibble each: (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) / (0,1) (2,3)
      const int fa = (int)(((K == 2 ? 0x211000u : 0x20u) >> (4u * c)) & 15u), fb = (int)(((K == 2 ? 0x332321u : 0x31u) >> (4u * c)) & 15u);
      const uint32_t row = c * (uint32_t)SHORT_ROWS + sub_key(W, fa, fb);
      uint32_t cur = 0, stop = 0;
      if (valid) { cur = a.rows[row]; stop = a.rows[row + 1]; }
      const int64_t p = bb + 16 * (int64_t)from + (int64_t)win;
      while (__ballot(cur < stop)) {
        bool pass = false;
        uint32_t pi = 0;
        if (cur < stop) {
          const uint2 r = a.runs[cur];
          pi = r.x;
          pass = sub_others_within(W, r.y, K);
          ++cur;
        }
        const unsigned long long bal = __ballot(pass);
        if (bal == 0) continue;
        const int n = __popcll(bal);
        if (n > ob_left) {                                           // a fresh run of slots; what is left of the old one is marked unused
          for (int u = lane; u < ob_left; u += 64) if (ob_next + u < a.susp_cap) a.susp[ob_next + u] = ~0ull;
          unsigned long long got = 0;
          if (lane == 0) got = atomicAdd(a.susp_count, (unsigned long long)SUB_OUT_BLOCK);
          ob_next = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(got >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)got);
          ob_left = SUB_OUT_BLOCK;
        }
        if (pass) {
          const unsigned long long slot = ob_next + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
          if (slot < a.susp_cap) a.susp[slot] = ((uint64_t)c << 61) | ((uint64_t)(a.tile_base + pi) << 40) | ((uint64_t)p & SUB_POS_MASK);
        }
        ob_next += n; ob_left -= n;
      }
    }
    qn = 0;
  };

  for (int64_t bb = ws + (lo - ws) / 1024 * 1024; bb < hi; bb += 1024) {
    const int64_t pbase = bb + 16 * lane;                            // this lane's windows: p = pbase .. pbase + 15
    uint32_t own = 0xffffu;
    {
      const int64_t l = lo - pbase, h = hi - pbase;
      const uint32_t lb = l <= 0 ? 0u : (l >= 16 ? 16u : (uint32_t)l), hb = h <= 0 ? 0u : (h >= 16 ? 16u : (uint32_t)h);
      own = ((1u << hb) - 1u) & ~((1u << lb) - 1u);
    }
    w1 = 0; w2 = 0;
    if (own) { w1 = load_words(a.packed, a.npacked, pbase - 16); w2 = load_words(a.packed, a.npacked, pbase); }   // (lanes outside the range read nothing)
    // two combos per mask: bit j of the low / high half = window j has the key of combo 2r / 2r + 1 in that combo's bitmap
    uint32_t m[NC / 2];
#pragma unroll
    for (int r = 0; r < NC / 2; ++r) m[r] = 0;
    static_each(std::make_integer_sequence<int, 16>(), [&](auto J) __attribute__((always_inline)) {
      constexpr int j = decltype(J)::value;
      const uint32_t W = sub_window(w1, w2, j);
      static_each(std::make_integer_sequence<int, NC>(), [&](auto C) __attribute__((always_inline)) {
        constexpr int c = decltype(C)::value;
        const uint32_t key = sub_key(W, sub_fa(K, c), sub_fb(K, c));
        m[c / 2] |= ((s_bm[c * SHORT_BM_WORDS + (key >> 5)] >> (key & 31u)) & 1u) << (16 * (c & 1) + j);
      });
    });
    static_each(std::make_integer_sequence<int, NC / 2>(), [&](auto R) __attribute__((always_inline)) {
      constexpr int r = decltype(R)::value;
      uint32_t mm = m[r] & (own | (own << 16));
      const int cnt = __popc(mm);
      if (__ballot(cnt != 0)) {
        int x = cnt;                                                 // inclusive prefix sum over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
        const int total = __shfl(x, 63);
        if (qn + total > SHORT_QCAP) drain(bb);                      // (total <= SHORT_QCAP)
        int at = qn + x - cnt;
        while (mm) {
          const int b = __builtin_ctz(mm);
          mm &= mm - 1u;
          q[at++] = (uint16_t)(((uint32_t)lane << 8) | ((uint32_t)(b & 15) << 4) | (uint32_t)(2 * r + (b >> 4)));
        }
        qn += total;
      }
    });
    if (qn) drain(bb);
  }
  for (int u = lane; u < ob_left; u += 64) if (ob_next + u < a.susp_cap) a.susp[ob_next + u] = ~0ull;
}

// The scan's suspects, one per thread: the pair plan's exact stage with fields of four bases.  Records leave through the
// workgroup's LDS stage (pair_emit), as in pm_pair_verify.
__global__ __launch_bounds__(256) void pm_short_sub_verify(SubArgs a) {
  __shared__ pm_hit s_rec[VSTAGE];
  __shared__ unsigned long long s_base;
  __shared__ uint32_t s_fill, s_valid, s_full;
  const VerifyStage vs = {s_rec, &s_fill, &s_valid};
  unsigned long long n = *a.susp_count;
  if (n > a.susp_cap) n = a.susp_cap;
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  if (threadIdx.x == 0) { s_fill = 0; s_valid = (uint32_t)VSTAGE; }
  __syncthreads();
  auto flush = [&]() __attribute__((always_inline)) {               // the staged records join the list: one atomic (block-uniform call)
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
    bool have = false;
    if (i < n) {
      const uint64_t r = a.susp[i];
      if (r != ~0ull)                                                 // (a slot its wave reserved and did not need)
        have = pair_verify<4>(a, (int)(r >> 61), (int64_t)(r & SUB_POS_MASK), (uint32_t)(r >> 40) & (uint32_t)(SUB_MAX_PATTERNS - 1), &hh);
    }
    pair_emit(a, vs, have, hh);                                       // (every lane is here)
    __syncthreads();
    if (threadIdx.x == 0) s_full = s_fill > (uint32_t)(VSTAGE - 512);
    __syncthreads();
    if (s_full) flush();
  }
  flush();
}

}  // namespace

std::string short_build(const std::vector<Pattern> &pats, const std::vector<uint32_t> &ids, const Alphabet &alpha, int k, int eos_code,
                        size_t tile, ShortTables *out) {
  ShortTables &t = *out;
  t = ShortTables();
  if (k < 1 || k > 2) return "pm_short_edit_scan is built for k = 1 and k = 2";
  const bool norm = alpha.nch['A'] == 0 && alpha.nch['C'] == 1 && alpha.nch['G'] == 2 && alpha.nch['T'] == 3;
  const bool ascii = alpha.size == 256 && alpha.nch['A'] == 'A' && alpha.nch['C'] == 'C' && alpha.nch['G'] == 'G' && alpha.nch['T'] == 'T';
  if (!norm && !ascii) return "stream alphabet is neither A,C,G,T-normalized nor raw ASCII";
  t.k = k; t.ascii = ascii && !norm; t.eos_code = eos_code >= 0 && eos_code < 256 ? eos_code : -1;
  auto base2 = [&](unsigned char ch) -> int {                       // the stream's packing (pm_seed.hip pack4)
    switch (ch) { case 'A': return 0; case 'C': return 1; case 'G': return t.ascii ? 3 : 2; case 'T': return t.ascii ? 2 : 3; }
    return -1;
  };
  const size_t np = pats.size();
  if (np >= ((size_t)1 << 22)) return "too many patterns of 16..19 characters (22-bit pattern index)";
  t.records.assign(np * 32, 0);
  std::vector<uint32_t> p16(np);
  for (size_t j = 0; j < np; ++j) {
    const std::string &s = pats[j].s;
    const int L = (int)s.size();
    if (L < 16 || L > 19) return "pm_short_edit_scan takes patterns of 16..19 characters";
    for (unsigned char ch : s) if (base2(ch) < 0) return "pattern with characters other than A,C,G,T";
    t.maxlen = std::max(t.maxlen, L);
    uint32_t w = 0;
    for (int i = 0; i < 16; ++i) w |= (uint32_t)base2((unsigned char)s[L - 16 + i]) << (2 * i);
    p16[j] = w;
    edit_record_fill(s, ids[j], &t.records[j * 32]);
  }
  if (tile == 0) tile = SHORT_TILE_DEFAULT;
  const size_t ntile = np ? (np + tile - 1) / tile : 0, per = ntile ? (np + ntile - 1) / ntile : 0;
  t.tiles.resize(ntile);
  for (size_t ti = 0; ti < ntile; ++ti) {
    ShortTables::Tile &tt = t.tiles[ti];
    const size_t lo = ti * per, hi = std::min(np, lo + per), m = hi - lo;
    tt.base = (uint32_t)lo;
    tt.pat16.assign(p16.begin() + lo, p16.begin() + hi);
    tt.bitmap.assign((size_t)SHORT_PAIRS * SHORT_BM_WORDS, 0);
    tt.rows.assign((size_t)SHORT_PAIRS * SHORT_ROWS, 0);
    tt.runs.assign((size_t)SHORT_PAIRS * m, 0);
    for (int a = 0; a < 4; ++a) for (int b = a + 1; b < 4; ++b) {
      const int pr = pair_of(a, b);
      auto key_of = [&](uint32_t w) { return ((w >> (8 * a)) & 0xffu) | (((w >> (8 * b)) & 0xffu) << 8); };
      uint32_t *rows = &tt.rows[(size_t)pr * SHORT_ROWS];
      for (size_t j = 0; j < m; ++j) {                               // counting sort by key: rows[key] = first entry of the key's run
        const uint32_t key = key_of(tt.pat16[j]);
        tt.bitmap[(size_t)pr * SHORT_BM_WORDS + (key >> 5)] |= 1u << (key & 31u);
        ++rows[key + 1];
      }
      rows[0] = (uint32_t)((size_t)pr * m);
      for (int key = 0; key < 65536; ++key) rows[key + 1] += rows[key];
      std::vector<uint32_t> fill(rows, rows + 65536);
      for (size_t j = 0; j < m; ++j) tt.runs[fill[key_of(tt.pat16[j])]++] = (uint32_t)j;
    }
  }
  return "";
}

hipError_t short_upload(const ShortTables &t, ShortDevice *d, hipStream_t st) {
  short_free(d);
  d->k = t.k; d->maxlen = t.maxlen; d->ascii = t.ascii; d->eos_code = t.eos_code; d->npat = t.records.size() / 32;
  auto up = [&](const void *src, size_t bytes, void **dst) -> hipError_t {
    hipError_t e = hipMalloc(dst, bytes ? bytes : 16);
    if (e != hipSuccess) return e;
    return bytes ? hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  hipError_t e;
  if ((e = up(t.records.data(), t.records.size(), (void **)&d->records)) != hipSuccess) return e;
  d->tiles.resize(t.tiles.size());
  for (size_t i = 0; i < t.tiles.size(); ++i) {
    const ShortTables::Tile &s = t.tiles[i];
    ShortDevice::Tile &x = d->tiles[i];
    x.base = s.base;
    if ((e = up(s.bitmap.data(), s.bitmap.size() * 4, (void **)&x.bitmap)) != hipSuccess) return e;
    if ((e = up(s.rows.data(), s.rows.size() * 4, (void **)&x.rows)) != hipSuccess) return e;
    if ((e = up(s.runs.data(), s.runs.size() * 4, (void **)&x.runs)) != hipSuccess) return e;
    if ((e = up(s.pat16.data(), s.pat16.size() * 4, (void **)&x.pat16)) != hipSuccess) return e;
  }
  return hipStreamSynchronize(st);                                   // (the host tables may go now)
}

void short_free(ShortDevice *d) {
  if (d->records) (void)hipFree(d->records);
  for (ShortDevice::Tile &x : d->tiles) { void *ptrs[] = {x.bitmap, x.rows, x.runs, x.pat16}; for (void *p : ptrs) if (p) (void)hipFree(p); }
  *d = ShortDevice();
}

hipError_t short_launch(const ShortDevice &d, const uint8_t *d_text, const uint32_t *d_packed, int64_t n, int64_t begin, int64_t end,
                        pm_hit *d_out, unsigned long long *d_counter, uint64_t cap, uint64_t *d_seeds, unsigned long long *d_seed_count,
                        uint64_t seed_cap, hipStream_t st, ScanGeometry *geo_out) {
  if (!d_packed || !d_seeds || !d_seed_count) return hipErrorInvalidValue;
  if (end > n) end = n;
  ScanGeometry g;
  // a seed at window position p stands for the ends p - 1 .. p + 3: ends in (begin, end] come from begin - 2 <= p <= end + 1
  // (p beyond the last base: a match whose last characters are deleted keeps its frame)
  const int64_t p_lo = begin > 2 ? begin - 2 : 0, p_hi = end + 2;
  g.seg_len = end - begin >= ((int64_t)1 << 24) ? (int64_t)1 << 18 : (int64_t)1 << 16;
  const int64_t c_lo = p_lo / g.seg_len, c_hi = (p_hi - 1) / g.seg_len;
  g.nseg = end > begin ? (int)(c_hi - c_lo + 1) : 0;
  g.threads = SHORT_THREADS; g.blocks = g.nseg;
  if (geo_out) *geo_out = g;
  if (g.nseg <= 0 || d.tiles.empty()) return hipSuccess;
  for (const ShortDevice::Tile &x : d.tiles) {
    ShortArgs a;
    a.packed = d_packed; a.npacked = (n + 15) / 16; a.p_lo = p_lo; a.p_hi = p_hi; a.chunk0 = c_lo; a.chunk_len = g.seg_len;
    a.bitmap = x.bitmap; a.rows = x.rows; a.runs = x.runs; a.pat16 = x.pat16; a.tile_base = x.base;
    a.seed_out = d_seeds; a.seed_count = d_seed_count; a.seed_cap = seed_cap;
    if (d.k == 2) hipLaunchKernelGGL(pm_short_edit_scan<2>, dim3(g.nseg), dim3(SHORT_THREADS), 0, st, a);
    else hipLaunchKernelGGL(pm_short_edit_scan<1>, dim3(g.nseg), dim3(SHORT_THREADS), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return edits_verify_launch(d.records, d.k, d.maxlen, d.ascii, d.eos_code, d_text, n, begin, end, d_seeds, d_seed_count, seed_cap, d_out, d_counter, cap, st);
}

// ---- the substitution class: tables, launch ------------------------------------------------------------------------

std::string short_sub_build(const std::vector<Pattern> &pats, const std::vector<uint32_t> &ids, const Alphabet &alpha, int k, int eos_code,
                            size_t tile, ShortSubTables *out) {
  ShortSubTables &t = *out;
  t = ShortSubTables();
  if (k < 1 || k > 2) return "pm_short_sub_scan is built for k = 1 and k = 2";
  const bool norm = alpha.nch['A'] == 0 && alpha.nch['C'] == 1 && alpha.nch['G'] == 2 && alpha.nch['T'] == 3;
  const bool ascii = alpha.size == 256 && alpha.nch['A'] == 'A' && alpha.nch['C'] == 'C' && alpha.nch['G'] == 'G' && alpha.nch['T'] == 'T';
  if (!norm && !ascii) return "stream alphabet is neither A,C,G,T-normalized nor raw ASCII";
  t.k = k; t.ascii = ascii && !norm; t.eos_code = eos_code >= 0 && eos_code < 256 ? eos_code : -1;
  t.ncombos = sub_ncombos(k);
  for (int c = 0; c < t.ncombos; ++c) { t.fa[c] = sub_fa(k, c); t.fb[c] = sub_fb(k, c); }
  auto base2 = [&](unsigned char ch) -> int {                       // the stream's packing (pm_seed.hip pack4)
    switch (ch) { case 'A': return 0; case 'C': return 1; case 'G': return t.ascii ? 3 : 2; case 'T': return t.ascii ? 2 : 3; }
    return -1;
  };
  const size_t np = pats.size();
  if (np >= SUB_MAX_PATTERNS) return "too many patterns of 16..19 characters (21-bit pattern index)";
  t.pat_len.resize(np); t.pat_id.resize(np); t.pat_codes.assign(np * 32, 0); t.pat_zone.assign(np, 0);
  std::vector<uint32_t> p16(np);
  for (size_t j = 0; j < np; ++j) {
    const std::string &s = pats[j].s;
    const int L = (int)s.size();
    if (L < 16 || L > 19) return "pm_short_sub_scan takes patterns of 16..19 characters";
    for (int i = 0; i < L; ++i) {
      if (base2((unsigned char)s[i]) < 0) return "pattern with characters other than A,C,G,T";
      t.pat_codes[j * 32 + i] = (uint8_t)alpha.nch[(unsigned char)s[i]];
    }
    t.maxlen = std::max(t.maxlen, L);
    uint32_t w = 0;
    for (int i = 0; i < 16; ++i) w |= (uint32_t)base2((unsigned char)s[L - 16 + i]) << (2 * i);
    p16[j] = w;
    t.pat_len[j] = (uint8_t)L; t.pat_id[j] = ids[j];
    const int es = std::max(0, std::min(L, pats[j].esb)), ee = std::max(0, std::min(L, pats[j].eeb));
    uint32_t z = 0;
    for (int i = 0; i < L; ++i) if (i < es || i >= L - ee) z |= 1u << i;
    t.pat_zone[j] = z;
  }
  if (tile == 0) tile = SHORT_TILE_DEFAULT;
  const size_t ntile = np ? (np + tile - 1) / tile : 0, per = ntile ? (np + ntile - 1) / ntile : 0;
  t.tiles.resize(ntile);
  for (size_t ti = 0; ti < ntile; ++ti) {
    ShortSubTables::Tile &tt = t.tiles[ti];
    const size_t lo = ti * per, hi = std::min(np, lo + per), m = hi - lo;
    tt.base = (uint32_t)lo;
    tt.bitmap.assign((size_t)t.ncombos * SHORT_BM_WORDS, 0);
    tt.rows.assign((size_t)t.ncombos * SHORT_ROWS, 0);
    tt.runs.assign((size_t)t.ncombos * m, 0);
    for (int c = 0; c < t.ncombos; ++c) {
      uint32_t *rows = &tt.rows[(size_t)c * SHORT_ROWS];
      for (size_t j = 0; j < m; ++j) {                               // counting sort by key: rows[key] = first entry of the key's run
        const uint32_t key = sub_key(p16[lo + j], t.fa[c], t.fb[c]);
        tt.bitmap[(size_t)c * SHORT_BM_WORDS + (key >> 5)] |= 1u << (key & 31u);
        ++rows[key + 1];
      }
      rows[0] = (uint32_t)((size_t)c * m);
      for (int key = 0; key < 65536; ++key) rows[key + 1] += rows[key];
      std::vector<uint32_t> fill(rows, rows + 65536);
      for (size_t j = 0; j < m; ++j) tt.runs[fill[sub_key(p16[lo + j], t.fa[c], t.fb[c])]++] = (uint64_t)j | ((uint64_t)p16[lo + j] << 32);
    }
  }
  return "";
}

hipError_t short_sub_upload(const ShortSubTables &t, ShortSubDevice *d, hipStream_t st) {
  short_sub_free(d);
  d->k = t.k; d->maxlen = t.maxlen; d->ascii = t.ascii; d->eos_code = t.eos_code; d->ncombos = t.ncombos; d->npat = t.pat_len.size();
  for (int c = 0; c < SUB_MAX_COMBOS; ++c) { d->fa[c] = t.fa[c]; d->fb[c] = t.fb[c]; }
  auto up = [&](const void *src, size_t bytes, void **dst) -> hipError_t {
    hipError_t e = hipMalloc(dst, bytes ? bytes : 16);
    if (e != hipSuccess) return e;
    return bytes ? hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  hipError_t e;
  if ((e = up(t.pat_len.data(), t.pat_len.size(), (void **)&d->pat_len)) != hipSuccess) return e;
  if ((e = up(t.pat_id.data(), t.pat_id.size() * 4, (void **)&d->pat_id)) != hipSuccess) return e;
  if ((e = up(t.pat_codes.data(), t.pat_codes.size(), (void **)&d->pat_codes)) != hipSuccess) return e;
  if ((e = up(t.pat_zone.data(), t.pat_zone.size() * 4, (void **)&d->pat_zone)) != hipSuccess) return e;
  d->tiles.resize(t.tiles.size());
  for (size_t i = 0; i < t.tiles.size(); ++i) {
    const ShortSubTables::Tile &s = t.tiles[i];
    ShortSubDevice::Tile &x = d->tiles[i];
    x.base = s.base;
    if ((e = up(s.bitmap.data(), s.bitmap.size() * 4, (void **)&x.bitmap)) != hipSuccess) return e;
    if ((e = up(s.rows.data(), s.rows.size() * 4, (void **)&x.rows)) != hipSuccess) return e;
    if ((e = up(s.runs.data(), s.runs.size() * 8, (void **)&x.runs)) != hipSuccess) return e;
  }
  return hipStreamSynchronize(st);                                   // (the host tables may go now)
}

void short_sub_free(ShortSubDevice *d) {
  { void *ptrs[] = {d->pat_len, d->pat_id, d->pat_codes, d->pat_zone}; for (void *p : ptrs) if (p) (void)hipFree(p); }
  for (ShortSubDevice::Tile &x : d->tiles) { void *ptrs[] = {x.bitmap, x.rows, x.runs}; for (void *p : ptrs) if (p) (void)hipFree(p); }
  *d = ShortSubDevice();
}

hipError_t short_sub_launch(const ShortSubDevice &d, const uint8_t *d_text, const uint32_t *d_packed, int64_t n, int64_t begin, int64_t end,
                            pm_hit *d_out, unsigned long long *d_counter, uint64_t cap, uint64_t *d_susp, unsigned long long *d_susp_count,
                            uint64_t susp_cap, hipStream_t st) {
  if (!d_packed || !d_susp || !d_susp_count) return hipErrorInvalidValue;
  if (end > n) end = n;
  if (end <= begin || d.tiles.empty()) return hipSuccess;
  // a hit that ends at e (begin < e <= end) is the window whose last base is p = e - 1
  const int64_t seg_len = end - begin >= ((int64_t)1 << 24) ? (int64_t)1 << 18 : (int64_t)1 << 16;
  const int64_t c_lo = begin / seg_len, c_hi = (end - 1) / seg_len;
  const int nseg = (int)(c_hi - c_lo + 1);
  SubArgs a;
  memset(&a, 0, sizeof(a));
  a.text = d_text; a.n = n; a.packed = d_packed; a.npacked = (n + 15) / 16; a.p_lo = begin; a.p_hi = end; a.chunk0 = c_lo; a.chunk_len = seg_len;
  a.k = d.k; a.eos_code = d.eos_code; a.ncombos = d.ncombos; a.viol_level = d.viol_level;
  for (int c = 0; c < SUB_MAX_COMBOS; ++c) { a.fa[c] = d.fa[c]; a.fb[c] = d.fb[c]; }
  a.pat_len = d.pat_len; a.pat_id = d.pat_id; a.pat_codes = d.pat_codes; a.pat_zone = d.pat_zone;
  a.susp = d_susp; a.susp_count = d_susp_count; a.susp_cap = susp_cap;
  a.out = d_out; a.counter = d_counter; a.cap = cap;
  for (const ShortSubDevice::Tile &x : d.tiles) {
    a.bitmap = x.bitmap; a.rows = x.rows; a.runs = reinterpret_cast<const uint2 *>(x.runs); a.tile_base = x.base;
    if (d.k == 2) hipLaunchKernelGGL(pm_short_sub_scan<2>, dim3(nseg), dim3(SHORT_THREADS), 0, st, a);
    else hipLaunchKernelGGL(pm_short_sub_scan<1>, dim3(nseg), dim3(SHORT_THREADS), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pm_short_sub_verify, dim3(SUB_VERIFY_BLOCKS), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace pm
