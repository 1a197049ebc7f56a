// pm_short.hip -- patterns of 16..19 characters: the first stage of the edit-distance plan (pm_short_edit_scan, DESIGN.md
// 4.7) and the substitution class beside the pair plan (pm_short_sub_scan + pm_short_sub_verify).  The two
// scan kernels are ONE scan (short_scan: bitmaps in LDS, the wave's range, the key-hit queue, its drain, reserved slot
// blocks) around a struct each -- EditTests, SubCombos -- that says how windows become masks, how a run entry is judged
// and how a record is packed; their host tables come from one builder (pm_short_tables.h), one upload and one free.
// The same scan runs the wild class (pm_wild_sub_scan + pm_wild_sub_verify): -w primers of 16..32 characters
// with more than 16 concrete variants, keys expanded per field pair, everything else compared by class (WildCombos,
// pm_wild_tables.h).
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
#include "pm_bits.h"
#include "pm_internal.h"
#include "pm_seed.h"
#include "pm_short_tables.h"
#include "pm_slots.h"
#include "pm_verify.h"
#include "pm_wild_tables.h"

#include <algorithm>
#include <cstring>
#include <initializer_list>

namespace pm {

namespace {

constexpr int SHORT_THREADS = 256;                  // 4 waves share the bitmaps; 48 KiB + 16 KiB of queues: two workgroups per CU
constexpr int SHORT_WAVES = SHORT_THREADS / 64;
constexpr int SHORT_PAIRS = 6;
constexpr int SHORT_QCAP = 2048;                    // 2-byte key-hit entries per wave: two tests of a block (2 x 1024 windows) fit behind a drain
constexpr int SHORT_OUT_BLOCK = 256;                // seed list slots a wave reserves per atomic
constexpr int SUB_OUT_BLOCK = 64;                   // suspect slots a wave reserves per atomic
constexpr uint64_t SHORT_POS_MASK = 0xffffffffffull;   // both lists: position in the low 40 bits, class index of the pattern from bit 40 on

// ---- the scan both kernels are ------------------------------------------------------------------------------------------
// A workgroup holds the tile's key bitmaps in LDS; each of its waves walks its share of the workgroup's chunk in blocks of
// 1024 positions, 16 windows per lane.  Per block and round, a lane's windows become a mask (bit j / 16 + j: window j has
// the key of the round's first / second test in that test's bitmap); the set bits are queued in the wave's LDS queue and
// resolved with every lane busy: the key's run behind the offset table, one verdict per run entry, and what passes goes
// to slots of the output list that the wave reserves a block at a time.
//
// What a kernel supplies (EditTests, SubCombos below):
//   NBM, ROUNDS, OUT_BLOCK   bitmaps in LDS, masks per block, list slots per reservation
//   test(r, half)            the test a bit of round r's low / high half stands for (< 16)
//   load(pbase, own, s_bm)   the lane's stream words of a block (pbase = its first window; own = false: it has none)
//   mask<R>(s_bm)            the mask of round R
//   hit(bb, from, win, v)    a queued key hit -- window win of lane from in block bb, test v -- as the row of its key
//                            in the offset table and whatever judge needs of the window (called by the whole wave)
//   judge(h, cur, &pi)       run entry cur: its pattern (index inside the tile), and whether it leaves as a record
//   record(v, pi, p)         the 8-byte record of pattern pi at window position p
struct ShortScanArgs {
  const uint32_t *packed;               // the stream, 2 bits per base, 16 bases per dword
  int64_t npacked;
  int64_t p_lo, p_hi;                   // window positions lo <= p < hi (p = the window's last base)
  int64_t chunk0, chunk_len;            // first chunk (absolute, chunk_len aligned); positions per workgroup, a multiple of 1024 * SHORT_WAVES
  const uint32_t *bitmap;               // the tile's: [field pair][SHORT_BM_WORDS]
  const uint32_t *rows;                 //             [field pair][SHORT_ROWS]: first entry of the key's run in runs
  uint32_t tile_base;                   // index of the tile's first pattern in the class (records carry class indices)
  uint64_t *list;                       // seed records / suspects for the kernel behind the scan
  unsigned long long *list_count;
  unsigned long long list_cap;
};

// s_bm: P::NBM * SHORT_BM_WORDS words, s_q: SHORT_WAVES * SHORT_QCAP entries of the workgroup's LDS
template <typename P>
__device__ __forceinline__ void short_scan(const ShortScanArgs &a, P &pol, uint32_t *s_bm, uint16_t *s_q) {
  {
    const uint4 *src = reinterpret_cast<const uint4 *>(a.bitmap);
    uint4 *dst = reinterpret_cast<uint4 *>(s_bm);
    for (int i = threadIdx.x; i < P::NBM * SHORT_BM_WORDS / 4; i += SHORT_THREADS) dst[i] = src[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t sub = a.chunk_len / SHORT_WAVES;
  const int64_t ws = (a.chunk0 + (int64_t)blockIdx.x) * a.chunk_len + (int64_t)wave * sub;   // a multiple of 1024
  const int64_t lo = ws > a.p_lo ? ws : a.p_lo, hi = ws + sub < a.p_hi ? ws + sub : a.p_hi;
  if (lo >= hi) return;
  uint16_t *q = s_q + wave * SHORT_QCAP;                             // entries: lane << 8 | window << 4 | test
  int qn = 0;                                                       // wave-uniform: key hits queued
  SlotBlocks<P::OUT_BLOCK> out = {a.list, a.list_count, a.list_cap};

  // every queued key hit of block bb: the key's run, a verdict per entry, records
  auto drain = [&](int64_t bb) __attribute__((always_inline)) {
    for (int base = 0; base < qn; base += 64) {
      const bool valid = base + lane < qn;
      const uint32_t e = valid ? (uint32_t)q[base + lane] : 0u;
      const uint32_t from = e >> 8, win = (e >> 4) & 15u, v = e & 15u;
      const auto h = pol.hit(bb, from, win, v);
      uint32_t cur = 0, stop = 0;
      if (valid) { cur = a.rows[h.row]; stop = a.rows[h.row + 1]; }
      const int64_t p = bb + 16 * (int64_t)from + (int64_t)win;
      while (__ballot(cur < stop)) {
        bool pass = false;
        uint32_t pi = 0;
        if (cur < stop) { pass = pol.judge(h, cur, &pi); ++cur; }
        out.put(lane, pass, pol.record(v, pi, p));
      }
    }
    qn = 0;
  };

  for (int64_t bb = ws + (lo - ws) / 1024 * 1024; bb < hi; bb += 1024) {
    const int64_t pbase = bb + 16 * lane;                            // this lane's windows: p = pbase .. pbase + 15
    const uint32_t own = own_mask16(pbase, lo, hi);
    pol.load(pbase, own != 0, s_bm);                                 // (lanes outside the range read nothing: the range's halo bounds every load)
    static_for<P::ROUNDS>([&](auto R) __attribute__((always_inline)) {
      constexpr int r = decltype(R)::value;
      uint32_t m = pol.template mask<r>(s_bm) & (own | (own << 16));
      const int cnt = __popc(m);
      if (__ballot(cnt != 0)) {
        int x = cnt;                                                 // inclusive prefix sum over the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o); if (lane >= o) x += y; }
        const int total = __shfl(x, 63);
        if (qn + total > SHORT_QCAP) drain(bb);                      // (total <= SHORT_QCAP; the block's words stay where load put them)
        int at = qn + x - cnt;
        while (m) {
          const int b = __builtin_ctz(m);
          m &= m - 1u;
          q[at++] = (uint16_t)(((uint32_t)lane << 8) | ((uint32_t)(b & 15) << 4) | (uint32_t)(b < 16 ? P::test(r, 0) : P::test(r, 1)));
        }
        qn += total;
      }
    });
    if (qn) drain(bb);
  }
  out.mark_unused(lane);
}

// ---- edits: 14 tests (field pair, displacement) on four stream words, a q-gram count per run entry ------------------------
// the tests in table order (the pair-edit plan's): (0,1,0); (0,2,-1..1); (0,3,-2..2); (1,2,0); (1,3,-1..1); (2,3,0) -- the
// field pairs in the order of sub_fa(2, c) / sub_fb(2, c) (pm_verify.h)
constexpr int t_pair(int v) { const int t[SHORT_NTESTS] = {0, 1, 1, 1, 2, 2, 2, 2, 2, 3, 4, 4, 4, 5}; return t[v]; }
constexpr int t_d(int v) { const int t[SHORT_NTESTS] = {0, -1, 0, 1, -2, -1, 0, 1, 2, 0, -1, 0, 1, 0}; return t[v]; }
// A window's text: 20 bases from p - 17 on, base t at bits 2t of a 40-bit string; window base i (0..15) = t = i + 2.
constexpr int off_a(int v) { return 4 + 8 * sub_fa(2, t_pair(v)) - 2 * t_d(v); }   // field A, d bases early
constexpr int off_b(int v) { return 4 + 8 * sub_fb(2, t_pair(v)); }
constexpr uint32_t test_word(int v) { return (uint32_t)off_a(v) | ((uint32_t)off_b(v) << 8) | ((uint32_t)t_pair(v) << 16); }
__constant__ uint32_t SHORT_TEST[16] = {test_word(0), test_word(1), test_word(2), test_word(3), test_word(4), test_word(5), test_word(6),
                                        test_word(7), test_word(8), test_word(9), test_word(10), test_word(11), test_word(12), test_word(13), 0, 0};

struct ShortArgs : ShortScanArgs {
  const uint32_t *runs;                 // pattern indices (inside the tile) by pair and key
  const uint32_t *pat16;                // the patterns' last 16 bases, 2 bits each
};

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
struct EditTests {
  static constexpr int NBM = SHORT_PAIRS, ROUNDS = (K == 2 ? SHORT_NTESTS : 2) / 2, OUT_BLOCK = SHORT_OUT_BLOCK;
  static constexpr int test(int r, int half) { return K == 2 ? 2 * r + half : (half ? SHORT_NTESTS - 1 : 0); }   // (k = 1: the tests (0,1,0) and (2,3,0))
  struct Hit { uint32_t row, xlo, xhi; };                           // xlo : xhi as short_plausible takes them
  const ShortArgs &a;
  uint32_t w0, w1, w2, w3;                                          // the 64 bases from pbase - 32 on

  __device__ __forceinline__ void load(int64_t pbase, bool own, const uint32_t *) {
    w0 = w1 = w2 = w3 = 0;
    if (own) {
      w0 = load_packed(a.packed, a.npacked, pbase - 32); w1 = load_packed(a.packed, a.npacked, pbase - 16);
      w2 = load_packed(a.packed, a.npacked, pbase); w3 = load_packed(a.packed, a.npacked, pbase + 16);
    }
  }
  template <int R>
  __device__ __forceinline__ uint32_t mask(const uint32_t *s_bm) const {
    uint32_t m = 0;
    static_for<16>([&](auto J) __attribute__((always_inline)) {
      constexpr int j = decltype(J)::value, O = 30 + 2 * j;
      auto in_bitmap = [&](auto VV) __attribute__((always_inline)) -> uint32_t {
        constexpr int v = decltype(VV)::value, OA = O + off_a(v), OB = O + off_b(v), BM = t_pair(v) * SHORT_BM_WORDS;
        const uint32_t key = (bits_at<OA>(w0, w1, w2, w3) & 0xffu) | ((bits_at<OB>(w0, w1, w2, w3) & 0xffu) << 8);
        return (s_bm[BM + (key >> 5)] >> (key & 31u)) & 1u;
      };
      m |= in_bitmap(std::integral_constant<int, test(R, 0)>()) << j;
      m |= in_bitmap(std::integral_constant<int, test(R, 1)>()) << (16 + j);
    });
    return m;
  }
  __device__ __forceinline__ Hit hit(int64_t bb, uint32_t from, uint32_t win, uint32_t v) const {
    const uint32_t tw = SHORT_TEST[v];
    const int64_t pb = bb + 16 * (int64_t)from;
    const uint32_t x0 = load_packed(a.packed, a.npacked, pb - 32), x1 = load_packed(a.packed, a.npacked, pb - 16);
    const uint32_t x2 = load_packed(a.packed, a.npacked, pb), x3 = load_packed(a.packed, a.npacked, pb + 16);
    // the window's 40 bits start at bit 30 + 2 win of x0 : x1 : x2 : x3
    const bool up = win != 0;                                        // (bit 30 + 2 win >= 32)
    const uint32_t sh = (30u + 2u * win) & 31u;
    const uint32_t b0 = up ? x1 : x0, b1 = up ? x2 : x1, b2 = up ? x3 : x2;
    const uint32_t xlo = __builtin_amdgcn_alignbit(b1, b0, sh), xhi = __builtin_amdgcn_alignbit(b2, b1, sh);
    const uint32_t ka = __builtin_amdgcn_alignbit(xhi, xlo, tw & 31u) & 0xffu, kb = __builtin_amdgcn_alignbit(xhi, xlo, (tw >> 8) & 31u) & 0xffu;
    return {(tw >> 16) * (uint32_t)SHORT_ROWS + (ka | (kb << 8)), xlo, xhi};
  }
  __device__ __forceinline__ bool judge(const Hit &h, uint32_t cur, uint32_t *pi) const {
    *pi = a.runs[cur];
    return short_plausible<K>(a.pat16[*pi], h.xlo, h.xhi);
  }
  __device__ __forceinline__ uint64_t record(uint32_t, uint32_t pi, int64_t p) const {   // a seed: pattern i, position p
    return ((uint64_t)(a.tile_base + pi) << 40) | ((uint64_t)p & SHORT_POS_MASK);
  }
};

template <int K>
__global__ __launch_bounds__(SHORT_THREADS) void pm_short_edit_scan(ShortArgs a) {
  __shared__ uint32_t s_bm[SHORT_PAIRS * SHORT_BM_WORDS];
  __shared__ uint16_t s_q[SHORT_WAVES][SHORT_QCAP];
  EditTests<K> tests = {a, 0, 0, 0, 0};
  short_scan(a, tests, s_bm, s_q[0]);
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
constexpr int SUB_VERIFY_BLOCKS = 4096;
constexpr int SUB_INDEX_BITS = 21;                  // suspect: combo << 61 | class index of the pattern (21 bits) << 40 | position

struct SubArgs : ShortScanArgs {
  const uint2 *runs;                    // {pattern index inside the tile, its last 16 bases} by combo and key
  const uint8_t *text;                  // from here on: what pair_verify and pair_emit read (pm_verify.h)
  int64_t n;
  int k, eos_code, ncombos, viol_level;
  int fa[SUB_MAX_COMBOS], fb[SUB_MAX_COMBOS];
  const uint8_t *pat_len;               // the class's
  const uint32_t *pat_id;
  const uint8_t *pat_codes;
  const uint32_t *pat_zone;
  pm_hit *out;
  unsigned long long *counter;
  unsigned long long cap;
};

// the first (second) field of every combo, a nibble each: a lane looks up the fields of its own combo with a shift
template <int K>
constexpr uint32_t combo_fields(bool second) {
  uint32_t x = 0;
  for (int c = 0; c < sub_ncombos(K); ++c) x |= (uint32_t)(second ? sub_fb(K, c) : sub_fa(K, c)) << (4 * c);
  return x;
}

template <int K>
struct SubCombos {
  static constexpr int NC = sub_ncombos(K), NBM = NC, ROUNDS = NC / 2, OUT_BLOCK = SUB_OUT_BLOCK;
  static constexpr int test(int r, int half) { return 2 * r + half; }   // a test is a combo
  struct Hit { uint32_t row, W; };                                   // W: the window (sub_window)
  const SubArgs &a;
  uint32_t w1, w2;                                                  // the 32 bases from pbase - 16 on
  uint32_t m[ROUNDS];

  // all masks at once: every window is cut out of the words once, for all combos
  __device__ __forceinline__ void load(int64_t pbase, bool own, const uint32_t *s_bm) {
    w1 = 0; w2 = 0;
    if (own) { w1 = load_packed(a.packed, a.npacked, pbase - 16); w2 = load_packed(a.packed, a.npacked, pbase); }
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) m[r] = 0;
    static_for<16>([&](auto J) __attribute__((always_inline)) {
      constexpr int j = decltype(J)::value;
      const uint32_t W = sub_window(w1, w2, j);
      static_for<NC>([&](auto C) __attribute__((always_inline)) {
        constexpr int c = decltype(C)::value;
        const uint32_t key = sub_key(W, sub_fa(K, c), sub_fb(K, c));
        m[c / 2] |= ((s_bm[c * SHORT_BM_WORDS + (key >> 5)] >> (key & 31u)) & 1u) << (16 * (c & 1) + j);
      });
    });
  }
  template <int R>
  __device__ __forceinline__ uint32_t mask(const uint32_t *) const { return m[R]; }
  __device__ __forceinline__ Hit hit(int64_t, uint32_t from, uint32_t win, uint32_t c) const {
    const uint32_t W = sub_window((uint32_t)__shfl((int)w1, (int)from), (uint32_t)__shfl((int)w2, (int)from), win);
    const int fa = (int)((combo_fields<K>(false) >> (4u * c)) & 15u), fb = (int)((combo_fields<K>(true) >> (4u * c)) & 15u);
    return {c * (uint32_t)SHORT_ROWS + sub_key(W, fa, fb), W};
  }
  __device__ __forceinline__ bool judge(const Hit &h, uint32_t cur, uint32_t *pi) const {
    const uint2 r = a.runs[cur];
    *pi = r.x;
    return sub_others_within(h.W, r.y, K);
  }
  __device__ __forceinline__ uint64_t record(uint32_t c, uint32_t pi, int64_t p) const {
    return ((uint64_t)c << 61) | ((uint64_t)(a.tile_base + pi) << 40) | ((uint64_t)p & SHORT_POS_MASK);
  }
};

template <int K>
__global__ __launch_bounds__(SHORT_THREADS) void pm_short_sub_scan(SubArgs a) {
  __shared__ uint32_t s_bm[sub_ncombos(K) * SHORT_BM_WORDS];
  __shared__ uint16_t s_q[SHORT_WAVES][SHORT_QCAP];
  SubCombos<K> combos = {a, 0, 0, {}};
  short_scan(a, combos, s_bm, s_q[0]);
}

// The scan's suspects, one per thread: the pair plan's exact stage with fields of four bases.  Records leave through the
// workgroup's LDS stage (verify_staged), as in pm_pair_verify.
__global__ __launch_bounds__(256) void pm_short_sub_verify(SubArgs a) {
  unsigned long long n = *a.list_count;
  if (n > a.list_cap) n = a.list_cap;
  verify_staged(a, n, [&](unsigned long long i, const VerifyStage &, pm_hit *hh) __attribute__((always_inline)) {
    const uint64_t r = a.list[i];
    return r != ~0ull &&                                              // (a slot its wave reserved and did not need)
           pair_verify<4>(a, (int)(r >> 61), (int64_t)(r & SHORT_POS_MASK), (uint32_t)(r >> 40) & ((1u << SUB_INDEX_BITS) - 1u), hh);
  });
}

// ---- the wild class: -w primers with more than 16 concrete variants, compared by class -----------------
//
//   pm_wild_sub_scan     pm_short_sub_scan's scan -- same windows, same key lookup in LDS -- over bitmaps that hold every key in
//                        the cross product of the classes of a field pair's eight bases (pm_wild_tables.h).  A run entry is
//                        {primer, class word}: four bits per base for the eight bases outside the key, so one read settles a
//                        key hit here too: the window's other eight bases become one bit each in their nibble, AND + popcount.
//                        k = 0 runs the k = 1 instance (two bitmaps), every primer entered under one of the two pairs.
//   pm_wild_sub_verify   wild_verify<4> of pm_verify.h per suspect: pair_verify with the per-byte verdict by class.
//   pm_wild_sub_verify_wide   the same loop over wild_verify<4, 64>, for a class that holds a primer of 33..64 characters
//                        (DESIGN.md 4.14).  The scan, the suspects and their counter are the same.
//
// N, end-of-sequence and positions outside the stream pack to arbitrary bases, as above: such a window can only gain
// suspects, and it cannot lose a candidate -- such a character is one of the <= k mismatches and leaves two clean fields.
struct WildArgs : SubArgs {
  const uint8_t *pat_class;             // 16 bytes per primer, 32 in a wide class (pat_codes is unused)
  const uint8_t *pat_reg;
  int ascii;
};

template <int K>
struct WildCombos : SubCombos<K> {
  struct Hit { uint32_t row, others; };                              // others: the window's eight bases outside the key (wild_others)
  __device__ __forceinline__ Hit hit(int64_t bb, uint32_t from, uint32_t win, uint32_t c) const {
    const typename SubCombos<K>::Hit b = SubCombos<K>::hit(bb, from, win, c);
    const int fa = (int)((combo_fields<K>(false) >> (4u * c)) & 15u), fb = (int)((combo_fields<K>(true) >> (4u * c)) & 15u);
    return {b.row, wild_others(b.W, fa, fb)};
  }
  __device__ __forceinline__ bool judge(const Hit &h, uint32_t cur, uint32_t *pi) const {
    const uint2 r = this->a.runs[cur];
    *pi = r.x;
    return wild_others_within(h.others, r.y, this->a.k);
  }
};

template <int K>
__global__ __launch_bounds__(SHORT_THREADS) void pm_wild_sub_scan(WildArgs a) {
  __shared__ uint32_t s_bm[sub_ncombos(K) * SHORT_BM_WORDS];
  __shared__ uint16_t s_q[SHORT_WAVES][SHORT_QCAP];
  WildCombos<K> combos = {{a, 0, 0, {}}};
  short_scan(a, combos, s_bm, s_q[0]);
}

__global__ __launch_bounds__(256) void pm_wild_sub_verify(WildArgs a) {
  unsigned long long n = *a.list_count;
  if (n > a.list_cap) n = a.list_cap;
  verify_staged(a, n, [&](unsigned long long i, const VerifyStage &, pm_hit *hh) __attribute__((always_inline)) {
    const uint64_t r = a.list[i];
    return r != ~0ull &&                                              // (a slot its wave reserved and did not need)
           wild_verify<4>(a, (int)(r >> 61), (int64_t)(r & SHORT_POS_MASK), (uint32_t)(r >> 40) & ((1u << SUB_INDEX_BITS) - 1u), hh);
  });
}

// a class that holds a primer of 33..64 characters: rows of 64 class nibbles, zone masks of two dwords
__global__ __launch_bounds__(256) void pm_wild_sub_verify_wide(WildArgs a) {
  unsigned long long n = *a.list_count;
  if (n > a.list_cap) n = a.list_cap;
  verify_staged(a, n, [&](unsigned long long i, const VerifyStage &, pm_hit *hh) __attribute__((always_inline)) {
    const uint64_t r = a.list[i];
    return r != ~0ull &&                                              // (a slot its wave reserved and did not need)
           wild_verify<4, 64>(a, (int)(r >> 61), (int64_t)(r & SHORT_POS_MASK), (uint32_t)(r >> 40) & ((1u << SUB_INDEX_BITS) - 1u), hh);
  });
}

// ---- host: tables ------------------------------------------------------------------------------------------------------
// What the two classes' builds share: the option and alphabet checks, the patterns' last 16 bases in the stream's packing,
// the split into tiles.
struct ShortClassPlan {
  bool ascii = false;
  int eos_code = -1, maxlen = 0;
  std::vector<uint32_t> tail;           // per pattern: its last 16 bases, 2 bits each
  size_t ntile = 0, per = 0;            // tiles of `per` patterns (the last one may hold fewer)
};

// index_bits: what a record of the kernel has for the pattern's class index
std::string short_class_plan(const std::string &kernel, const std::vector<Pattern> &pats, const Alphabet &alpha, int k, int eos_code, int index_bits,
                             size_t tile, ShortClassPlan *c) {
  if (k < 1 || k > 2) return kernel + " is built for k = 1 and k = 2";
  const bool norm = alpha.nch['A'] == 0 && alpha.nch['C'] == 1 && alpha.nch['G'] == 2 && alpha.nch['T'] == 3;
  const bool ascii = alpha.size == 256 && alpha.nch['A'] == 'A' && alpha.nch['C'] == 'C' && alpha.nch['G'] == 'G' && alpha.nch['T'] == 'T';
  if (!norm && !ascii) return "stream alphabet is neither A,C,G,T-normalized nor raw ASCII";
  c->ascii = ascii && !norm; c->eos_code = eos_code >= 0 && eos_code < 256 ? eos_code : -1;
  auto base2 = [&](unsigned char ch) -> int {                       // the stream's packing (pm_seed.hip pack4)
    switch (ch) { case 'A': return 0; case 'C': return 1; case 'G': return c->ascii ? 3 : 2; case 'T': return c->ascii ? 2 : 3; }
    return -1;
  };
  const size_t np = pats.size();
  if (np >= ((size_t)1 << index_bits)) return "too many patterns of 16..19 characters (" + std::to_string(index_bits) + "-bit pattern index)";
  c->tail.resize(np);
  for (size_t j = 0; j < np; ++j) {
    const std::string &s = pats[j].s;
    const int L = (int)s.size();
    if (L < 16 || L > 19) return kernel + " takes patterns of 16..19 characters";
    for (unsigned char ch : s) if (base2(ch) < 0) return "pattern with characters other than A,C,G,T";
    c->maxlen = std::max(c->maxlen, L);
    uint32_t w = 0;
    for (int i = 0; i < 16; ++i) w |= (uint32_t)base2((unsigned char)s[L - 16 + i]) << (2 * i);
    c->tail[j] = w;
  }
  if (tile == 0) tile = SHORT_TILE_DEFAULT;
  c->ntile = np ? (np + tile - 1) / tile : 0; c->per = c->ntile ? (np + c->ntile - 1) / c->ntile : 0;
  return "";
}

// The tiles' key indices (pm_short_tables.h) over the field pairs (fa[c], fb[c]); runs(tile, tails of the tile's patterns,
// their order by pair and key) makes the kernel's run entries of the order.
template <typename Tile, typename Runs>
void short_tiles(const ShortClassPlan &c, int npairs, const int *fa, const int *fb, std::vector<Tile> *tiles, Runs &&runs) {
  tiles->resize(c.ntile);
  for (size_t ti = 0; ti < c.ntile; ++ti) {
    Tile &tt = (*tiles)[ti];
    const size_t lo = ti * c.per, hi = std::min(c.tail.size(), lo + c.per);
    ShortKeyIndex x = short_key_index(c.tail.data() + lo, hi - lo, npairs, fa, fb);
    tt.base = (uint32_t)lo;
    tt.bitmap = std::move(x.bitmap); tt.rows = std::move(x.rows);
    runs(tt, c.tail.data() + lo, hi - lo, x.order);
  }
}

// hipMalloc + copy of one table after the other; the first error stays
struct Upload {
  hipStream_t st;
  hipError_t err = hipSuccess;
  template <typename T, typename D>
  void operator()(const std::vector<T> &src, D **dst) {
    if (err != hipSuccess) return;
    const size_t bytes = src.size() * sizeof(T);
    err = hipMalloc((void **)dst, bytes ? bytes : 16);
    if (err == hipSuccess && bytes) err = hipMemcpyAsync(*dst, src.data(), bytes, hipMemcpyHostToDevice, st);
  }
  template <typename Tile>
  void tile(const Tile &s, ShortTileDevice *x) { x->base = s.base; (*this)(s.bitmap, &x->bitmap); (*this)(s.rows, &x->rows); (*this)(s.runs, &x->runs); }
  hipError_t done() const { return err != hipSuccess ? err : hipStreamSynchronize(st); }   // (the host tables may go now)
};

void free_tables(std::initializer_list<void *> ptrs, std::vector<ShortTileDevice> *tiles) {
  for (void *p : ptrs) if (p) (void)hipFree(p);
  for (ShortTileDevice &x : *tiles) for (void *p : {(void *)x.bitmap, (void *)x.rows, x.runs, (void *)x.pat16}) if (p) (void)hipFree(p);
}

}  // namespace

std::string short_build(const std::vector<Pattern> &pats, const std::vector<uint32_t> &ids, const Alphabet &alpha, int k, int eos_code,
                        size_t tile, ShortTables *out) {
  ShortTables &t = *out;
  t = ShortTables();
  ShortClassPlan c;
  const std::string why = short_class_plan("pm_short_edit_scan", pats, alpha, k, eos_code, 22, tile, &c);
  if (!why.empty()) return why;
  t.k = k; t.ascii = c.ascii; t.eos_code = c.eos_code; t.maxlen = c.maxlen;
  t.records.assign(pats.size() * 32, 0);
  for (size_t j = 0; j < pats.size(); ++j) edit_record_fill(pats[j].s, ids[j], &t.records[j * 32]);
  int fa[SHORT_PAIRS], fb[SHORT_PAIRS];                              // all six pairs, in the substitution plan's order at k = 2
  for (int p = 0; p < SHORT_PAIRS; ++p) { fa[p] = sub_fa(2, p); fb[p] = sub_fb(2, p); }
  short_tiles(c, SHORT_PAIRS, fa, fb, &t.tiles, [](ShortTables::Tile &tt, const uint32_t *tail, size_t m, std::vector<uint32_t> &order) {
    tt.runs = std::move(order);
    tt.pat16.assign(tail, tail + m);
  });
  return "";
}

hipError_t short_upload(const ShortTables &t, ShortDevice *d, hipStream_t st) {
  short_free(d);
  d->k = t.k; d->maxlen = t.maxlen; d->ascii = t.ascii; d->eos_code = t.eos_code; d->npat = t.records.size() / 32;
  Upload up = {st};
  up(t.records, &d->records);
  d->tiles.resize(t.tiles.size());
  for (size_t i = 0; i < t.tiles.size(); ++i) { up.tile(t.tiles[i], &d->tiles[i]); up(t.tiles[i].pat16, &d->tiles[i].pat16); }
  return up.done();
}

void short_free(ShortDevice *d) {
  free_tables({d->records}, &d->tiles);
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
  for (const ShortTileDevice &x : d.tiles) {
    ShortArgs a;
    a.packed = d_packed; a.npacked = (n + 15) / 16; a.p_lo = p_lo; a.p_hi = p_hi; a.chunk0 = c_lo; a.chunk_len = g.seg_len;
    a.bitmap = x.bitmap; a.rows = x.rows; a.runs = static_cast<const uint32_t *>(x.runs); a.pat16 = x.pat16; a.tile_base = x.base;
    a.list = d_seeds; a.list_count = d_seed_count; a.list_cap = seed_cap;
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
  ShortClassPlan c;
  const std::string why = short_class_plan("pm_short_sub_scan", pats, alpha, k, eos_code, SUB_INDEX_BITS, tile, &c);
  if (!why.empty()) return why;
  t.k = k; t.ascii = c.ascii; t.eos_code = c.eos_code; t.maxlen = c.maxlen;
  t.ncombos = sub_ncombos(k);
  for (int p = 0; p < t.ncombos; ++p) { t.fa[p] = sub_fa(k, p); t.fb[p] = sub_fb(k, p); }
  const size_t np = pats.size();
  t.pat_len.resize(np); t.pat_id.resize(np); t.pat_codes.assign(np * 32, 0); t.pat_zone.assign(np, 0);
  for (size_t j = 0; j < np; ++j) {
    const std::string &s = pats[j].s;
    const int L = (int)s.size();
    for (int i = 0; i < L; ++i) t.pat_codes[j * 32 + i] = (uint8_t)alpha.nch[(unsigned char)s[i]];
    t.pat_len[j] = (uint8_t)L; t.pat_id[j] = ids[j];
    const int es = std::max(0, std::min(L, pats[j].esb)), ee = std::max(0, std::min(L, pats[j].eeb));
    uint32_t z = 0;
    for (int i = 0; i < L; ++i) if (i < es || i >= L - ee) z |= 1u << i;
    t.pat_zone[j] = z;
  }
  short_tiles(c, t.ncombos, t.fa, t.fb, &t.tiles, [](ShortSubTables::Tile &tt, const uint32_t *tail, size_t, const std::vector<uint32_t> &order) {
    tt.runs.resize(order.size());
    for (size_t i = 0; i < order.size(); ++i) tt.runs[i] = (uint64_t)order[i] | ((uint64_t)tail[order[i]] << 32);
  });
  return "";
}

hipError_t short_sub_upload(const ShortSubTables &t, ShortSubDevice *d, hipStream_t st) {
  short_sub_free(d);
  d->k = t.k; d->maxlen = t.maxlen; d->ascii = t.ascii; d->eos_code = t.eos_code; d->ncombos = t.ncombos; d->npat = t.pat_len.size();
  for (int c = 0; c < SUB_MAX_COMBOS; ++c) { d->fa[c] = t.fa[c]; d->fb[c] = t.fb[c]; }
  Upload up = {st};
  up(t.pat_len, &d->pat_len); up(t.pat_id, &d->pat_id); up(t.pat_codes, &d->pat_codes); up(t.pat_zone, &d->pat_zone);
  d->tiles.resize(t.tiles.size());
  for (size_t i = 0; i < t.tiles.size(); ++i) up.tile(t.tiles[i], &d->tiles[i]);
  return up.done();
}

void short_sub_free(ShortSubDevice *d) {
  free_tables({d->pat_len, d->pat_id, d->pat_codes, d->pat_zone}, &d->tiles);
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
  a.list = d_susp; a.list_count = d_susp_count; a.list_cap = susp_cap;
  a.out = d_out; a.counter = d_counter; a.cap = cap;
  for (const ShortTileDevice &x : d.tiles) {
    a.bitmap = x.bitmap; a.rows = x.rows; a.runs = static_cast<const uint2 *>(x.runs); a.tile_base = x.base;
    if (d.k == 2) hipLaunchKernelGGL(pm_short_sub_scan<2>, dim3(nseg), dim3(SHORT_THREADS), 0, st, a);
    else hipLaunchKernelGGL(pm_short_sub_scan<1>, dim3(nseg), dim3(SHORT_THREADS), 0, st, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(pm_short_sub_verify, dim3(SUB_VERIFY_BLOCKS), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---- the wild class: tables, launch --------------------------------------------------------------------------------

static_assert(WILD_MAX_ENTRIES == SHORT_SUB_MAX_PATTERNS, "the wild class's entry cap is the short substitution class's measured ceiling (pm_wild_tables.h cannot see pm_internal.h)");
bool wild_takes(const std::string &s, int k, size_t maxL) { return wild_primer_fits(s, k, maxL); }
bool wild_class_fits(const std::vector<std::string> &pats, int k) { return wild_entries_fit(pats, k); }

std::string wild_build(const std::vector<Pattern> &pats, const std::vector<uint32_t> &ids, const Alphabet &alpha, int k, int eos_code, WildTables *out) {
  WildTables &t = *out;
  t = WildTables();
  const bool norm = alpha.nch['A'] == 0 && alpha.nch['C'] == 1 && alpha.nch['G'] == 2 && alpha.nch['T'] == 3;
  const bool ascii = alpha.size == 256 && alpha.nch['A'] == 'A' && alpha.nch['C'] == 'C' && alpha.nch['G'] == 'G' && alpha.nch['T'] == 'T';
  if (!norm && !ascii) return "stream alphabet is neither A,C,G,T-normalized nor raw ASCII";
  const size_t np = pats.size();
  if (np >= ((size_t)1 << SUB_INDEX_BITS)) return "too many primers in the wild class";
  std::vector<std::string> strs(np);
  for (size_t j = 0; j < np; ++j) strs[j] = pats[j].s;
  WildIndex x;
  const std::string why = wild_build_index(strs, k, ascii && !norm, &x);
  if (!why.empty()) return why;
  t.k = k; t.ascii = x.ascii; t.eos_code = eos_code >= 0 && eos_code < 256 ? eos_code : -1; t.ncombos = x.ncombos;
  for (int c = 0; c < x.ncombos; ++c) { t.fa[c] = x.fa[c]; t.fb[c] = x.fb[c]; }
  t.wide = x.row_bytes == 32;                                        // (a primer of 33..64 characters: every row of the class is wide)
  const size_t zw = t.wide ? 2 : 1;
  t.pat_len.resize(np); t.pat_id.resize(np); t.pat_zone.assign(np * zw, 0);
  for (size_t j = 0; j < np; ++j) {
    const int L = (int)strs[j].size();
    t.maxlen = std::max(t.maxlen, L);
    if (L > 32) ++t.nlong;
    t.pat_len[j] = (uint8_t)L; t.pat_id[j] = ids[j];
    const int es = std::max(0, std::min(L, pats[j].esb)), ee = std::max(0, std::min(L, pats[j].eeb));
    uint64_t z = 0;
    for (int i = 0; i < L; ++i) if (i < es || i >= L - ee) z |= 1ull << i;
    t.pat_zone[j * zw] = (uint32_t)z;
    if (t.wide) t.pat_zone[j * zw + 1] = (uint32_t)(z >> 32);
  }
  for (size_t e : x.entries) t.max_entries = std::max(t.max_entries, e);
  t.pat_class = std::move(x.pat_class); t.pat_reg = std::move(x.reg);
  t.bitmap = std::move(x.bitmap); t.rows = std::move(x.rows); t.runs = std::move(x.runs);
  return "";
}

hipError_t wild_upload(const WildTables &t, WildDevice *d, hipStream_t st) {
  wild_free(d);
  d->k = t.k; d->maxlen = t.maxlen; d->ascii = t.ascii; d->wide = t.wide; d->nlong = t.nlong; d->eos_code = t.eos_code; d->ncombos = t.ncombos; d->npat = t.pat_len.size();
  d->max_entries = t.max_entries;
  for (int c = 0; c < SUB_MAX_COMBOS; ++c) { d->fa[c] = t.fa[c]; d->fb[c] = t.fb[c]; }
  Upload up = {st};
  up(t.pat_len, &d->pat_len); up(t.pat_id, &d->pat_id); up(t.pat_class, &d->pat_class); up(t.pat_reg, &d->pat_reg); up(t.pat_zone, &d->pat_zone);
  d->tiles.resize(1);
  up(t.bitmap, &d->tiles[0].bitmap); up(t.rows, &d->tiles[0].rows); up(t.runs, &d->tiles[0].runs);
  return up.done();
}

void wild_free(WildDevice *d) {
  free_tables({d->pat_len, d->pat_id, d->pat_class, d->pat_reg, d->pat_zone}, &d->tiles);
  *d = WildDevice();
}

hipError_t wild_launch(const WildDevice &d, const uint8_t *d_text, const uint32_t *d_packed, int64_t n, int64_t begin, int64_t end,
                       pm_hit *d_out, unsigned long long *d_counter, uint64_t cap, uint64_t *d_susp, unsigned long long *d_susp_count,
                       uint64_t susp_cap, hipStream_t st, ScanGeometry *geo_out) {
  if (!d_packed || !d_susp || !d_susp_count) return hipErrorInvalidValue;
  if (end > n) end = n;
  // a hit that ends at e (begin < e <= end) is the window whose last base is p = e - 1
  const int64_t seg_len = end - begin >= ((int64_t)1 << 24) ? (int64_t)1 << 18 : (int64_t)1 << 16;
  const int64_t c_lo = begin / seg_len, c_hi = end > begin ? (end - 1) / seg_len : c_lo - 1;
  const int nseg = (int)(c_hi - c_lo + 1);
  if (geo_out) { geo_out->seg_len = seg_len; geo_out->nseg = nseg; geo_out->blocks = nseg; geo_out->threads = SHORT_THREADS; geo_out->work_map = 0; }
  if (end <= begin || d.tiles.empty()) return hipSuccess;
  WildArgs a;
  memset(&a, 0, sizeof(a));
  a.text = d_text; a.n = n; a.packed = d_packed; a.npacked = (n + 15) / 16; a.p_lo = begin; a.p_hi = end; a.chunk0 = c_lo; a.chunk_len = seg_len;
  a.k = d.k; a.eos_code = d.eos_code; a.ncombos = d.ncombos; a.viol_level = d.viol_level; a.ascii = d.ascii ? 1 : 0;
  for (int c = 0; c < SUB_MAX_COMBOS; ++c) { a.fa[c] = d.fa[c]; a.fb[c] = d.fb[c]; }
  a.pat_len = d.pat_len; a.pat_id = d.pat_id; a.pat_class = d.pat_class; a.pat_reg = d.pat_reg; a.pat_zone = d.pat_zone;
  a.list = d_susp; a.list_count = d_susp_count; a.list_cap = susp_cap;
  a.out = d_out; a.counter = d_counter; a.cap = cap;
  const ShortTileDevice &x = d.tiles[0];
  a.bitmap = x.bitmap; a.rows = x.rows; a.runs = static_cast<const uint2 *>(x.runs); a.tile_base = x.base;
  if (d.k == 2) hipLaunchKernelGGL(pm_wild_sub_scan<2>, dim3(nseg), dim3(SHORT_THREADS), 0, st, a);
  else hipLaunchKernelGGL(pm_wild_sub_scan<1>, dim3(nseg), dim3(SHORT_THREADS), 0, st, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (d.wide) hipLaunchKernelGGL(pm_wild_sub_verify_wide, dim3(SUB_VERIFY_BLOCKS), dim3(256), 0, st, a);   // (the class's rows hold 64 characters)
  else hipLaunchKernelGGL(pm_wild_sub_verify, dim3(SUB_VERIFY_BLOCKS), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace pm
