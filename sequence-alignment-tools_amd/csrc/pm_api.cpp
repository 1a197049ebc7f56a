// pm_api.cpp -- the C ABI of include/pm_gpu.h: handle life cycle, engine selection, the device
// scan stage and the host verify/cluster stage.
//
// Split of work (DESIGN.md "stages"):
//   device  : scan kernels (pm_bitpar.hip / pm_seed.hip) turn the stream into sparse candidate
//             records -- a pure function of (stream range, patterns), so it shards by position;
//   host    : the order-dependent, sparse part of the reference wrappers -- filter_bitvec's
//             clustering + one verify per cluster (filter_bitvec.cc:88-177), exact_halves'
//             seed extension + per-pattern dedup (exact_halves.cc:140-190), exact_bases
//             (exact_bases.cc:92-121) -- in stream order over the gathered records.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <chrono>
#include <thread>
#include <unordered_map>

#include "pm_internal.h"
#include "pm_iupac.h"
#include "pm_seed.h"
#include "pm_pair.h"

using namespace pm;

namespace pm {
void Alphabet::set_raw() {
  size = 256;
  for (int i = 0; i < 256; ++i) { ch[i] = (uint8_t)i; nch[i] = i; present[i] = true; }
}
void Alphabet::set_table(const uint8_t *table, int len) {      // char_io.t:222-236
  size = len;
  for (int i = 0; i < 256; ++i) { ch[i] = 0; nch[i] = -1; present[i] = true; }
  for (int i = 0; i < len; ++i) { ch[i] = table[i]; nch[table[i]] = i; }
}
}  // namespace pm

// windowed stream (pm_init_windowed): host -> HBM in chunks through pinned staging buffers, one HIP stream per thread
constexpr int WIN_UP_THREADS = 4;
constexpr int64_t WIN_UP_CHUNK = (int64_t)4 << 20;

// One slot of the window ring: stream text [lo, hi) at bytes + guard (and its 2-bit words at words + guard / 16), with
// guard margins of unused memory on both sides: a stage that reads beyond its computed reach gets wrong characters, never
// memory outside an allocation.
struct WinSlot {
  uint8_t *bytes = nullptr;
  uint32_t *words = nullptr;
  uint8_t *pk = nullptr;              // pm_init_packed: the window's bit-packed bytes as they crossed PCIe (unpacked into bytes / words)
  int64_t cap = 0, lo = 0, hi = 0;
  bool loaded = false, used_rec = false;
  hipEvent_t ready = nullptr;         // upload + packing done (recorded on the upload stream)
  hipEvent_t used = nullptr;          // the last kernel that reads the slot (recorded on the handle's stream when it is unbound)
};

// The host-side rules that add a few records at the stream's edges, where the scan kernels have no whole window.  Each
// rule's records depend on the stream and the patterns only: built once per init, handed to whatever range holds their end.
enum EdgeRule {
  EDGE_EDITS_START,                   // edits: candidates that end in the first Lw+2k+2 characters (edits_start_candidates)
  EDGE_EDITS_END,                     // edits: candidates that end in the last four characters (edits_end_candidates)
  EDGE_STREAM_START,                  // -K on the automaton's semantics: records of the stream start (stream_start_candidates)
  EDGE_OVERHANG,                      // exact_halves / exact_bases -K: hits that hang over the end of the stream (stream_end_overhang_candidates)
  EDGE_BLOCKS,                        // exact_bases -k: block occurrences in the first and last 56 characters (bases_edge_candidates)
  EDGE_RULES
};
struct EdgeRecords {
  std::vector<pm_hit> recs;
  bool built = false;
};

struct pm_handle {
  pm_config cfg{};
  Knobs knobs;                        // the environment's test / measurement knobs as pm_create found them
  std::vector<Pattern> pats;
  std::unordered_map<uint32_t, uint32_t> id2idx;   // caller's pattern id -> index into pats
  Alphabet alpha;
  int eos_code = -1;
  int sem = 0, kern = 0;
  bool inited = false;
  bool host_only = false;             // pm_init_host: host stage only, no stream on the device

  const uint8_t *h_text = nullptr;
  // pm_init_packed: the host form of the stream is bit-packed (pk_bits bits per code, MSB first) and h_text is NULL
  const uint8_t *h_packed = nullptr;
  int64_t h_packed_bytes = 0;
  int pk_bits = 0;
  int64_t pk_peak_extra = 0;          // resident form: HBM the packed staging buffer held during init
  const uint8_t *d_text = nullptr;
  bool own_d_text = false;
  int64_t n = 0;
  hipStream_t stream = nullptr;

  // device stage
  std::vector<Pattern> inner;
  std::vector<uint32_t> inner_ids;
  BitparDevice bp;
  SeedDevice sd;                      // first pattern tile (plan parameters are read from here)
  std::vector<SeedDevice> sd_more;    // further tiles when the pattern set is too large for one LDS filter
  std::vector<PairDevice> pair;       // -K 1 / -K 2 on 20..32 character patterns: the pair plan's tiles (pm_pair.hip) instead of sd
  std::vector<PairDevice> epair;      // the pair geometry as the edit plan's first stage: a table set per seed tile (same cut, same pattern order as sd / sd_more).
                                      // -k 2 on one tile without exact_bases; with the PM_EDIT_PAIR bit also every tile, -k 1 and exact_bases
  unsigned long long last_suspects = 0;   // suspects of the last scan's fullest tile (pm_scan_stats [8])
  bool epair_on = false;              // all tiles or none: routes are never mixed across tiles
  bool seed_flags = false;            // exact_halves on whole-pattern Hamming candidates (aux flags)
  bool bases_flags = false;           // exact_bases -K on whole-pattern Hamming candidates with clean exact zones (pair plan): records are final
  bool zoned = false;                 // some pattern has exact-base constraints
  bool nn_quirk = false;              // -w without -W on a stream that holds N, and some pattern has the letter N (pattern_n_quirk)
  bool wild_seed = false;             // -w/-W on the seed family: primers with <= 2 ambiguity letters expanded into their concrete variants
  bool bases_edits = false;           // exact_bases -k on the seed family: the k-error automaton's candidates -> block seeds (pm_bases_seeds)
  int64_t own_begin = 0, own_end = 0; //   the range the caller asked for (the candidates are scanned a little wider)
  bool halves_dev = false;            // exact_halves -k: half seeds extended by pm_seed_extend on the GPU
  bool half_ranked_any = false;       // ... and some pattern tile runs on pm_half_scan (needs the seed record buffer)
  bool edits_dev = false;             // filter_bitvec / shift_and_inexact -k on the seed kernels: records deduplicated after the scan
  unsigned long long *d_seed_count = nullptr;   // edits: [0] unused, [1+t] seed records of tile t
  uint64_t *d_seeds = nullptr;                  // edits: 8-byte seed records between the scan and the verify kernel
  size_t seed_cap = 0;
  void *d_susp = nullptr;                       // pair plan: 16-byte suspect records between its scan and verify kernels
  size_t susp_cap = 0;
  unsigned long long *h_seed_count = nullptr;   // pinned, 1 + 256 entries: a copy into pageable memory would make the "async" scan call wait for the kernels
  EdgeRecords edge[EDGE_RULES];       // the records the host adds at the stream's edges, per rule
  uint8_t *d_dp_codes = nullptr;      // device DP (pm_cluster_dp): 32 stream codes per pattern (64 with nlong_edits), exact zones
  int32_t *d_dp_esb = nullptr, *d_dp_eeb = nullptr;
  pm_hit *d_ext = nullptr;            // its output (swapped with d_cands after every scan)
  uint8_t *d_half_codes = nullptr, *d_half_len = nullptr;
  int32_t *d_hesb = nullptr, *d_heeb = nullptr;
  int scan_k = 0, seed_k = 0;
  int64_t scan_end = 0;               // end of the range of the scan in flight / last scan
  bool scan_indels = false;
  pm_hit *d_cands = nullptr;
  unsigned long long *d_counter = nullptr;
  unsigned long long *h_counter = nullptr;     // pinned
  size_t cap = 0;
  size_t last_count = 0;
  int64_t scan_begin = 0;
  bool scan_pending = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  float last_ms = 0.f;
  int last_launches = 0;
  unsigned long long internal_rescans = 0;   // scans repeated inside pm_scan_wait since pm_init (an internal buffer was too small)
  // pm_scan on hit-dense text: a range whose record lists would outgrow dense_bound records is scanned in pieces (scan_range)
  // instead of growing the lists; bound_on is set while pm_scan drives the scan (direct pm_scan_candidates calls keep growing)
  bool bound_on = false, too_dense = false, dense_mode = false;
  int64_t piece_len = 0;                     // pm_scan scans in pieces of at most this many positions (0: whole ranges)
  unsigned long long last_peak = 0;          // longest record list of the last scan
  unsigned long long range_splits = 0;       // times pm_scan halved its piece length since pm_init
  unsigned long long lookaheads = 0;         // scans pm_scan enqueued for the range it expected next, since pm_init
  ScanGeometry geo{};

  // host stage state
  std::vector<pm_hit> carry;          // filter_bitvec: candidates whose cluster is not complete yet
  std::vector<int64_t> lasthit;       // exact_halves: last kept end per pattern (exact_halves.cc:163)
  // pm_scan: the final hits of the ranges scanned so far, in (end, pid, k) order, in pinned host memory; handed out
  // by pm_scan (copied) or pm_scan_view (as a span) from land_pos on
  pm_hit *land = nullptr;
  size_t land_cap = 0, land_n = 0, land_pos = 0;
  hipStream_t copy_stream = nullptr;  // copies out of HBM that run beside the next range's scan (non-blocking stream)
  hipEvent_t ev_fin = nullptr;        // "the finalize stage of this range is done" on the handle's stream
  pm_hit *d_fsorted = nullptr;        // final hits after the device sort
  size_t fsorted_cap = 0;
  bool sort_dev = false;              // (end, pid, k) order by one keys-only radix sort on the device (device_sort_plan)
  int sort_idxbits = 0, sort_keybits = 0;
  bool spec = false;                  // pm_scan has the scan of the range it expects next in flight: (spec_b, spec_e]
  int64_t spec_b = 0, spec_e = 0;
  int64_t next_begin = 0;
  AlignScratch scratch;
  // window staging (verify stage)
  std::vector<uint8_t> winbuf;
  int64_t *d_wstart = nullptr; int32_t *d_wlen = nullptr; int64_t *d_woff = nullptr; uint8_t *d_wout = nullptr;
  size_t d_wcap = 0, d_woutcap = 0;

  // device finalize workspace (pm_finalize_device)
  uint64_t *d_keys = nullptr, *d_keys_alt = nullptr;
  void *d_ctemp = nullptr;
  size_t ckeys_cap = 0, ctemp_bytes = 0;
  pm_hit *d_fout = nullptr, *d_fleft = nullptr;
  const pm_hit *d_final = nullptr;    // final hits left in HBM by a finalize call with out == NULL
  size_t n_final = 0;
  float pack_ms = 0.f;                // duration of the last 2-bit re-encoding of the stream (ensure_packed)
  unsigned long long *d_fcounts = nullptr, *h_fcounts = nullptr;
  uint8_t *d_fpat_len = nullptr;
  uint32_t *d_fpat_id = nullptr;
  // exact_halves rule on the device: payload arrays and the pair sort's workspace
  uint32_t *d_packed = nullptr;       // the stream at 2 bits per base (seed family's first stage), rebuilt by every pm_init
  size_t packed_cap = 0;
  pm_hit *d_carry = nullptr;          // carried candidates of an earlier range, uploaded for the device clustering
  size_t d_carry_cap = 0;
  uint32_t *d_vals = nullptr, *d_vals_alt = nullptr;
  void *d_htemp = nullptr;
  size_t vals_cap = 0, htemp_bytes = 0;
  size_t nlong = 0;                   // patterns of 33..64 characters on the pair plan (pm_config.long_patterns); 0: no pattern beyond 32 on the seed family
  size_t nlong_edits = 0;             // patterns of 33..64 characters on the edit plan under -k 1 / -k 2 (PM_LONG_EDITS bit of pm_config.long_patterns): wide tiles of pm_edits_verify_wide, rows of 64 for pm_cluster_dp<64>
  size_t nlong_halves = 0;            // patterns of 33..64 characters on the halves plan under exact_halves -k 1 / -k 2 (PM_LONG_HALVES bit of pm_config.long_patterns): wide tiles of pm_half_scan<true> + pm_half_verify_wide, rows of 32 for pm_seed_extend<32>
  size_t nlong_exact = 0;             // patterns of 33..64 characters on the Bloom plan at k = 0 (PM_LONG_EXACT bit of pm_config.long_patterns): wide tiles of pm_seed_scan
  std::vector<uint8_t> in_rest;       // per inner pattern: 1 = scanned by the bit-parallel residue engine beside the seed family
  size_t nrest = 0;
  // edit-distance plan, patterns of 16..19 characters: a class of their own beside the 20..32 character main class and the
  // residue (pm_short.hip).  Its device state lives here, not in sd_more: the main class keeps its one-tile plans.
  std::vector<uint8_t> in_short;      // per inner pattern: 1 = scanned by pm_short_edit_scan
  size_t nshort = 0;
  bool short_only = false;            // no main class: the short engine is the handle's whole device stage
  ShortDevice shd;
  // -K 1 / -K 2, patterns of 16..19 characters: a class of their own on pm_short_sub_scan beside a main class on the pair
  // plan.  Both classes write the same records into d_cands; the host's edge records cover both.
  std::vector<uint8_t> in_ssub;       // per pattern: 1 = scanned by pm_short_sub_scan
  size_t nssub = 0;
  ShortSubDevice ssd;
  // -w, k = 0 / -K 1 / -K 2: primers of 16..32 (with PM_WILD_LONG: 16..64) characters with more than 16 concrete variants, a class of their own on
  // pm_wild_sub_scan (PM_WILD_CLASS bit of pm_config.long_patterns) beside the main class -- Bloom or pair
  // plan -- or without one.  Its records are the main class's; the host's edge records cover it (in_main_class).
  std::vector<uint8_t> in_wild;       // per inner pattern: 1 = scanned by pm_wild_sub_scan
  size_t nwild = 0;
  size_t nwild_long = 0;              // of them: primers of 33..64 characters (PM_WILD_LONG): the class's verify is pm_wild_sub_verify_wide
  bool wild_only = false;             // no main class: the wild class (and a residue, if any) is the handle's whole device stage
  WildDevice wd;
  bool halves_fresh = true;           // no host-side exact_halves state (lasthit, carried seeds) since init / pm_reset

  // windowed stream (pm_init_windowed): d_text / d_packed point at the bound slot, rebased so that absolute stream
  // positions index it; the scan and finalize kernels need no change
  int64_t win = 0;                    // window bytes (0: the whole stream is resident)
  int64_t win_back = 0, win_fwd = 0;  // halo of the device stages (stream_halo)
  int64_t win_guard = 0;              // guard margin of every slot, each side
  WinSlot slot[2];
  int bound = -1;
  hipStream_t up_stream = nullptr;    // packing of uploaded windows
  uint8_t *stage[WIN_UP_THREADS][2] = {};
  hipStream_t stage_st[WIN_UP_THREADS] = {};
  hipEvent_t stage_ev[WIN_UP_THREADS][2] = {};
  hipEvent_t stage_done[WIN_UP_THREADS] = {};
  int64_t win_held = 0, win_peak = 0, win_uploaded = 0, win_loads = 0;

  // counts (pm_count_scan / pm_counts) and the device re-alignment (pm_align_hits_device): DESIGN.md 5d
  AlignDevice ad;                     // tables of pm_align.hip, built on first use after an init (ensure_align_tables)
  bool ad_ready = false, ad_any_long = false;   // ad_any_long: some pattern is beyond the device limit of the DP
  bool ad_any_wide = false;           // PM_LONG_ALIGN: some pattern of 33..64 characters is re-aligned by pm_align_hits_wide_kernel (indels, 1 <= k <= AL_MAXK)
  void *ad_mem[8] = {};
  int scan_mode = 0;                  // since pm_reset: 0 nothing scanned, 1 pm_scan / pm_scan_view, 2 pm_count_scan, 3 pm_pcr_scan
  bool counting = false;              // a pm_count_scan is in its scan_range and the finals stay on the device
  uint64_t cnt_max = 0;               // its max_count
  bool cnt_dev = false;               // the tallies live on the device (else: cnt_host)
  uint64_t *d_ck = nullptr, *d_ck_alt = nullptr, *d_ck_scan = nullptr;   // tally keys + the tally's two workspaces
  size_t ck_cap = 0, cnt_fed = 0;     // cnt_fed: upper bound of the records the range's feed kernel looked at
  void *d_cktemp = nullptr;
  size_t cktemp_bytes = 0, cktemp_for = 0;
  unsigned long long *d_cnt = nullptr, *d_cinfo = nullptr, *d_actr = nullptr, *h_actr = nullptr;   // tallies [npat * (k + 1)], info [4], kernel counters [3], [4] with ad_any_wide (+ pinned copy)
  size_t cnt_words = 0;
  pm_hit *d_hostq = nullptr;          // records the feed kernel leaves to the host (patterns beyond the device limit)
  size_t hostq_cap = 0;
  uint64_t *d_hostq_idx = nullptr;    // ad_any_wide: the indices of d_hostq's records, which the wide kernel reads, and
  pm_hit *d_hostq2 = nullptr;         // the records that kernel leaves to the host in its turn; both hostq_cap long
  pm_hit *d_extra = nullptr;          // the range's host-decided hits, uploaded for the same kernel
  size_t d_extra_cap = 0;
  std::vector<uint64_t> cnt_host;     // host tally (k > 3 or 2^22 patterns and more)
  pm_count_info cinfo{};              // the host's share of pm_counts' info
  bool cnt_has_bogus = false;

  // pcr_match's pairing stage (pm_pcr_setup .. pm_pcr_pair): DESIGN.md 5e
  bool pcr_on = false;                // pm_pcr_setup was called since init
  PcrDevice pcr;
  void *pcr_mem[4] = {};              // patlen, size_lb, size_ub, entry_starts
  uint32_t pcr_nmask[8] = {};         // bit c: stream code c decodes to N or n
  pm_hit *d_held = nullptr;           // the held hits; pm_pcr_scan appends behind held_n
  size_t held_cap = 0, held_n = 0;
  bool pcr_scanning = false;          // a pm_pcr_scan is in its scan_range and the finals stay on the device
  size_t pcr_fed = 0;                 // upper bound of the records the range's finalize stage left behind held_n
  void *d_pcr_a = nullptr, *d_pcr_b = nullptr, *d_pcr_c = nullptr;   // a round's workspaces by held hits / by candidate pairs / by survivors
  size_t pcr_a_bytes = 0, pcr_b_bytes = 0, pcr_c_bytes = 0;
  void *pcr_out = nullptr;            // pinned: survivor records, then their strings
  size_t pcr_out_bytes = 0;
  unsigned long long *pcr_h_tot = nullptr;   // pinned: totals of a round's scans
  uint64_t pcr_stat[6] = {};

  std::string err;
};

// per-tile record counts between a scan's first-stage and verify kernels: [0] unused, [1 + t] tile t, then 8 measurement counters
// [SHORT_COUNT_AT]: seed records of the short class (all its tiles); the pair plan's short class counts its suspects there
// [WILD_COUNT_AT]: suspects of the wild class
// [EPAIR_COUNT_AT + t]: suspects of tile t between pm_pair_edit_scan and pm_pair_edit_resolve (the edit plan on the pair geometry);
// a word per tile, zeroed with the others in front of the tile loop, so every tile counts from zero in stream order
constexpr size_t SEEDCOUNT_WORDS = 1 + 256 + 8 + 2 + 256;
constexpr size_t EPAIR_COUNT_AT = 1 + 256 + 8 + 2;
constexpr size_t SHORT_COUNT_AT = 1 + 256 + 8;
constexpr size_t WILD_COUNT_AT = 1 + 256 + 8 + 1;

static thread_local std::string g_create_error;

static int fail(pm_handle *h, int code, const std::string &msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return code;
}
static int hipfail(pm_handle *h, hipError_t e, const char *what) {
  return fail(h, PM_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(h, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hipfail((h), e_, #expr); } while (0)
#define PM_TRY(expr) do { const int rc_ = (expr); if (rc_) return rc_; } while (0)

// A device buffer whose contents need not survive is too small: discard it and allocate `bytes` (the caller's size rule).
// The old block goes first, so the peak of HBM in use does not rise.  `what` names the buffer in the error message.
template <class T> static int dev_regrow(pm_handle *h, T **p, size_t bytes, const char *what) {
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  const hipError_t e = hipMalloc((void **)p, bytes);
  return e == hipSuccess ? PM_OK : hipfail(h, e, (std::string("hipMalloc of ") + what).c_str());
}

// A small host table into a fresh device allocation of at least `minimum` bytes (an empty table still has a pointer).
static int dev_upload(pm_handle *h, void **dst, const void *src, size_t bytes, size_t minimum, const char *what) {
  hipError_t e = hipMalloc(dst, std::max(bytes, minimum));
  if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
  return e == hipSuccess ? PM_OK : hipfail(h, e, (std::string("upload of ") + what).c_str());
}
template <class D, class T> static int dev_upload(pm_handle *h, D **dst, const std::vector<T> &v, size_t minimum, const char *what) {
  return dev_upload(h, (void **)dst, v.data(), v.size() * sizeof(T), minimum, what);
}

// ---- bit-packed codes on the host (<db>.sqz: char_io.t:18-214) ---------------------------------
// Code c sits in bits [c*bits, (c+1)*bits) of the packed bytes, bit 0 being the MSB of byte 0.  Eight codes are exactly
// `bits` bytes, so both directions move eight codes through one 64-bit word with constant shifts.
namespace {

template <int BITS> void unpack8(const uint8_t *p, uint8_t *out) {
  uint64_t w = 0;
  for (int i = 0; i < BITS; ++i) w = (w << 8) | p[i];
  for (int j = 0; j < 8; ++j) out[j] = (uint8_t)((w >> (BITS * (7 - j))) & ((1u << BITS) - 1u));
}
template <int BITS> uint32_t pack8(const uint8_t *c, uint8_t *p) {
  uint64_t w = 0;
  uint32_t seen = 0;
  for (int j = 0; j < 8; ++j) { w = (w << BITS) | c[j]; seen |= c[j]; }
  for (int i = 0; i < BITS; ++i) p[i] = (uint8_t)(w >> (8 * (BITS - 1 - i)));
  return seen;
}
template <int BITS> void unpack_run(const uint8_t *p, int64_t groups, uint8_t *out) {
  for (int64_t g = 0; g < groups; ++g) unpack8<BITS>(p + g * BITS, out + 8 * g);
}
template <int BITS> uint32_t pack_run(const uint8_t *c, int64_t groups, uint8_t *p) {
  uint32_t seen = 0;
  for (int64_t g = 0; g < groups; ++g) seen |= pack8<BITS>(c + 8 * g, p + g * BITS);
  return seen;
}
// one code at any position: the two bytes that hold it (bits <= 8: a code spans at most two)
inline uint8_t code_at(const uint8_t *p, int64_t packed_bytes, int bits, int64_t c) {
  const int64_t bit = c * bits, b = bit >> 3;
  const uint32_t w = ((uint32_t)p[b] << 8) | (b + 1 < packed_bytes ? p[b + 1] : 0u);
  return (uint8_t)((w >> (16 - bits - (int)(bit & 7))) & ((1u << bits) - 1u));
}

}  // namespace

extern "C" int pm_unpack_codes(const uint8_t *packed, int64_t packed_bytes, int32_t bits, int64_t first, int64_t n, uint8_t *out) {
  if (bits < 1 || bits > 8 || first < 0 || n < 0 || packed_bytes < 0 || packed_bytes > ((int64_t)1 << 59)) return PM_E_INVALID;
  if (n == 0) return PM_OK;
  if (!packed || !out || first > packed_bytes * 8 / bits - n) return PM_E_INVALID;
  int64_t i = 0;
  for (; i < n && ((first + i) & 7); ++i) out[i] = code_at(packed, packed_bytes, bits, first + i);
  const int64_t groups = (n - i) / 8;
  const uint8_t *p = packed + (first + i) / 8 * bits;
  switch (bits) {
    case 1: unpack_run<1>(p, groups, out + i); break;
    case 2: unpack_run<2>(p, groups, out + i); break;
    case 3: unpack_run<3>(p, groups, out + i); break;
    case 4: unpack_run<4>(p, groups, out + i); break;
    case 5: unpack_run<5>(p, groups, out + i); break;
    case 6: unpack_run<6>(p, groups, out + i); break;
    case 7: unpack_run<7>(p, groups, out + i); break;
    case 8: unpack_run<8>(p, groups, out + i); break;
  }
  for (i += 8 * groups; i < n; ++i) out[i] = code_at(packed, packed_bytes, bits, first + i);
  return PM_OK;
}

extern "C" int pm_pack_codes(const uint8_t *codes, int64_t n, int32_t bits, uint8_t *out, int64_t out_bytes) {
  if (bits < 1 || bits > 8 || n < 0 || out_bytes < 0 || n > ((int64_t)1 << 59)) return PM_E_INVALID;
  const int64_t need = (n * bits + 7) / 8;
  if (out_bytes < need || (n > 0 && (!codes || !out))) return PM_E_INVALID;
  const int64_t groups = n / 8;
  uint32_t seen = 0;
  switch (bits) {
    case 1: seen = pack_run<1>(codes, groups, out); break;
    case 2: seen = pack_run<2>(codes, groups, out); break;
    case 3: seen = pack_run<3>(codes, groups, out); break;
    case 4: seen = pack_run<4>(codes, groups, out); break;
    case 5: seen = pack_run<5>(codes, groups, out); break;
    case 6: seen = pack_run<6>(codes, groups, out); break;
    case 7: seen = pack_run<7>(codes, groups, out); break;
    case 8: seen = pack_run<8>(codes, groups, out); break;
  }
  if (n > 8 * groups) {                                             // the last, partial group: fill bits are zero
    uint8_t last[8] = {0, 0, 0, 0, 0, 0, 0, 0}, bytes[8];
    for (int64_t i = 8 * groups; i < n; ++i) { last[i - 8 * groups] = codes[i]; seen |= codes[i]; }
    uint64_t w = 0;
    for (int j = 0; j < 8; ++j) w = (w << bits) | (last[j] & ((1u << bits) - 1u));
    for (int i = 0; i < bits; ++i) bytes[i] = (uint8_t)(w >> (8 * (bits - 1 - i)));
    memcpy(out + groups * bits, bytes, (size_t)(need - groups * bits));
  }
  if (out_bytes > need) memset(out + need, 0, (size_t)(out_bytes - need));
  return (seen >> bits) ? PM_E_INVALID : PM_OK;                     // a code that does not fit `bits` bits
}

// Where the host stage reads stream codes from: the caller's bytes (pm_init, pm_init_windowed, pm_init_host), the caller's
// packed bytes (pm_init_packed), or -- no host form: pm_init_device -- the resident text in HBM.
static bool has_host_form(const pm_handle *h) { return h->h_text || h->h_packed; }
static int host_codes(pm_handle *h, int64_t pos, int64_t len, uint8_t *dst) {
  if (len <= 0) return PM_OK;
  if (h->h_text) memcpy(dst, h->h_text + pos, (size_t)len);
  else if (h->h_packed) {
    if (pm_unpack_codes(h->h_packed, h->h_packed_bytes, h->pk_bits, pos, len, dst) != PM_OK) return fail(h, PM_E_INVALID, "packed stream: read outside the packed bytes");
  } else HIP_TRY(h, hipMemcpy(dst, h->d_text + pos, (size_t)len, hipMemcpyDeviceToHost));
  return PM_OK;
}

// ---- pick_pattern_index, automatic branch (reference select.cc:31-141, NOPRIMEGEN, -x 0) -----
extern "C" int pm_pick_semantics(int32_t alphabet_size, int32_t acgt_normalized, int32_t k, int32_t wildcards,
                                 int32_t npat, const int32_t *patlen, const int32_t *esb, const int32_t *eeb) {
  long min_exact = INT_MAX, at_least_half = 0, excess = 0, min_inexact = INT_MAX, min_len = INT_MAX;
  for (int i = 0; i < npat; ++i) {
    const int a = esb ? esb[i] : 0, b = eeb ? eeb[i] : 0;
    const int c = a >= b ? a : b;                                  // the larger exact block decides
    min_exact = std::min<long>(min_exact, c);
    excess += c - patlen[i] / 2;
    at_least_half += (c - patlen[i] / 2) >= 0;
    min_inexact = std::min<long>(min_inexact, patlen[i] - c);
    min_len = std::min<long>(min_len, patlen[i]);
  }
  min_inexact = std::min(min_inexact, min_len);
  if (k > 0 && k >= min_inexact) return PM_E_FATAL;                // select.cc:87-90
  int exact_engine;                                                // select.cc:101-115
  if (wildcards) exact_engine = 4;
  else if (alphabet_size < 255) exact_engine = acgt_normalized ? 2 : 3;
  else exact_engine = 3;
  if (k == 0) return exact_engine == 4 ? PM_SEM_SHIFT_AND : PM_SEM_KEYWORD_TREE;
  const bool long_enough = (min_len >= 12 && alphabet_size < 10) || (min_len >= 8 && alphabet_size >= 10);
  if (k == 1 && long_enough && (at_least_half <= 0 || excess <= 0)) return PM_SEM_EXACT_HALVES;   // :121-126
  if (min_exact >= 6) return PM_SEM_EXACT_BASES;                   // :131-133
  return PM_SEM_FILTER_BITVEC;                                     // :137-139
}

// The one place the library looks at its environment (see Knobs, pm_internal.h).
static void read_knobs(Knobs *k) {
  auto num = [](const char *name) -> long long { const char *v = getenv(name); return v && *v ? atoll(v) : 0; };
  auto is = [](const char *name, const char *val) { const char *v = getenv(name); return v && !strcmp(v, val); };
  *k = Knobs();
  k->seed_chunk = num("PM_SEED_CHUNK"); k->seed_group = (int)num("PM_SEED_GROUP"); k->seed_debug = (int)num("PM_SEED_DEBUG");
  k->seed_tile = (long)num("PM_SEED_TILE");
  if (const char *v = getenv("PM_PAIR")) k->pair = atoi(v);
  k->pair_row = (int)num("PM_PAIR_ROW");
  k->pair_map = is("PM_PAIR_MAP", "superchunk") ? PAIR_MAP_SUPERCHUNK : is("PM_PAIR_MAP", "xcd") ? PAIR_MAP_XCD : is("PM_PAIR_MAP", "xcd-superchunk") ? PAIR_MAP_XCD_SUPERCHUNK : -1;
  k->half_bloom = is("PM_HALF_SCAN", "bloom"); k->edit_bloom = is("PM_EDIT_SCAN", "bloom"); k->edit_hash = is("PM_EDIT_SCAN", "hash");
  k->edit_table_log = (int)num("PM_EDIT_TABLE_LOG");
  if (const char *v = getenv("PM_BITPAR_TP")) k->bitpar_tp = atoi(v) != 0;
  k->bitpar_seglen = num("PM_BITPAR_SEGLEN");
  k->dense_bound = num("PM_DENSE_BOUND");
  k->short_bitpar = is("PM_SHORT_SCAN", "bitpar"); k->short_tile = (long)num("PM_SHORT_TILE");
  k->short_sub_off = is("PM_SHORT_SUB", "off");
  k->long_sub_off = is("PM_LONG_SUB", "off");
  k->long_exact_off = is("PM_LONG_EXACT", "off");
  k->long_edits_off = is("PM_LONG_EDITS", "off");
  k->long_halves_off = is("PM_LONG_HALVES", "off");
  k->wild_off = is("PM_WILD_CLASS", "off");
  k->wild_long_off = is("PM_WILD_LONG", "off");
  k->edit_pair_off = is("PM_EDIT_PAIR", "off");
  k->debug = getenv("PM_DEBUG") != nullptr;
}

extern "C" int pm_prepare_device(int device) {
  if (hipSetDevice(device) != hipSuccess) return PM_E_HIP;
  return hipFree(nullptr) == hipSuccess ? PM_OK : PM_E_HIP;         // (forces the runtime's lazy initialisation)
}

extern "C" int pm_create(const pm_config *cfg, pm_handle **out) {
  if (!cfg || !out) return fail(nullptr, PM_E_INVALID, "pm_create: null argument");
  if (cfg->abi_version != PM_ABI_VERSION) return fail(nullptr, PM_E_INVALID, "pm_create: ABI version mismatch");
  if (cfg->k < 0) return fail(nullptr, PM_E_INVALID, "pm_create: negative k");
  pm_handle *h = new (std::nothrow) pm_handle();
  if (!h) return fail(nullptr, PM_E_NOMEM, "out of memory");
  h->cfg = *cfg;
  read_knobs(&h->knobs);
  h->alpha.set_raw();
  *out = h;
  return PM_OK;
}

extern "C" int pm_add_pattern(pm_handle *h, const char *pat, size_t len, uint64_t id, int32_t esb, int32_t eeb) {
  if (!h || !pat) return PM_E_INVALID;
  if (h->inited) return fail(h, PM_E_INVALID, "pm_add_pattern after pm_init");
  if (id == 0) id = h->pats.size() + 1;                            // pattern_match.h:92-94
  if (id > 0xffffffffull) return fail(h, PM_E_UNSUPPORTED, "pattern ids above 2^32-1");
  h->id2idx[(uint32_t)id] = (uint32_t)h->pats.size();
  h->pats.push_back(Pattern{std::string(pat, len), id, esb, eeb});
  return PM_OK;
}

static void drain_spec(pm_handle *h);
static int ensure_landing(pm_handle *h, size_t need_more);
static void device_sort_plan(pm_handle *h);
static void win_release(pm_handle *h);
static void count_free(pm_handle *h);
static int count_clear(pm_handle *h);
static int count_feed_device(pm_handle *h, const pm_hit *d_hits, const unsigned long long *d_count, size_t n_upper);
static int count_collect(pm_handle *h, size_t nfin, std::vector<pm_hit> &extra, size_t *n_out);
static void pcr_free(pm_handle *h);
static int pcr_land_device(pm_handle *h, const pm_hit *d_hits, size_t n_upper);
static int pcr_collect(pm_handle *h, size_t nfin, std::vector<pm_hit> &extra, size_t *n_out);

static void free_device(pm_handle *h) {
  drain_spec(h);
  win_release(h);
  count_free(h);
  pcr_free(h);
  if (h->land) (void)hipHostFree(h->land);
  h->land = nullptr; h->land_cap = h->land_n = h->land_pos = 0;
  if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
  if (h->ev_fin) (void)hipEventDestroy(h->ev_fin);
  h->copy_stream = nullptr; h->ev_fin = nullptr;
  if (h->d_fsorted) (void)hipFree(h->d_fsorted);
  h->d_fsorted = nullptr; h->fsorted_cap = 0;
  bitpar_free(&h->bp);
  short_free(&h->shd);
  short_sub_free(&h->ssd);
  wild_free(&h->wd);
  seed_free(&h->sd);
  for (SeedDevice &d : h->sd_more) seed_free(&d);
  h->sd_more.clear();
  for (PairDevice &d : h->pair) pair_free(&d);
  h->pair.clear();
  for (PairDevice &d : h->epair) pair_free(&d);
  h->epair.clear(); h->epair_on = false;
  if (h->d_cands) (void)hipFree(h->d_cands);
  { void *hx[] = {h->d_ext, h->d_half_codes, h->d_half_len, h->d_hesb, h->d_heeb, h->d_dp_codes, h->d_dp_esb, h->d_dp_eeb, h->d_seed_count, h->d_seeds, h->d_susp}; for (void *q : hx) if (q) (void)hipFree(q); }
  h->d_seed_count = nullptr; h->d_seeds = nullptr; h->d_susp = nullptr; h->susp_cap = 0;
  h->d_dp_codes = nullptr; h->d_dp_esb = h->d_dp_eeb = nullptr;
  h->d_ext = nullptr; h->d_half_codes = h->d_half_len = nullptr; h->d_hesb = h->d_heeb = nullptr;
  if (h->d_counter) (void)hipFree(h->d_counter);
  if (h->h_counter) (void)hipHostFree(h->h_counter);
  if (h->h_seed_count) (void)hipHostFree(h->h_seed_count);
  h->h_seed_count = nullptr;
  if (h->own_d_text && h->d_text) (void)hipFree((void *)h->d_text);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  if (h->d_wstart) (void)hipFree(h->d_wstart);
  if (h->d_wlen) (void)hipFree(h->d_wlen);
  if (h->d_woff) (void)hipFree(h->d_woff);
  if (h->d_wout) (void)hipFree(h->d_wout);
  void *fw[] = {h->d_keys, h->d_keys_alt, h->d_ctemp, h->d_fout, h->d_fleft, h->d_fcounts, h->d_fpat_len, h->d_fpat_id, h->d_vals, h->d_vals_alt, h->d_htemp, h->d_carry, h->d_packed};
  h->d_packed = nullptr; h->packed_cap = 0;
  h->d_vals = h->d_vals_alt = nullptr; h->d_htemp = nullptr; h->vals_cap = 0; h->htemp_bytes = 0; h->d_carry = nullptr; h->d_carry_cap = 0;
  for (void *q : fw) if (q) (void)hipFree(q);
  if (h->h_fcounts) (void)hipHostFree(h->h_fcounts);
  h->d_keys = h->d_keys_alt = nullptr; h->d_ctemp = nullptr; h->d_fout = h->d_fleft = nullptr; h->d_fcounts = nullptr;
  h->h_fcounts = nullptr; h->d_fpat_len = nullptr; h->d_fpat_id = nullptr; h->ckeys_cap = 0; h->ctemp_bytes = 0;
  h->d_cands = nullptr; h->d_counter = nullptr; h->h_counter = nullptr; h->d_text = nullptr;
  h->ev0 = h->ev1 = nullptr; h->d_wstart = nullptr; h->d_wlen = nullptr; h->d_woff = nullptr; h->d_wout = nullptr;
  h->d_wcap = h->d_woutcap = 0;
}

static int ensure_capacity(pm_handle *h, size_t cap, bool exact = false) {
  if (h->d_cands && (exact ? h->cap == cap : h->cap >= cap)) return PM_OK;
  PM_TRY(dev_regrow(h, &h->d_cands, cap * sizeof(pm_hit), "d_cands"));
  if (h->d_ext) { (void)hipFree(h->d_ext); h->d_ext = nullptr; }
  h->cap = cap;
  return PM_OK;
}

// Decide the reference engine to reproduce and derive the inner (device) pattern set from it.
static int resolve(pm_handle *h) {
  const int np = (int)h->pats.size();
  std::vector<int32_t> len(np), esb(np), eeb(np);
  for (int i = 0; i < np; ++i) { len[i] = (int)h->pats[i].s.size(); esb[i] = h->pats[i].esb; eeb[i] = h->pats[i].eeb; }
  const Alphabet &A = h->alpha;
  const bool acgt = A.nch['A'] == 0 && A.nch['C'] == 1 && A.nch['G'] == 2 && A.nch['T'] == 3;
  int sem = h->cfg.semantics;
  // the "edits >= inexact bases" check runs for every -N (select.cc:87-90)
  const int autosem = pm_pick_semantics(A.size, acgt, h->cfg.k, h->cfg.wildcards, np, len.data(), esb.data(), eeb.data());
  if (autosem == PM_E_FATAL)
    return fail(h, PM_E_FATAL, "Fatal error: Number of edits >= Minimum number of inexact bases");
  if (sem == PM_SEM_AUTO) sem = autosem;
  switch (sem) {
    case 1: case 2: case 3: sem = PM_SEM_KEYWORD_TREE; break;
    case 4: break;
    case 5: break;
    case 7: case 8: case 9: case 10: sem = PM_SEM_EXACT_BASES; break;
    case 11: case 12: case 13: case 14: sem = PM_SEM_EXACT_HALVES; break;
    case PM_SEM_SHIFT_AND_INEXACT: break;
    default: return fail(h, PM_E_INVALID, "unknown semantics selector");
  }
  h->sem = sem;
  h->inner.clear(); h->inner_ids.clear();
  h->scan_k = 0; h->scan_indels = false;
  switch (sem) {
    case PM_SEM_KEYWORD_TREE: case PM_SEM_SHIFT_AND:
      for (const Pattern &p : h->pats) { h->inner.push_back(p); h->inner_ids.push_back((uint32_t)p.id); }
      break;
    case PM_SEM_SHIFT_AND_INEXACT:
      for (const Pattern &p : h->pats) { h->inner.push_back(p); h->inner_ids.push_back((uint32_t)p.id); }
      h->scan_k = h->cfg.k; h->scan_indels = h->cfg.indels != 0;
      break;
    case PM_SEM_FILTER_BITVEC:                                      // filter_bitvec.cc:185-196
      for (int i = 0; i < np; ++i) { h->inner.push_back(h->pats[i]); h->inner_ids.push_back((uint32_t)(i + 1)); }
      h->scan_k = h->cfg.k; h->scan_indels = h->cfg.indels != 0;
      break;
    case PM_SEM_EXACT_HALVES:                                       // exact_halves.cc:199-224
      for (int i = 0; i < np; ++i) {
        const std::string &s = h->pats[i].s;
        const size_t l1 = s.size() / 2;
        if (l1 == 0) return fail(h, PM_E_UNSUPPORTED, "exact_halves needs patterns of length >= 2");
        h->inner.push_back(Pattern{s.substr(0, l1), 0, 0, 0}); h->inner_ids.push_back((uint32_t)(2 * i + 1));
        h->inner.push_back(Pattern{s.substr(l1), 0, 0, 0});    h->inner_ids.push_back((uint32_t)(2 * i + 2));
      }
      h->lasthit.assign(np + 1, 0);
      h->halves_fresh = true;
      break;
    case PM_SEM_EXACT_BASES:                                        // exact_bases.cc:131-160
      for (int i = 0; i < np; ++i) {
        const Pattern &p = h->pats[i];
        const int L = (int)p.s.size();
        const int cut = p.esb >= p.eeb ? p.esb : p.eeb;
        if (cut <= 0 || cut > L) return fail(h, PM_E_UNSUPPORTED, "exact_bases needs 0 < exact bases <= pattern length");
        h->inner.push_back(Pattern{p.esb >= p.eeb ? p.s.substr(0, p.esb) : p.s.substr(L - p.eeb), 0, 0, 0});
        h->inner_ids.push_back((uint32_t)(i + 1));
      }
      break;
  }
  h->kern = h->cfg.kernel;
  return PM_OK;
}

// -w / -W on the seed family.  The seed kernels compare A,C,G,T exactly, so an ambiguity letter of a
// primer is expanded at table build: the primer becomes its concrete variants (same id), and the
// smallest distance over the variants is the wildcard distance (shift_and.cc:108-117: a pattern
// character accepts every stream letter of its IUPAC compatibility set).  That is only the whole story
// while the STREAM holds nothing but A,C,G,T (and N without -W): a stream letter R would match a
// primer's A under -w.
static std::string acgt_of(unsigned char ch) {                      // the A,C,G,T a pattern character accepts under -w
  std::string r;
  const char *set = iupac_compatible_set(ch);
  if (!set) return r;
  for (const char *q = set; *q; ++q) if (*q == 'A' || *q == 'C' || *q == 'G' || *q == 'T') r.push_back(*q);
  return r;
}
static bool stream_letters_plain(const pm_handle *h) {
  for (int c = 0; c < h->alpha.size && c < 256; ++c) {
    if (!h->alpha.present[c] || c == h->eos_code) continue;
    const unsigned char l = h->alpha.ch[c];
    if (l == 'A' || l == 'C' || l == 'G' || l == 'T') continue;
    if (l == 'N' && !h->cfg.text_n) continue;                       // a text N matches nothing without -W
    return false;
  }
  return true;
}
// The one letter pair on which the reference's automaton and its verify DP disagree: pattern N at a stream N under -w
// without -W.  The mask build leaves the stream's N out of every class (shift_and.cc:112: `wccompat[j]!='N' || _textn`),
// so the automaton counts a substitution there; the DP looks for EQUAL characters first (pattern_alignment.cc:314-316)
// and charges nothing.  filter_bitvec's hit value is the DP's, so for such a pattern it cannot be read off the
// candidate levels (found by tests/test_gpu_adversarial.py against the oracle; both kernel families shared the shortcut).
static bool stream_has_N(const pm_handle *h) {
  const int c = h->alpha.nch[(unsigned char)'N'];
  return c >= 0 && c < 256 && h->alpha.present[c];
}
static bool pattern_n_quirk(const pm_handle *h, const Pattern &p) {
  return h->cfg.wildcards && !h->cfg.text_n && p.s.find('N') != std::string::npos && stream_has_N(h);
}
// concrete variants of a primer (at most `cap`; empty + false when there would be more)
static bool expand_iupac(const std::string &p, size_t cap, std::vector<std::string> *out) {
  out->assign(1, std::string());
  for (unsigned char ch : p) {
    const std::string alts = acgt_of(ch);
    if (alts.empty()) { out->clear(); return true; }                // accepts no base at all: the primer cannot match
    if (out->size() * alts.size() > cap) { out->clear(); return false; }
    std::vector<std::string> next;
    next.reserve(out->size() * alts.size());
    for (const std::string &pre : *out) for (char a : alts) next.push_back(pre + a);
    out->swap(next);
  }
  return true;
}

// Inner pattern set of the seed family: Hamming candidates of the WHOLE patterns; the wrappers'
// rules are then applied to (end, pattern, distance, clean-half flags) records on the host.
static bool seed_eligible(pm_handle *h, std::string *why) {
  const int sem = h->sem;
  if (h->cfg.wildcards && !h->wild_seed) { *why = "IUPAC wildcards run on the bit-parallel family (the seed family takes them on A,C,G,T streams for the exact engines and filter_bitvec)"; return false; }
  if (h->cfg.k > 0 && h->cfg.indels && sem == PM_SEM_EXACT_HALVES) {
    // exact_halves with edits: exact seeds of the halves + partner prefilter on the GPU, DP on the host
    if (h->cfg.k > 2) { *why = "exact_halves -k > 2 runs on the bit-parallel family"; return false; }
    for (const Pattern &p : h->pats) if (p.s.size() > (h->nlong_halves ? 64u : 32u) || p.s.size() < 16) { *why = "exact_halves -k on the seed family needs 16..32 character patterns"; return false; }
    return true;
  }
  if (h->cfg.k > 0 && h->cfg.indels && (sem == PM_SEM_FILTER_BITVEC || sem == PM_SEM_SHIFT_AND_INEXACT)) {
    // the automaton's candidates from displaced-piece seeds + a per-seed automaton run (pm_seed.hip, EDITS)
    if (h->cfg.k > 2) { *why = "edit distance > 2 runs on the bit-parallel family"; return false; }
    for (size_t i = 0; i < h->pats.size(); ++i) {
      if (i < h->in_rest.size() && h->in_rest[i]) continue;         // goes to the bit-parallel residue
      if (i < h->in_short.size() && h->in_short[i]) continue;       // 16..19 characters: pm_short_edit_scan
      const Pattern &p = h->pats[i];
      if (p.s.size() > (h->nlong_edits ? 64u : 32u) || p.s.size() < 20) { *why = "the edit-distance seed plan needs 16..32 character patterns"; return false; }
    }
    for (uint32_t id : h->inner_ids) if (id >= (1u << 22)) { *why = "the edit-distance seed plan packs pattern ids into 22 bits"; return false; }
    if (sem == PM_SEM_SHIFT_AND_INEXACT) {
      // its records carry the pattern's id and the dedup keeps one per (id, end); the automaton reports every pattern on its
      // own (shift_and_inexact.cc:316-335), so two patterns under one id that end at the same character are two hits
      std::vector<uint32_t> ids(h->inner_ids);
      std::sort(ids.begin(), ids.end());
      if (std::adjacent_find(ids.begin(), ids.end()) != ids.end()) { *why = "patterns that share an id: the edit-distance seed plan keeps one record per (id, end)"; return false; }
    }
    return true;
  }
  if (h->cfg.k > 0 && h->cfg.indels && sem == PM_SEM_EXACT_BASES) {
    // every exact_bases hit is a window within k edits of the whole pattern: the edit-distance seed plan
    // finds those, pm_bases_seeds turns them into the reference's block seeds (pm_cluster.hip)
    if (h->cfg.k > 2) { *why = "edit distance > 2 runs on the bit-parallel family"; return false; }
    if (h->pats.size() >= ((size_t)1 << 22)) { *why = "the edit-distance seed plan packs pattern ids into 22 bits"; return false; }
    for (const Pattern &p : h->pats) {
      if (p.s.size() > 32 || p.s.size() < 20) { *why = "the edit-distance seed plan needs 20..32 character patterns"; return false; }
      for (unsigned char ch : p.s) if (!(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T')) { *why = "pattern with characters other than A,C,G,T"; return false; }
    }
    return true;
  }
  if (h->cfg.k > 0 && h->cfg.indels && sem != PM_SEM_KEYWORD_TREE && sem != PM_SEM_SHIFT_AND) { *why = "edit-distance search (-k) runs on the bit-parallel family"; return false; }
  // substitution-only search of 20..32 character A,C,G,T patterns with k = 1, 2 runs on the pair plan
  // (pm_pair.hip; 20..64 where the long route applies, long_route_allowed), whose exact verify knows the patterns' exact zones: a substitution there fails
  // the reference's constrained verifies (pattern_alignment.cc:320-323, primer_alignment.cc:155)
  bool pair_ok = !h->cfg.indels && (h->cfg.k == 1 || h->cfg.k == 2) && !h->pats.empty();
  for (size_t i = 0; i < h->pats.size(); ++i) {
    const Pattern &p = h->pats[i];
    if (i < h->in_wild.size() && h->in_wild[i]) continue;           // the wild class: its own exact stage (wild_verify) knows the zones
    const bool sub = i < h->in_ssub.size() && h->in_ssub[i];        // 16..19 characters beside the pair plan: pm_short_sub_scan, the same exact verify
    pair_ok = pair_ok && p.s.size() >= (sub ? 16u : 20u) && p.s.size() <= (h->nlong ? 64u : 32u);
    for (unsigned char ch : p.s) pair_ok = pair_ok && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
  }
  if (h->knobs.pair >= 0) pair_ok = pair_ok && h->knobs.pair != 0;
  if (sem == PM_SEM_EXACT_BASES && !pair_ok) { *why = "exact_bases runs on the bit-parallel family (the seed family takes it for -K 1 / -K 2 on 20..32 character patterns)"; return false; }
  if ((sem == PM_SEM_FILTER_BITVEC || sem == PM_SEM_EXACT_HALVES) && !pair_ok)
    for (const Pattern &p : h->pats) if (p.esb || p.eeb) { *why = "exact-base constraints need the text-based verify of the bit-parallel family"; return false; }
  return true;
}

// the stream is one the pair plan takes
static bool stream_for_pair_plan(const pm_handle *h) {
  const Alphabet &A = h->alpha;
  const bool norm = A.nch['A'] == 0 && A.nch['C'] == 1 && A.nch['G'] == 2 && A.nch['T'] == 3;
  const bool ascii = A.size == 256 && A.nch['A'] == 'A' && A.nch['C'] == 'C' && A.nch['G'] == 'G' && A.nch['T'] == 'T';
  return norm || ascii;                                             // (what pair_build asks of the stream)
}

// -K 1 / -K 2 with primers of 33..64 characters: the caller allows them on the pair plan
// (pm_config.long_patterns) and the option set is one whose records the plan's exact stage makes -- substitutions only,
// k = 1 or 2, filter_bitvec, bare shift_and_inexact or exact_halves, no kernel asked for by name, a stream the pair plan
// takes.  Anything else, PM_LONG_SUB=off included, leaves every handle as it was built before the route existed.
// Called with wild_seed decided.
static bool long_route_allowed(const pm_handle *h) {
  if (!(h->cfg.long_patterns & PM_LONG_SUB) || h->knobs.long_sub_off || h->knobs.pair == 0 || h->kern != PM_KERNEL_AUTO) return false;
  if (h->cfg.indels || (h->cfg.k != 1 && h->cfg.k != 2)) return false;
  if (h->sem != PM_SEM_FILTER_BITVEC && h->sem != PM_SEM_SHIFT_AND_INEXACT && h->sem != PM_SEM_EXACT_HALVES) return false;
  if (h->cfg.wildcards && !h->wild_seed) return false;
  return stream_for_pair_plan(h);
}

// k = 0 with primers of 33..64 characters: the caller allows them on the Bloom plan (the PM_LONG_EXACT
// bit of pm_config.long_patterns), the engine is one whose records verify_exact makes as they are -- keyword_tree or
// shift_and at k = 0 -- no kernel is asked for by name and the stream is one seed_build takes (the pair plan's
// condition).  Anything else, PM_LONG_EXACT=off included, leaves every handle as it was built before the route existed.
// Called with wild_seed decided.
static bool long_exact_allowed(const pm_handle *h) {
  if (!(h->cfg.long_patterns & PM_LONG_EXACT) || h->knobs.long_exact_off || h->kern != PM_KERNEL_AUTO) return false;
  if (h->cfg.k != 0 || (h->sem != PM_SEM_KEYWORD_TREE && h->sem != PM_SEM_SHIFT_AND)) return false;
  if (h->cfg.wildcards && !h->wild_seed) return false;
  return stream_for_pair_plan(h);
}

// -k 1 / -k 2 with primers of 33..64 characters: the caller allows them on the edit plan (the PM_LONG_EDITS
// bit of pm_config.long_patterns), the engine is one whose candidates are the automaton's -- filter_bitvec or bare
// shift_and_inexact with indels -- no kernel is asked for by name and the stream is one seed_build takes (the pair plan's
// condition).  Anything else, PM_LONG_EDITS=off included, leaves every handle as it was built before the route existed.
// Called with wild_seed decided.
static bool long_edits_allowed(const pm_handle *h) {
  if (!(h->cfg.long_patterns & PM_LONG_EDITS) || h->knobs.long_edits_off || h->kern != PM_KERNEL_AUTO) return false;
  if (!h->cfg.indels || (h->cfg.k != 1 && h->cfg.k != 2)) return false;
  if (h->sem != PM_SEM_FILTER_BITVEC && h->sem != PM_SEM_SHIFT_AND_INEXACT) return false;
  if (h->cfg.wildcards && !h->wild_seed) return false;
  return stream_for_pair_plan(h);
}

static size_t half_row(const pm_handle *h) { return h->nlong_halves ? 32 : 16; }   // codes per half in d_half_codes (pm_seed_extend<16> / <32>)
// exact_halves -k 1 / -k 2 with primers of 33..64 characters: the caller allows them on the halves plan (the
// PM_LONG_HALVES bit of pm_config.long_patterns), the engine is exact_halves -- selected or asked for -- with indels, no
// wildcards, no kernel is asked for by name and the stream is one seed_build takes (the pair plan's condition).  The list
// itself is looked at by init_common: exact_halves keeps no residue, so every pattern has to be one the plan takes.
// Anything else, PM_LONG_HALVES=off included, leaves every handle as it was built before the route existed.
static bool long_halves_allowed(const pm_handle *h) {
  if (!(h->cfg.long_patterns & PM_LONG_HALVES) || h->knobs.long_halves_off || h->kern != PM_KERNEL_AUTO) return false;
  if (!h->cfg.indels || (h->cfg.k != 1 && h->cfg.k != 2)) return false;
  if (h->sem != PM_SEM_EXACT_HALVES || h->cfg.wildcards) return false;
  return stream_for_pair_plan(h);
}

// -K 1 / -K 2 on a list of mixed lengths: the primers of 16..19 characters become a class of their own
// (in_ssub) when the list also holds a primer of 20..32 characters the pair plan takes and every other primer the seed
// family could take has 16..19.  Anything else -- a primer of 10..15 characters, no long or no short primer, more short
// primers than SHORT_SUB_MAX_PATTERNS, exact_bases, a kernel on request, -k, k = 0, PM_SHORT_SUB=off -- leaves the list on
// the route it had.  Called with in_rest decided.  maxL: the longest primer the main class takes, 32 or -- the long route,
// long_route_allowed -- 64; a primer of 33..64 characters then counts as one of the main class like one of 20..32.
static void short_sub_route(pm_handle *h, size_t maxL) {
  h->in_ssub.assign(h->pats.size(), 0);
  h->nssub = 0;
  if (h->knobs.short_sub_off || h->knobs.pair == 0 || h->cfg.indels || (h->cfg.k != 1 && h->cfg.k != 2) || h->kern != PM_KERNEL_AUTO) return;
  if (h->sem != PM_SEM_FILTER_BITVEC && h->sem != PM_SEM_SHIFT_AND_INEXACT && h->sem != PM_SEM_EXACT_HALVES) return;
  if (h->cfg.wildcards && !h->wild_seed) return;
  if (!stream_for_pair_plan(h)) return;
  size_t nmain = 0, nsub = 0;
  std::vector<uint8_t> sub(h->pats.size(), 0);
  std::vector<std::string> variants;
  for (size_t i = 0; i < h->pats.size(); ++i) {
    const Pattern &p = h->pats[i];
    const size_t L = p.s.size();
    bool ok = L >= 10 && L <= maxL;                                 // the main class's conditions (init_common)
    if (h->wild_seed) ok = ok && expand_iupac(p.s, 16, &variants) && !(h->sem == PM_SEM_FILTER_BITVEC && pattern_n_quirk(h, p));
    else for (unsigned char ch : p.s) ok = ok && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
    if (!ok) {
      if (h->sem == PM_SEM_EXACT_HALVES) return;                    // (no residue beside exact_halves)
      continue;                                                     // residue: the bit-parallel kernel, after both classes
    }
    if (L >= 20) ++nmain;
    else if (L >= 16) { sub[i] = 1; ++nsub; }
    else return;
  }
  if (!nmain || !nsub || nsub > SHORT_SUB_MAX_PATTERNS) return;     // (above the cap the key runs outgrow what the Bloom plan costs)
  h->in_ssub.swap(sub);
  h->nssub = nsub;
}

// -w primers with more than 16 concrete variants: with the PM_WILD_CLASS bit of pm_config.long_patterns
// they leave the residue for a class of their own on pm_wild_sub_scan.  The handle: no kernel asked for by name, wild_seed
// (a plain stream; keyword_tree, shift_and or filter_bitvec), substitutions only -- keyword_tree / shift_and scan at k = 0,
// filter_bitvec at -K 1 / -K 2 -- and a stream the pair plan takes.  The primer: refused by expand_iupac(p, 16), one
// wild_takes holds (16..32 characters, a base at every character, <= 256 keys per field pair), no pattern_n_quirk primer
// under filter_bitvec.  The class: wild_class_fits (run entries per field pair); a class beyond it leaves every primer where
// it was.  Anything else, PM_WILD_CLASS=off included, leaves every handle as it was built before the class existed.
// With the PM_WILD_LONG bit as well a primer of 33..64 characters joins under the same rules -- its keys are
// those of its last 16 characters -- whatever the main class's longest primer is (maxL of classify_patterns): such a primer
// is in the residue under either classification, for its length or for its variants.  PM_WILD_LONG=off keeps 32.
// Called by classify_patterns with in_rest decided.
static void wild_route(pm_handle *h) {
  if (!(h->cfg.long_patterns & PM_WILD_CLASS) || h->knobs.wild_off || h->kern != PM_KERNEL_AUTO || !h->wild_seed) return;
  if (h->sem == PM_SEM_FILTER_BITVEC ? (h->cfg.indels || (h->scan_k != 1 && h->scan_k != 2)) : h->scan_k != 0) return;
  if (!stream_for_pair_plan(h)) return;
  const size_t maxWL = (h->cfg.long_patterns & PM_WILD_LONG) && !h->knobs.wild_long_off ? 64 : 32;
  std::vector<std::string> variants, cls;
  std::vector<size_t> who;
  for (size_t i = 0; i < h->inner.size(); ++i) {
    const Pattern &p = h->inner[i];
    if (!h->in_rest[i] || !wild_takes(p.s, h->scan_k, maxWL)) continue;
    if (expand_iupac(p.s, 16, &variants)) continue;                 // (in the residue for another reason)
    if (h->sem == PM_SEM_FILTER_BITVEC && pattern_n_quirk(h, p)) continue;
    who.push_back(i); cls.push_back(p.s);
  }
  if (who.empty() || who.size() >= ((size_t)1 << 21) || !wild_class_fits(cls, h->scan_k)) return;
  for (size_t i : who) { h->in_rest[i] = 0; --h->nrest; h->in_wild[i] = 1; ++h->nwild; if (h->inner[i].s.size() > 32) ++h->nwild_long; }
}

// Which engine and class every pattern of the list goes to: in_rest (the bit-parallel residue beside the seed family),
// in_short (16..19 characters under -k: pm_short_edit_scan), short_only, and -- short_sub_route -- in_ssub.  A pattern set is
// rarely uniform: a few primers with an ambiguity letter, one that is too short or too long for the seed plan.  Where the
// engines' records mean the same (one inner pattern per pattern: keyword_tree, shift_and, shift_and_inexact,
// filter_bitvec) those few are scanned by the bit-parallel kernels into the same record buffer and the rest stays on the
// seed family.  maxL: the longest pattern the main class takes -- 32, or 64 where the long route applies (init_common
// classifies for 64 first and again for 32 when the long route does not hold for the list: every call starts afresh).
// Called with wild_seed decided.
static void classify_patterns(pm_handle *h, bool want_seed, size_t maxL) {
  const bool edits_plan = h->cfg.indels && h->cfg.k > 0 && (h->sem == PM_SEM_FILTER_BITVEC || h->sem == PM_SEM_SHIFT_AND_INEXACT);
  const bool short_class = edits_plan && h->cfg.k <= 2 && !h->knobs.short_bitpar;   // patterns of 16..19 characters: pm_short_edit_scan
  h->in_rest.assign(h->inner.size(), 0);
  h->nrest = 0;
  h->in_short.assign(h->inner.size(), 0);
  h->nshort = 0; h->short_only = false;
  h->in_wild.assign(h->inner.size(), 0);
  h->nwild = 0; h->nwild_long = 0; h->wild_only = false;
  if (want_seed && (!h->cfg.wildcards || h->wild_seed) && h->kern == PM_KERNEL_AUTO &&
      (h->sem == PM_SEM_KEYWORD_TREE || h->sem == PM_SEM_SHIFT_AND || h->sem == PM_SEM_SHIFT_AND_INEXACT || h->sem == PM_SEM_FILTER_BITVEC)) {
    std::vector<std::string> variants;
    for (size_t i = 0; i < h->inner.size(); ++i) {
      const std::string &ps = h->inner[i].s;
      const bool is_short = short_class && ps.size() >= 16 && ps.size() <= 19;   // otherwise under exactly the main class's conditions
      bool ok = (ps.size() <= maxL && ps.size() >= (edits_plan ? 20u : 10u)) || is_short;
      if (h->wild_seed) ok = ok && expand_iupac(ps, 16, &variants) &&   // up to two ambiguity letters (16 variants)
                         !(h->sem == PM_SEM_FILTER_BITVEC && pattern_n_quirk(h, h->inner[i]));   // (its value needs the text-based verify)
      else for (unsigned char ch : ps) ok = ok && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
      if (!ok) { h->in_rest[i] = 1; ++h->nrest; }
      else if (is_short) { h->in_short[i] = 1; ++h->nshort; }
    }
    wild_route(h);
    // nothing for the main class and something for the residue: one engine, the bit-parallel family
    // (a wild class stands without a main class: wild_only)
    if (!h->nwild && h->nrest && h->nrest + h->nshort == h->inner.size()) {
      std::fill(h->in_rest.begin(), h->in_rest.end(), 0); h->nrest = 0;
      std::fill(h->in_short.begin(), h->in_short.end(), 0); h->nshort = 0;
    }
  }
  else if (short_class && h->kern == PM_KERNEL_SEED && !h->cfg.wildcards) {
    // the seed family on request: no residue, but the two length classes of the edit plan
    for (size_t i = 0; i < h->inner.size(); ++i) {
      const std::string &ps = h->inner[i].s;
      bool ok = ps.size() >= 16 && ps.size() <= 19;
      for (unsigned char ch : ps) ok = ok && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
      if (ok) { h->in_short[i] = 1; ++h->nshort; }
    }
  }
  h->short_only = h->nshort != 0 && h->nshort == h->inner.size();
  h->wild_only = h->nwild != 0 && h->nwild + h->nrest == h->inner.size();
  short_sub_route(h, maxL);
}

static int init_common(pm_handle *h, const uint8_t *table, int32_t table_len) {
  drain_spec(h);
  h->land_n = h->land_pos = 0;
  if (table) {
    if (table_len <= 0 || table_len > 256) return fail(h, PM_E_INVALID, "bad alphabet table length");
    h->alpha.set_table(table, table_len);
  } else h->alpha.set_raw();
  // -w/-W on a raw stream: IUPAC classes name up to 16 letters each, the kernels keep 6 character
  // classes in registers -- only the letters that occur in the stream need one
  if (!table && h->cfg.wildcards) {
    if (h->host_only || h->win) {                                   // no device copy of the whole stream: look at the host bytes
      for (int i = 0; i < 256; ++i) h->alpha.present[i] = false;
      for (int64_t i = 0; i < h->n; ++i) h->alpha.present[h->h_text[i]] = true;
    } else HIP_TRY(h, stream_presence(h->d_text, h->n, h->alpha.present, h->stream));
  }
  h->eos_code = h->alpha.nch[(uint8_t)h->cfg.eos];                  // shift_and_inexact.cc:131
  int rc = resolve(h);
  if (rc) return rc;
  bitpar_free(&h->bp); seed_free(&h->sd); short_free(&h->shd); short_sub_free(&h->ssd); wild_free(&h->wd);
  for (SeedDevice &d : h->sd_more) seed_free(&d);
  h->sd_more.clear();
  for (PairDevice &d : h->pair) pair_free(&d);
  h->pair.clear();
  for (PairDevice &d : h->epair) pair_free(&d);
  h->epair.clear(); h->epair_on = false;
  // tables pm_finalize_device builds on first use depend on the alphabet mapping and the pattern
  // list of THIS init: drop the ones of an earlier init
  { void *lazy[] = {h->d_dp_codes, h->d_dp_esb, h->d_dp_eeb, h->d_fpat_len, h->d_fpat_id}; for (void *q : lazy) if (q) (void)hipFree(q); }
  h->d_dp_codes = nullptr; h->d_dp_esb = h->d_dp_eeb = nullptr; h->d_fpat_len = nullptr; h->d_fpat_id = nullptr;
  h->d_final = nullptr; h->n_final = 0;
  count_free(h);
  h->seed_flags = false; h->bases_flags = false; h->bases_edits = false; h->half_ranked_any = false;
  h->zoned = false;
  for (const Pattern &p : h->pats) h->zoned = h->zoned || p.esb || p.eeb;
  h->nn_quirk = false;
  for (const Pattern &p : h->pats) h->nn_quirk = h->nn_quirk || pattern_n_quirk(h, p);
  for (EdgeRecords &e : h->edge) e = EdgeRecords();
  std::string why;
  bool want_seed = h->kern == PM_KERNEL_SEED || h->kern == PM_KERNEL_AUTO;
  h->wild_seed = h->cfg.wildcards && want_seed && h->kern == PM_KERNEL_AUTO && stream_letters_plain(h) &&
                 (h->sem == PM_SEM_KEYWORD_TREE || h->sem == PM_SEM_SHIFT_AND || h->sem == PM_SEM_FILTER_BITVEC);
  h->nlong = 0; h->nlong_exact = 0; h->nlong_edits = 0; h->nlong_halves = 0;
  bool any_long = false;                                            // (a list without a primer of 33..64 is classified once, as without the flag)
  for (const Pattern &p : h->pats) any_long = any_long || (p.s.size() > 32 && p.s.size() <= 64);
  if (any_long && long_route_allowed(h)) {
    // The long primers join the main class only where the main class is the pair plan's: every primer that is neither
    // residue nor of the 16..19 class has 20..64 characters (exact_halves, which keeps no residue: and A,C,G,T only).
    // A list for which that does not hold -- and one without a primer of 33..64 -- is classified as without the route.
    classify_patterns(h, want_seed, 64);
    size_t nlong = 0;
    bool pair_takes = true;
    for (size_t i = 0; i < h->pats.size(); ++i) {
      const std::string &ps = h->pats[i].s;
      if (h->in_ssub[i] || (i < h->in_wild.size() && h->in_wild[i])) continue;
      if (h->sem == PM_SEM_EXACT_HALVES) { for (unsigned char ch : ps) pair_takes = pair_takes && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T'); pair_takes = pair_takes && ps.size() <= 64; }
      else if (i < h->in_rest.size() && h->in_rest[i]) continue;
      pair_takes = pair_takes && ps.size() >= 20;
      if (ps.size() > 32) ++nlong;
    }
    if (nlong && pair_takes) h->nlong = nlong;
  }
  else if (any_long && long_exact_allowed(h)) {
    // k = 0: a primer of 33..64 characters is a main-class primer under the rule of 10..32 (A,C,G,T only, or <= 16 concrete
    // variants under -w on a plain stream).  Kept only if the main class then holds such a primer; a list whose long primers
    // are all residue anyway is classified as without the route.
    classify_patterns(h, want_seed, 64);
    size_t nlong = 0;
    std::vector<std::string> variants;
    for (size_t i = 0; i < h->inner.size(); ++i) {
      const std::string &ps = h->inner[i].s;
      if (ps.size() <= 32 || ps.size() > 64 || (i < h->in_rest.size() && h->in_rest[i])) continue;
      bool ok = true;                                               // (classify_patterns clears in_rest when nothing is left for the main class)
      if (h->wild_seed) ok = expand_iupac(ps, 16, &variants);
      else for (unsigned char ch : ps) ok = ok && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
      if (ok) ++nlong;
    }
    h->nlong_exact = nlong;
  }
  else if (any_long && long_edits_allowed(h)) {
    // -k 1 / -k 2: a primer of 33..64 characters is a main-class primer under the rule of 20..32 (A,C,G,T only, or <= 16
    // concrete variants under -w on a plain stream).  Kept only if the main class then holds such a primer; a list whose
    // long primers are all residue anyway is classified as without the route.
    classify_patterns(h, want_seed, 64);
    size_t nlong = 0;
    std::vector<std::string> variants;
    for (size_t i = 0; i < h->inner.size(); ++i) {
      const std::string &ps = h->inner[i].s;
      if (ps.size() <= 32 || ps.size() > 64 || (i < h->in_rest.size() && h->in_rest[i])) continue;
      bool ok = true;                                               // (classify_patterns clears in_rest when nothing is left for the main class)
      if (h->wild_seed) ok = expand_iupac(ps, 16, &variants) && !(h->sem == PM_SEM_FILTER_BITVEC && pattern_n_quirk(h, h->inner[i]));
      else for (unsigned char ch : ps) ok = ok && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
      if (ok) ++nlong;
    }
    h->nlong_edits = nlong;
  }
  else if (any_long && long_halves_allowed(h)) {
    // exact_halves -k 1 / -k 2: one engine, no residue -- the list stays on the halves plan only as a whole: every primer
    // A,C,G,T and of 16..64 characters.  A 65-mer, a 15-mer or a primer with an N leaves it on the bit-parallel family.
    classify_patterns(h, want_seed, 64);
    size_t nlong = 0;
    bool takes = true;
    for (const Pattern &p : h->pats) {
      takes = takes && p.s.size() >= 16 && p.s.size() <= 64;
      for (unsigned char ch : p.s) takes = takes && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T');
      if (p.s.size() > 32) ++nlong;
    }
    if (takes) h->nlong_halves = nlong;
  }
  if (!h->nlong && !h->nlong_exact && !h->nlong_edits && !h->nlong_halves) classify_patterns(h, want_seed, 32);
  else if (h->knobs.debug) fprintf(stderr, "[pm] long route: %zu patterns of 33..64 characters on the %s plan\n", h->nlong + h->nlong_exact + h->nlong_edits + h->nlong_halves, h->nlong ? "pair" : h->nlong_edits ? "edit" : h->nlong_halves ? "halves" : "seed");
  if (want_seed && !seed_eligible(h, &why)) {
    if (h->kern == PM_KERNEL_SEED) return fail(h, PM_E_UNSUPPORTED, "seed engine: " + why);
    want_seed = false;
  }
  if (want_seed) {
    std::vector<Pattern> sp; std::vector<uint32_t> sid;
    int sk = h->scan_k;
    std::vector<std::string> partners;
    std::vector<uint8_t> sides;
    const bool halves_mode = h->sem == PM_SEM_EXACT_HALVES && h->cfg.indels && h->cfg.k > 0;
    const bool edits_mode = h->cfg.indels && h->cfg.k > 0 && (h->sem == PM_SEM_FILTER_BITVEC || h->sem == PM_SEM_SHIFT_AND_INEXACT || h->sem == PM_SEM_EXACT_BASES);
    if (halves_mode) {                            // halves as exact patterns (ids 2j+1, 2j+2), partner = other half
      sp = h->inner; sid = h->inner_ids; sk = 0;
      for (size_t i = 0; i + 1 < sp.size(); i += 2) {
        partners.push_back(sp[i + 1].s); sides.push_back(0);      // left half: partner to the right
        partners.push_back(sp[i].s); sides.push_back(1);          // right half: partner to the left
      }
    } else if (h->sem == PM_SEM_EXACT_HALVES) {   // -K: whole patterns, distance <= k, halves decided by flags
      for (size_t i = 0; i < h->pats.size(); ++i) if (!h->in_ssub[i]) { sp.push_back(h->pats[i]); sid.push_back((uint32_t)(i + 1)); }
      sk = h->cfg.k;
    } else if (h->sem == PM_SEM_EXACT_BASES) {
      // -K: an occurrence of the mandated exact block whose remainder verifies (exact_bases.cc:92-121, the
      // extension DP with indels off walks the diagonal) = a whole-pattern window within k substitutions,
      // none of them in an exact zone; one hit per occurrence, no clustering: the records are final
      // (-k: the records in between are the automaton's candidates of pattern i + 1, see pm_bases_seeds)
      for (size_t i = 0; i < h->pats.size(); ++i) { sp.push_back(h->pats[i]); sid.push_back(h->cfg.indels ? (uint32_t)(i + 1) : (uint32_t)h->pats[i].id); }
      sk = h->cfg.k;
    } else if (h->wild_seed) {                    // every concrete variant of a primer is a seed-family pattern with the primer's id
      std::vector<std::string> variants;
      for (size_t i = 0; i < h->inner.size(); ++i) {
        if (h->in_rest[i] || h->in_short[i] || h->in_ssub[i] || h->in_wild[i]) continue;
        expand_iupac(h->inner[i].s, 16, &variants);
        for (const std::string &v : variants) { Pattern q = h->inner[i]; q.s = v; sp.push_back(q); sid.push_back(h->inner_ids[i]); }
      }
      if (sp.empty() && !h->short_only && !h->wild_only) { sp.push_back(Pattern{std::string(edits_mode ? 20 : 10, 'A'), 0, 0, 0}); sid.push_back(0); why = "no primer the seed family could take"; }
    } else if (h->nrest || h->nshort || h->nssub) {
      for (size_t i = 0; i < h->inner.size(); ++i) if (!h->in_rest[i] && !h->in_short[i] && !h->in_ssub[i]) { sp.push_back(h->inner[i]); sid.push_back(h->inner_ids[i]); }
    } else { sp = h->inner; sid = h->inner_ids; }
    // the automata and the keyword tree know nothing of exact_start_bases / exact_end_bases (shift_and_inexact.cc:85-86
    // stores them and never looks): their records are every window within k, whatever zone a substitution falls in
    if (h->sem == PM_SEM_SHIFT_AND_INEXACT || h->sem == PM_SEM_SHIFT_AND || h->sem == PM_SEM_KEYWORD_TREE)
      for (Pattern &p : sp) { p.esb = 0; p.eeb = 0; }
    // One LDS Bloom filter (1 Mbit) stays selective up to ~256k keys: larger pattern sets are cut
    // into tiles with their own tables; the scan launches once per tile into the same record buffer.
    size_t tile_keys = 262144;
    // the plan (window, pieces) must be the same for every tile: it depends on the shortest pattern
    // of the whole set, so every tile is built with that window forced
    int force_lw = 0;
    for (const Pattern &p : sp) force_lw = force_lw == 0 ? (int)p.s.size() : std::min(force_lw, (int)p.s.size());
    // halves of <= 10 bases: the filter is the exact bitmap of their keys (SeedArgs::exact_filter) and
    // has no capacity to exceed -- one pass over the stream for all of them
    if (halves_mode && force_lw > 0 && force_lw <= 10) tile_keys = (size_t)1 << 21;
    // halves of >= 10 bases go through the ranked plan (pm_half_scan): its key bitmap has no capacity either, and a
    // tile of 2^20 halves keeps the "further halves of a key" index inside the slot's 20 bits
    if (halves_mode && force_lw >= 10 && !h->knobs.half_bloom) {
      size_t fits = 0;                                 // seed_build's rule: the ranked plan when >= 90 % of the halves fit its partner test
      for (size_t i = 0; i < sp.size(); ++i) {
        const int L = (int)sp[i].s.size(), plen = (int)partners[i].size();
        if (L + plen > 32) ++fits;                       // (a half of a pattern of 33..64 characters: its slot tests the half itself)
        else if (sides[i] ? L + plen + h->cfg.k <= 32 : plen + h->cfg.k <= 16) ++fits;
      }
      if (fits * 10 >= sp.size() * 9) tile_keys = (size_t)1 << 20;
    }
    if (h->knobs.seed_tile > 0) tile_keys = (size_t)h->knobs.seed_tile;
    const size_t ntile = sp.empty() ? 1 : (sp.size() + tile_keys - 1) / tile_keys;
    size_t per = (sp.size() + ntile - 1) / ntile;
    if (halves_mode) per += per & 1;                // keep (left, right) half pairs together: side = index parity
    // Substitution-only search with k = 1, 2 on patterns of 20..32 characters: the pair plan (exact
    // 20-bit key bitmaps, pm_pair.hip) replaces the Bloom-filter plan of pm_seed.hip
    bool use_pair = !halves_mode && !edits_mode && (sk == 1 || sk == 2) && !sp.empty() && force_lw >= 20;
    if (h->knobs.pair >= 0) use_pair = use_pair && h->knobs.pair != 0;
    for (size_t ti = 0; ti < ntile && why.empty() && use_pair; ++ti) {
      const size_t lo = ti * per, hi = std::min(sp.size(), lo + per);
      std::vector<Pattern> tp(sp.begin() + lo, sp.begin() + hi);
      std::vector<uint32_t> tid(sid.begin() + lo, sid.begin() + hi);
      PairTables pt;
      const std::string msg = pair_build(tp, tid, h->alpha, sk, h->eos_code, &pt, h->knobs.pair_row, 3, h->nlong ? PAIR_MAX_LEN_WIDE : PAIR_MAX_LEN,
                                         (h->knobs.seed_debug & 64) != 0);
      // With long primers in the main class (h->nlong) the plan cannot refuse: long_route_allowed has checked k and the
      // stream, the classification has left the main class A,C,G,T patterns (variants under -w) of 20..64 characters, and
      // a tile holds at most 2^21 of them.  The seed plan below could not take such a list, so a refusal is an error here,
      // not a change of route.
      if (!msg.empty() && h->nlong) return fail(h, PM_E_UNSUPPORTED, "pair plan (long route): " + msg);
      if (!msg.empty()) {                                            // not for this set: the seed plan below takes it
        for (PairDevice &d : h->pair) pair_free(&d);
        h->pair.clear();
        use_pair = false;
        break;
      }
      h->pair.emplace_back();
      HIP_TRY(h, pair_upload(pt, &h->pair.back(), h->stream));
      h->pair.back().knobs = h->knobs;
      h->pair.back().viol_level = h->sem == PM_SEM_FILTER_BITVEC ? 3 : 0;   // filter_bitvec chains every candidate; the others drop zone violations
      // the plan facts the rest of this file reads from h->sd (no device tables behind them)
      h->sd.k = sk; h->sd.Lw = 20; h->sd.pb = 5; h->sd.r = 4 - sk; h->sd.ncombos = pt.ncombos; h->sd.ascii = pt.ascii;
      h->sd.maxlen = std::max(h->sd.maxlen, pt.maxlen);
    }
    for (size_t ti = 0; ti < ntile && why.empty() && !use_pair && !h->short_only && !h->wild_only; ++ti) {
      const size_t lo = ti * per, hi = std::min(sp.size(), lo + per);
      std::vector<Pattern> tp(sp.begin() + lo, sp.begin() + hi);
      std::vector<uint32_t> tid(sid.begin() + lo, sid.begin() + hi);
      std::vector<std::string> tpart;
      std::vector<uint8_t> tside;
      if (halves_mode) { tpart.assign(partners.begin() + lo, partners.begin() + hi); tside.assign(sides.begin() + lo, sides.begin() + hi); }
      SeedTables st;
      why = seed_build(tp, tid, h->alpha, sk, h->eos_code, &st, force_lw, halves_mode ? &tpart : nullptr,
                       halves_mode ? &tside : nullptr, h->cfg.k, edits_mode, h->knobs, h->nlong_exact || h->nlong_edits || h->nlong_halves ? SEED_MAX_LEN_WIDE : SEED_MAX_LEN);
      if (why.empty() && h->kern == PM_KERNEL_AUTO && st.Lw < (halves_mode ? 8 : 10)) why = "patterns too short for the seed family";
      if (!why.empty()) break;
      SeedDevice *dst = &h->sd;
      if (ti > 0) { h->sd_more.emplace_back(); dst = &h->sd_more.back(); }
      HIP_TRY(h, seed_upload(st, dst, h->stream));
      dst->knobs = h->knobs;
      dst->maxlen = std::max(dst->maxlen, h->sd.maxlen);
    }
    if (why.empty() && h->nshort) {                                 // the short class beside (or instead of) the main class
      std::vector<Pattern> shp; std::vector<uint32_t> shid;
      std::vector<std::string> variants;
      for (size_t i = 0; i < h->inner.size(); ++i) {
        if (!h->in_short[i]) continue;
        if (h->wild_seed) {                                           // as in the main class: every concrete variant with the primer's id
          expand_iupac(h->inner[i].s, 16, &variants);
          for (const std::string &v : variants) { Pattern q = h->inner[i]; q.s = v; shp.push_back(q); shid.push_back(h->inner_ids[i]); }
        } else { shp.push_back(h->inner[i]); shid.push_back(h->inner_ids[i]); }
      }
      ShortTables stt;
      why = short_build(shp, shid, h->alpha, sk, h->eos_code, h->knobs.short_tile > 0 ? (size_t)h->knobs.short_tile : 0, &stt);
      if (why.empty() && stt.tiles.size() > 256) why = "too many pattern tiles for pm_short_edit_scan";
      if (why.empty()) {
        HIP_TRY(h, short_upload(stt, &h->shd, h->stream));
        if (h->short_only) { h->sd.k = sk; h->sd.Lw = 16; h->sd.ascii = stt.ascii; h->sd.maxlen = stt.maxlen; }   // (the plan facts the rest of this file reads from h->sd)
      }
    }
    if (why.empty() && h->nssub) {                                  // -K: the class of 16..19 characters beside the pair plan's tiles
      std::vector<Pattern> shp; std::vector<uint32_t> shid;
      std::vector<std::string> variants;
      for (size_t i = 0; i < h->pats.size(); ++i) {
        if (!h->in_ssub[i]) continue;
        if (h->sem == PM_SEM_EXACT_HALVES) { shp.push_back(h->pats[i]); shid.push_back((uint32_t)(i + 1)); }   // whole patterns, as in the main class
        else if (h->wild_seed) {
          expand_iupac(h->inner[i].s, 16, &variants);
          for (const std::string &v : variants) { Pattern q = h->inner[i]; q.s = v; shp.push_back(q); shid.push_back(h->inner_ids[i]); }
        } else { shp.push_back(h->inner[i]); shid.push_back(h->inner_ids[i]); }
      }
      if (h->sem == PM_SEM_SHIFT_AND_INEXACT) for (Pattern &p : shp) { p.esb = 0; p.eeb = 0; }   // (the automaton knows no exact zones, see above)
      ShortSubTables stt;
      why = use_pair ? short_sub_build(shp, shid, h->alpha, sk, h->eos_code, h->knobs.short_tile > 0 ? (size_t)h->knobs.short_tile : 0, &stt)
                     : std::string("the pair plan does not take the list's patterns of 20..32 characters");
      if (why.empty() && stt.tiles.size() > 256) why = "too many pattern tiles for pm_short_sub_scan";
      if (why.empty()) {
        HIP_TRY(h, short_sub_upload(stt, &h->ssd, h->stream));
        h->ssd.viol_level = h->sem == PM_SEM_FILTER_BITVEC ? 3 : 0;  // as the main class's
      }
    }
    if (why.empty() && h->nwild) {                                  // -w: the class of primers with more than 16 concrete variants
      std::vector<Pattern> wp; std::vector<uint32_t> wid;
      for (size_t i = 0; i < h->inner.size(); ++i) if (h->in_wild[i]) { wp.push_back(h->inner[i]); wid.push_back(h->inner_ids[i]); }
      if (h->sem != PM_SEM_FILTER_BITVEC) for (Pattern &p : wp) { p.esb = 0; p.eeb = 0; }   // (the keyword tree and the automata know no exact zones, see above)
      WildTables wt;
      why = wild_build(wp, wid, h->alpha, h->scan_k, h->eos_code, &wt);
      if (why.empty()) {
        HIP_TRY(h, wild_upload(wt, &h->wd, h->stream));
        h->wd.viol_level = h->sem == PM_SEM_FILTER_BITVEC ? 3 : 0;   // as the main class's
        if (h->wild_only) { h->sd.k = sk; h->sd.Lw = 16; h->sd.ascii = wt.ascii; h->sd.maxlen = wt.maxlen; }   // (the plan facts the rest of this file reads from h->sd)
        else h->sd.maxlen = std::max(h->sd.maxlen, wt.maxlen);
      }
    }
    if (!why.empty()) {
      wild_free(&h->wd);
      seed_free(&h->sd);
      for (SeedDevice &d : h->sd_more) seed_free(&d);
      h->sd_more.clear();
      short_free(&h->shd);
      short_sub_free(&h->ssd);
      if (h->kern == PM_KERNEL_SEED) return fail(h, PM_E_UNSUPPORTED, "seed engine: " + why);
      want_seed = false;
    } else {
      if (h->nrest) {
        std::vector<Pattern> rp; std::vector<uint32_t> rid;
        for (size_t i = 0; i < h->inner.size(); ++i) if (h->in_rest[i]) { rp.push_back(h->inner[i]); rid.push_back(h->inner_ids[i]); }
        BitparTables tabs;
        std::string msg = bitpar_build(rp, rid, h->alpha, h->scan_k, h->eos_code, &tabs, h->cfg.wildcards != 0, h->cfg.text_n != 0);
        if (!msg.empty()) return fail(h, PM_E_UNSUPPORTED, "bit-parallel engine (residue): " + msg);
        HIP_TRY(h, bitpar_upload(tabs, h->scan_indels, &h->bp, h->stream));
        h->bp.knobs = h->knobs;
      }
      int mx = h->sd.maxlen;
      for (SeedDevice &d : h->sd_more) mx = std::max(mx, d.maxlen);
      h->sd.maxlen = mx;
      h->kern = PM_KERNEL_SEED;
      if (h->nwild && h->knobs.debug) fprintf(stderr, "[pm] wild class: %zu patterns with more than 16 concrete variants on pm_wild_sub_scan\n", h->nwild);
      h->seed_flags = h->sem == PM_SEM_EXACT_HALVES && !halves_mode;
      h->bases_flags = h->sem == PM_SEM_EXACT_BASES && !h->cfg.indels;
      h->bases_edits = h->sem == PM_SEM_EXACT_BASES && h->cfg.indels;
      h->halves_dev = halves_mode;
      h->half_ranked_any = h->sd.half_ranked;
      for (const SeedDevice &d : h->sd_more) h->half_ranked_any = h->half_ranked_any || d.half_ranked;
      h->edits_dev = edits_mode;
      // The edit plan's first stage on the PAIR geometry (pm_pair.hip): -k 2 on one pattern tile (14 field-pair
      // tests per window instead of 34 hashed piece triples; round 4) -- and, with the PM_EDIT_PAIR bit of
      // pm_config.long_patterns, every tile of a larger list, -k 1 (2 tests instead of 8: pm_pair_edit_scan_k1) and exact_bases
      // (pm_bases_verify behind it; tiles of up to 32 characters, as seed_launch demands).  Its tables are the substitution
      // plan's with two patterns per slot, one set per seed tile over that tile's patterns (the same cut and order as the
      // automaton records of h->sd / h->sd_more: seed records carry indices into them).  A tile pair_build refuses leaves
      // the whole list on pm_edit_scan: routes are never mixed across tiles.
      const bool epair_more = (h->cfg.long_patterns & PM_EDIT_PAIR) && !h->knobs.edit_pair_off;
      const bool epair_base = h->cfg.k == 2 && !h->bases_edits && h->sd_more.empty();
      if (edits_mode && (epair_base || (epair_more && (h->cfg.k == 1 || h->cfg.k == 2) && !(h->bases_edits && h->nlong_edits))) &&
          !h->knobs.edit_bloom && !h->knobs.edit_hash && !sp.empty()) {
        bool ok = true;
        for (size_t ti = 0; ti < ntile && ok; ++ti) {
          const size_t lo = ti * per, hi = std::min(sp.size(), lo + per);
          std::vector<Pattern> tp(sp.begin() + lo, sp.begin() + hi);
          std::vector<uint32_t> tid(sid.begin() + lo, sid.begin() + hi);
          PairTables pt;
          const std::string msg = pair_build(tp, tid, h->alpha, h->cfg.k, h->eos_code, &pt, h->knobs.pair_row, 2, h->nlong_edits ? PAIR_MAX_LEN_WIDE : PAIR_MAX_LEN,
                                             (h->knobs.seed_debug & 64) != 0);   // (the tables read a pattern's last 20 bases only)
          ok = msg.empty();
          if (!ok) break;
          h->epair.emplace_back();
          HIP_TRY(h, pair_upload(pt, &h->epair.back(), h->stream));
          h->epair.back().knobs = h->knobs;
        }
        if (ok && h->epair.size() == 1 + h->sd_more.size()) {
          h->epair_on = true;
          if (h->knobs.debug) fprintf(stderr, "[pm] edit plan: first stage on the pair geometry (k = %d, %zu tiles%s)\n", h->cfg.k, h->epair.size(), h->bases_edits ? ", exact_bases" : "");
        }
        else { for (PairDevice &d : h->epair) pair_free(&d); h->epair.clear(); }
      }
      if (halves_mode) {
        const size_t nh = h->inner.size();
        const size_t hrow = half_row(h);
        std::vector<uint8_t> codes(nh * hrow, 0), lens(nh, 0);
        for (size_t i = 0; i < nh; ++i) {
          lens[i] = (uint8_t)h->inner[i].s.size();
          for (size_t q = 0; q < h->inner[i].s.size() && q < hrow; ++q) codes[i * hrow + q] = (uint8_t)h->alpha.nch[(unsigned char)h->inner[i].s[q]];
        }
        std::vector<int32_t> es(h->pats.size()), ee(h->pats.size());
        for (size_t i = 0; i < h->pats.size(); ++i) { es[i] = h->pats[i].esb; ee[i] = h->pats[i].eeb; }
        { void *hx[] = {h->d_half_codes, h->d_half_len, h->d_hesb, h->d_heeb}; for (void *q : hx) if (q) (void)hipFree(q); }
        PM_TRY(dev_upload(h, &h->d_half_codes, codes, 16, "d_half_codes"));
        PM_TRY(dev_upload(h, &h->d_half_len, lens, 16, "d_half_len"));
        PM_TRY(dev_upload(h, &h->d_hesb, es, 16, "d_hesb"));
        PM_TRY(dev_upload(h, &h->d_heeb, ee, 16, "d_heeb"));
      }
      h->seed_k = sk;
    }
  }
  if (!want_seed) {
    h->nlong_exact = 0; h->nlong_edits = 0; h->nlong_halves = 0;    // (no wide tile was kept: the stream edges and pm_describe are the bit-parallel family's)
    h->halves_dev = false; h->edits_dev = false; h->half_ranked_any = false;
    std::fill(h->in_rest.begin(), h->in_rest.end(), 0); h->nrest = 0;
    std::fill(h->in_short.begin(), h->in_short.end(), 0); h->nshort = 0; h->short_only = false;
    std::fill(h->in_ssub.begin(), h->in_ssub.end(), 0); h->nssub = 0;
    std::fill(h->in_wild.begin(), h->in_wild.end(), 0); h->nwild = 0; h->nwild_long = 0; h->wild_only = false;
    h->kern = PM_KERNEL_BITPAR;
    BitparTables tabs;
    std::string msg = bitpar_build(h->inner, h->inner_ids, h->alpha, h->scan_k, h->eos_code, &tabs,
                                   h->cfg.wildcards != 0, h->cfg.text_n != 0);
    if (!msg.empty()) return fail(h, PM_E_UNSUPPORTED, "bit-parallel engine: " + msg);
    HIP_TRY(h, bitpar_upload(tabs, h->scan_indels, &h->bp, h->stream));
    h->bp.knobs = h->knobs;
  }
  if (!h->d_counter) HIP_TRY(h, hipMalloc((void **)&h->d_counter, sizeof(unsigned long long)));
  if (!h->h_counter) HIP_TRY(h, hipHostMalloc((void **)&h->h_counter, sizeof(unsigned long long), hipHostMallocDefault));
  if (!h->h_seed_count) { HIP_TRY(h, hipHostMalloc((void **)&h->h_seed_count, SEEDCOUNT_WORDS * sizeof(unsigned long long), hipHostMallocDefault)); memset(h->h_seed_count, 0, SEEDCOUNT_WORDS * sizeof(unsigned long long)); }
  if (!h->ev0) HIP_TRY(h, hipEventCreate(&h->ev0));
  if (!h->ev1) HIP_TRY(h, hipEventCreate(&h->ev1));
  if (!h->host_only) {
    if (!h->ev_fin) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_fin, hipEventDisableTiming));
    if (!h->copy_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
  }
  if (!h->d_cands) { rc = ensure_capacity(h, (size_t)1 << 20); if (rc) return rc; }
  if (h->edits_dev && !h->host_only) {                              // every candidate is reported by several seeds before the dedup
    const int64_t span = h->win ? std::min(h->n, h->win) : h->n;    // (a windowed handle scans at most a window at a time)
    const size_t want = std::min<size_t>(std::max<size_t>((size_t)(span / 24), (size_t)1 << 22), (size_t)1 << 28);
    if (h->cap < want) { rc = ensure_capacity(h, want); if (rc) return rc; }
  }
  device_sort_plan(h);
  // pm_scan's landing buffer for a database-sized stream: pinned now, beside the upload, rather than inside the first range
  // (2^20 records = 16 MiB take ~5 ms to pin; a 1 GiB range of uniform text hands back 3.3e5 -K 2 hits, 1.2e6 with -k 2)
  if (!h->host_only && h->n >= ((int64_t)1 << 28) && h->land_cap < ((size_t)1 << 20)) { rc = ensure_landing(h, (size_t)1 << 20); if (rc) return rc; }
  h->internal_rescans = 0; h->range_splits = 0; h->lookaheads = 0; h->dense_mode = false; h->piece_len = 0;
  h->inited = true;
  return pm_reset(h);
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Host stream -> HBM.  A single hipMemcpy from pageable memory runs at the speed of one core's copy
// into the runtime's staging buffer (≈11 GB/s here); several threads, each staging its slice
// through two pinned buffers of its own on its own HIP stream, fill the PCIe link instead.
static hipError_t upload_stream(int device, void *d, const uint8_t *text, size_t n) {
  constexpr size_t CH = (size_t)8 << 20;
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const int T = (int)std::min<size_t>(std::min<unsigned>(6u, hw), (n + 4 * CH - 1) / (4 * CH));
  if (T <= 1) return hipMemcpy(d, text, n, hipMemcpyHostToDevice);
  std::vector<hipError_t> errs((size_t)T, hipSuccess);
  std::vector<std::thread> th;
  const size_t per = ((n + (size_t)T - 1) / (size_t)T + CH - 1) / CH * CH;
  for (int t = 0; t < T; ++t) th.emplace_back([&, t]() {
    hipError_t e = hipSetDevice(device);
    const size_t lo = std::min(n, (size_t)t * per), hi = std::min(n, lo + per);
    hipStream_t st = nullptr;
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
      e = hipHostMalloc(&pin[b], CH, hipHostMallocDefault);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[b], hipEventDisableTiming);
    }
    int b = 0;
    for (size_t off = lo; off < hi && e == hipSuccess; off += CH, b ^= 1) {
      const size_t len = std::min(CH, hi - off);
      e = hipEventSynchronize(ev[b]);                               // the copy that last used this buffer is done
      if (e != hipSuccess) break;
      memcpy(pin[b], text + off, len);
      e = hipMemcpyAsync((char *)d + off, pin[b], len, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = hipEventRecord(ev[b], st);
    }
    if (st) { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }
    for (int q = 0; q < 2; ++q) { if (ev[q]) (void)hipEventDestroy(ev[q]); if (pin[q]) (void)hipHostFree(pin[q]); }
    if (st) (void)hipStreamDestroy(st);
    errs[(size_t)t] = e;
  });
  for (std::thread &x : th) x.join();
  for (hipError_t e : errs) if (e != hipSuccess) return e;
  return hipSuccess;
}

// The seed family's first stage reads the stream at 2 bits per base (pm_seed.hip pack_stream): one
// pass over the stream per pm_init, on the handle's stream, after the bytes are in HBM.
static int ensure_words(pm_handle *h) {
  const size_t words = (size_t)((h->n + 15) / 16);
  if (!h->d_packed || h->packed_cap < words) {
    if (h->d_packed) (void)hipFree(h->d_packed);
    h->d_packed = nullptr;
    h->packed_cap = words;
    HIP_TRY(h, hipMalloc((void **)&h->d_packed, (words + 128) * sizeof(uint32_t)));   // + padding the scan kernels' block prefetch may read (zeroed by the caller)
  }
  return PM_OK;
}
static int ensure_packed(pm_handle *h) {
  if (h->kern != PM_KERNEL_SEED) return PM_OK;
  const size_t words = (size_t)((h->n + 15) / 16);
  { const int rc = ensure_words(h); if (rc) return rc; }
  if (h->n >= 16) HIP_TRY(h, pack_stream(h->d_text, 16, h->sd.ascii, h->d_packed + words + 64, 1, h->stream));   // the kernel's code is resident before the timed pass
  HIP_TRY(h, hipStreamSynchronize(h->stream));                      // table uploads of this init are not part of the figure
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  HIP_TRY(h, hipMemsetAsync(h->d_packed + words, 0, 128 * sizeof(uint32_t), h->stream));
  HIP_TRY(h, pack_stream(h->d_text, h->n, h->sd.ascii, h->d_packed, (int64_t)words, h->stream));
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  HIP_TRY(h, hipEventSynchronize(h->ev1));
  (void)hipEventElapsedTime(&h->pack_ms, h->ev0, h->ev1);
  return PM_OK;
}

// ---- windowed stream (pm_init_windowed) -------------------------------------

// How far the device stages of this handle read stream text behind and ahead of a scanned range (begin, end]:
//  - scan kernels: a hit that ends at e reads [e - L - k, e) (bit-parallel rows, seed and pair windows); the pair
//    geometry of the edit plan scans begin - 3 .. end + 2; exact_bases -k widens its range by L + 2k + 4 on both sides
//    (pm_scan_candidates_async) and then reads L + k behind that; exact_halves reads the zero bytes past n (overhang);
//  - finalize stages: extend_seeds reads L + k on either side of a seed, cluster_dp_device [first - L - k, last] of a
//    cluster (carried clusters: carry_reach), gather_windows is not used (the handle has the host copy);
//  - the seed family's kernels carry 16 bases from one block of 1024 into the next.
// L = the longest pattern; 64 bases of slack on top.  The kernels also READ text whose characters cannot reach a hit in
// (begin, end]: the bit-parallel kernel runs its automaton from the start of the aligned segment that holds `begin` (up to
// 4 Mi positions in front of it), a wave of the seed and pair kernels walks its whole sub-range of an aligned chunk and
// prefetches four blocks of 1024 bases ahead -- the guard margins of a slot (pm_init_windowed) cover those reads.
static void stream_halo(const pm_handle *h, int64_t *back, int64_t *fwd) {
  int64_t L = 0;
  for (const Pattern &p : h->pats) L = std::max<int64_t>(L, (int64_t)p.s.size());
  const int64_t k = h->cfg.k;
  const int64_t r = 2 * L + 3 * k + 4 + 16 + 64;
  *back = (r + 63) / 64 * 64;
  *fwd = *back;
}

// Where the records of a scan become final hits: the handle's route through the finalize stage, decided by its option set.
enum class Route {
  Host,                               // pm_finalize: the order-dependent rules of the reference wrappers on the host
  Passthrough,                        // the records are the hits
  Cluster,                            // filter_bitvec -K: clusters and "smallest level, left-most end" on the device (pm_cluster.hip)
  ClusterDp,                          // filter_bitvec -k on the seed family (A,C,G,T patterns of <= 32 characters): clusters and their DPs on the device
  Halves                              // exact_halves on the seed family: its per-pattern sequential rule as a sort + one walk per pattern (pm_halves_rule)
};
static bool device_cluster_plain(const pm_handle *h);
static Route finalize_route(const pm_handle *h) {
  if (h->sem == PM_SEM_EXACT_HALVES && (h->seed_flags || h->halves_dev) && h->pats.size() < ((size_t)1 << 22) - 1) return Route::Halves;
  if (h->sem == PM_SEM_KEYWORD_TREE || h->sem == PM_SEM_SHIFT_AND || h->sem == PM_SEM_SHIFT_AND_INEXACT || (h->sem == PM_SEM_EXACT_BASES && h->bases_flags))
    return Route::Passthrough;
  if (h->sem == PM_SEM_FILTER_BITVEC && h->edits_dev && !h->cfg.wildcards && h->pats.size() < ((size_t)1 << 22)) return Route::ClusterDp;
  return device_cluster_plain(h) ? Route::Cluster : Route::Host;
}

// the records pm_scan carries into the next piece: the earliest text the device cluster DP will read for them
static int64_t carry_reach(const pm_handle *h) {
  int64_t lo = INT64_MAX, L = 0;
  for (const pm_hit &c : h->carry) lo = std::min(lo, c.end);
  for (const Pattern &p : h->pats) L = std::max<int64_t>(L, (int64_t)p.s.size());
  return lo == INT64_MAX ? lo : lo - L - h->cfg.k - 64;
}

// longest piece pm_scan hands to one window: the piece plus its halo (and the 64-byte alignment of a window start) fit
static int64_t win_piece_cap(const pm_handle *h) { return h->win - h->win_back - h->win_fwd - 64; }

static size_t slot_bytes(const pm_handle *h, int64_t cap) { return (size_t)(cap + 2 * h->win_guard); }
static size_t slot_words(const pm_handle *h, int64_t cap) { return (size_t)((cap + 2 * h->win_guard) / 16 + 128); }

// bytes of a slot's packed buffer: `cap` codes (cap is a multiple of 64: whole bytes) and one 8-byte word of slack
static size_t slot_packed(const pm_handle *h, int64_t cap) { return (size_t)(cap / 8 * h->pk_bits + 8); }

static void win_account(pm_handle *h) {
  int64_t held = 0;
  for (const WinSlot &s : h->slot) {
    if (s.bytes) held += (int64_t)slot_bytes(h, s.cap);
    if (s.words) held += (int64_t)slot_words(h, s.cap) * 4;
    if (s.pk) held += (int64_t)slot_packed(h, s.cap);
  }
  h->win_held = held;
  h->win_peak = std::max(h->win_peak, held);
}

static void win_release(pm_handle *h) {
  if (!h->win && !h->up_stream && !h->stage_st[0] && !h->slot[0].bytes && !h->slot[1].bytes) return;
  (void)hipStreamSynchronize(h->stream);
  if (h->up_stream) (void)hipStreamSynchronize(h->up_stream);
  for (int t = 0; t < WIN_UP_THREADS; ++t) if (h->stage_st[t]) (void)hipStreamSynchronize(h->stage_st[t]);
  for (WinSlot &s : h->slot) {
    if (s.bytes) (void)hipFree(s.bytes);
    if (s.words) (void)hipFree(s.words);
    if (s.pk) (void)hipFree(s.pk);
    if (s.ready) (void)hipEventDestroy(s.ready);
    if (s.used) (void)hipEventDestroy(s.used);
    s = WinSlot();
  }
  for (int t = 0; t < WIN_UP_THREADS; ++t) {
    for (int q = 0; q < 2; ++q) {
      if (h->stage[t][q]) (void)hipHostFree(h->stage[t][q]);
      if (h->stage_ev[t][q]) (void)hipEventDestroy(h->stage_ev[t][q]);
      h->stage[t][q] = nullptr; h->stage_ev[t][q] = nullptr;
    }
    if (h->stage_done[t]) (void)hipEventDestroy(h->stage_done[t]);
    if (h->stage_st[t]) (void)hipStreamDestroy(h->stage_st[t]);
    h->stage_done[t] = nullptr; h->stage_st[t] = nullptr;
  }
  if (h->up_stream) (void)hipStreamDestroy(h->up_stream);
  h->up_stream = nullptr;
  if (h->win) { h->d_text = nullptr; h->d_packed = nullptr; h->packed_cap = 0; }   // (pointers into the slots, not allocations)
  h->win = 0; h->bound = -1;
  h->win_held = h->win_peak = h->win_uploaded = h->win_loads = 0;
}

// Upload stream text [lo, hi) into slot si (not the bound one) and pack it.  On a pm_init_packed handle the bytes that cross
// PCIe are the window's slice of the packed stream (lo is a multiple of 64 codes, so the slice starts on a whole byte, 8-byte
// aligned): they go into the slot's packed buffer and one kernel on the upload stream unpacks them into text and words.  The host copies chunks into pinned staging
// buffers, up to WIN_UP_THREADS threads on streams of their own (upload_stream's pattern); the copies wait for the last
// kernel that read the slot (its `used` event), the packing runs on the upload stream behind them and `ready` marks the
// end.  Returns once the last chunk is staged: the copies of the last chunks still run while the caller goes on.
static int win_load(pm_handle *h, int si, int64_t lo, int64_t hi) {
  WinSlot &s = h->slot[si];
  const int64_t len = hi - lo;
  const int64_t G = h->win_guard;
  const bool packed = h->kern == PM_KERNEL_SEED;
  const int pkb = h->pk_bits;                                       // > 0: the host form is bit-packed
  if (!s.ready) HIP_TRY(h, hipEventCreateWithFlags(&s.ready, hipEventDisableTiming));
  if (!s.used) HIP_TRY(h, hipEventCreateWithFlags(&s.used, hipEventDisableTiming));
  if (!h->up_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->up_stream, hipStreamNonBlocking));
  if (!h->stage_st[0]) {
    for (int t = 0; t < WIN_UP_THREADS; ++t) {
      HIP_TRY(h, hipStreamCreateWithFlags(&h->stage_st[t], hipStreamNonBlocking));
      HIP_TRY(h, hipEventCreateWithFlags(&h->stage_done[t], hipEventDisableTiming));
      for (int q = 0; q < 2; ++q) HIP_TRY(h, hipEventCreateWithFlags(&h->stage_ev[t][q], hipEventDisableTiming));
    }
  }
  if (!s.bytes || s.cap < len || (packed && !s.words) || (pkb && !s.pk)) {           // first use, or a carried chain that needs more than a window
    if (s.used_rec) HIP_TRY(h, hipEventSynchronize(s.used));
    for (int t = 0; t < WIN_UP_THREADS; ++t) if (h->stage_st[t]) HIP_TRY(h, hipStreamSynchronize(h->stage_st[t]));   // (an earlier upload into it)
    HIP_TRY(h, hipStreamSynchronize(h->up_stream));
    if (s.bytes) (void)hipFree(s.bytes);
    if (s.words) (void)hipFree(s.words);
    if (s.pk) (void)hipFree(s.pk);
    s.bytes = nullptr; s.words = nullptr; s.pk = nullptr;
    s.cap = std::max(h->win, (len + 63) / 64 * 64);
    HIP_TRY(h, hipMalloc((void **)&s.bytes, slot_bytes(h, s.cap)));
    HIP_TRY(h, hipMemsetAsync(s.bytes, 0, slot_bytes(h, s.cap), h->up_stream));
    if (packed) {
      HIP_TRY(h, hipMalloc((void **)&s.words, slot_words(h, s.cap) * 4));
      HIP_TRY(h, hipMemsetAsync(s.words, 0, slot_words(h, s.cap) * 4, h->up_stream));
    }
    if (pkb) HIP_TRY(h, hipMalloc((void **)&s.pk, slot_packed(h, s.cap)));
    win_account(h);
    HIP_TRY(h, hipStreamSynchronize(h->up_stream));
  }
  s.loaded = false;
  uint8_t *dst = s.bytes + G;
  // what the staging threads copy, and where to: the text itself into the slot, or its packed slice into the packed buffer
  const int64_t plo = pkb ? lo / 8 * pkb : 0;
  const int64_t up_len = pkb ? std::min(h->h_packed_bytes, (hi * pkb + 7) / 8) - plo : len;
  const uint8_t *src = pkb ? h->h_packed + plo : h->h_text + lo;
  uint8_t *up_dst = pkb ? s.pk : dst;
  const int T = (int)std::min<int64_t>(WIN_UP_THREADS, std::max<int64_t>(1, up_len / (4 * WIN_UP_CHUNK)));
  for (int t = 0; t < T; ++t)
    for (int q = 0; q < 2; ++q)
      if (!h->stage[t][q]) HIP_TRY(h, hipHostMalloc((void **)&h->stage[t][q], (size_t)WIN_UP_CHUNK, hipHostMallocDefault));
  const int64_t per = ((up_len + T - 1) / T + WIN_UP_CHUNK - 1) / WIN_UP_CHUNK * WIN_UP_CHUNK;
  std::vector<hipError_t> errs((size_t)T, hipSuccess);
  const bool wait_used = s.used_rec;
  auto work = [&](int t) {
    hipError_t e = hipSetDevice(h->cfg.device);
    const int64_t a = std::min(up_len, (int64_t)t * per), b = std::min(up_len, a + per);
    // the text is overwritten once its last reader is done; the packed buffer once the unpack of the slot's last load is
    if (e == hipSuccess && pkb) e = hipStreamWaitEvent(h->stage_st[t], s.ready, 0);
    else if (e == hipSuccess && wait_used) e = hipStreamWaitEvent(h->stage_st[t], s.used, 0);
    int q = 0;
    for (int64_t off = a; off < b && e == hipSuccess; off += WIN_UP_CHUNK, q ^= 1) {
      const size_t m = (size_t)std::min<int64_t>(WIN_UP_CHUNK, b - off);
      e = hipEventSynchronize(h->stage_ev[t][q]);                   // the copy that last used this buffer is done
      if (e != hipSuccess) break;
      memcpy(h->stage[t][q], src + off, m);
      e = hipMemcpyAsync(up_dst + off, h->stage[t][q], m, hipMemcpyHostToDevice, h->stage_st[t]);
      if (e == hipSuccess) e = hipEventRecord(h->stage_ev[t][q], h->stage_st[t]);
    }
    if (e == hipSuccess) e = hipEventRecord(h->stage_done[t], h->stage_st[t]);
    errs[(size_t)t] = e;
  };
  if (T == 1) work(0);
  else {
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(work, t);
    for (std::thread &x : th) x.join();
  }
  for (hipError_t e : errs) if (e != hipSuccess) return hipfail(h, e, "window upload");
  for (int t = 0; t < T; ++t) HIP_TRY(h, hipStreamWaitEvent(h->up_stream, h->stage_done[t], 0));
  if (pkb) {
    if (wait_used) HIP_TRY(h, hipStreamWaitEvent(h->up_stream, s.used, 0));
    HIP_TRY(h, unpack_stream(s.pk, up_len, pkb, len, h->sd.ascii, dst, packed ? s.words + G / 16 : nullptr, h->up_stream));
  }
  if (hi == h->n) HIP_TRY(h, hipMemsetAsync(dst + len, 0, 64, h->up_stream));     // the zero bytes past the end of the stream
  if (packed && pkb) {
    if (hi == h->n) HIP_TRY(h, hipMemsetAsync(s.words + G / 16 + (len + 15) / 16, 0, 128 * sizeof(uint32_t), h->up_stream));
  } else if (packed) {
    const int64_t nw = (len + 15) / 16;
    uint32_t *wdst = s.words + G / 16;
    HIP_TRY(h, pack_stream(dst, len, h->sd.ascii, wdst, nw, h->up_stream));       // (lo is a multiple of 64: words rebase like bytes)
    if (hi == h->n) HIP_TRY(h, hipMemsetAsync(wdst + nw, 0, 128 * sizeof(uint32_t), h->up_stream));
  }
  HIP_TRY(h, hipEventRecord(s.ready, h->up_stream));
  s.lo = lo; s.hi = hi; s.loaded = true;
  h->win_uploaded += up_len; ++h->win_loads;
  return PM_OK;
}

// Point d_text / d_packed at slot si; the handle's stream waits for its upload.  The slot given up is marked used up to
// here: everything that reads it was enqueued on the handle's stream before.
static int win_bind(pm_handle *h, int si) {
  if (h->bound != si) {
    if (h->bound >= 0) {
      HIP_TRY(h, hipEventRecord(h->slot[h->bound].used, h->stream));
      h->slot[h->bound].used_rec = true;
    }
    h->bound = si;
  }
  const WinSlot &s = h->slot[si];
  const uintptr_t G = (uintptr_t)h->win_guard;
  h->d_text = (const uint8_t *)((uintptr_t)s.bytes + G - (uintptr_t)s.lo);
  h->d_packed = s.words ? (uint32_t *)((uintptr_t)s.words + (G / 16) * 4 - (uintptr_t)(s.lo / 16) * 4) : nullptr;
  HIP_TRY(h, hipStreamWaitEvent(h->stream, s.ready, 0));
  return PM_OK;
}

// Make stream text [lo, hi) (clipped to the stream) resident and bound.  A slot that holds it is bound as it is; else the
// other slot takes the window [lo, lo + win).  A span longer than a window: `grow` (pm_scan, a carried chain) enlarges
// the slot, otherwise PM_E_INVALID.
static int win_need(pm_handle *h, int64_t lo, int64_t hi, bool grow, const char *who) {
  lo = std::max<int64_t>(0, lo) / 64 * 64;
  hi = std::max(lo, std::min(h->n, hi));
  for (int si = 0; si < 2; ++si) {
    const WinSlot &s = h->slot[si];
    if (s.loaded && s.lo <= lo && s.hi >= hi) return win_bind(h, si);
  }
  if (hi - lo > h->win && !grow)
    return fail(h, PM_E_INVALID, std::string(who) + ": the range needs " + std::to_string(hi - lo) + " bytes of stream text with its halo, more than the window of " +
                                 std::to_string(h->win) + " bytes (pm_init_windowed)");
  const int si = h->bound == 0 ? 1 : 0;
  const int64_t top = std::min(h->n, std::max((hi + 63) / 64 * 64, lo + h->win));
  int rc = win_load(h, si, lo, top);
  if (rc) return rc;
  return win_bind(h, si);
}

// pm_scan's look-ahead: when the range that follows (end, end + len] would not fit the bound window, the window it needs
// goes into the other slot now, while the GPU scans the current one.
static void win_prefetch(pm_handle *h, int64_t end, int64_t len) {
  if (!h->win || h->bound < 0 || end >= h->n) return;
  if (std::min(h->n, end + len + h->win_fwd) <= h->slot[h->bound].hi) return;
  const int64_t nlo = std::max<int64_t>(0, end - h->win_back) / 64 * 64;
  const int o = 1 - h->bound;
  if (h->slot[o].loaded && h->slot[o].lo == nlo) return;
  (void)win_load(h, o, nlo, std::min(h->n, nlo + h->win));          // (a failure leaves the slot unloaded: the next range loads it itself)
}

// One stream per handle.  Drops the stream of an earlier init -- its window ring, an owned text: before the new one takes
// memory -- and names the new one: n codes, on the host at `text` (NULL: none, or bit-packed: pm_init_packed sets those
// fields itself), in HBM at d_text or, with `own`, in n + 16 bytes allocated here.  On the default stream, with a device stage.
static int set_stream_source(pm_handle *h, int64_t n, const uint8_t *text, const void *d_text, bool own) {
  win_release(h);
  if (h->own_d_text && h->d_text) (void)hipFree((void *)h->d_text);
  h->d_text = nullptr; h->own_d_text = false;
  void *d = nullptr;
  if (own) { HIP_TRY(h, hipMalloc(&d, (size_t)(n > 0 ? n : 1) + 16)); d_text = d; }
  h->d_text = (const uint8_t *)d_text; h->own_d_text = own; h->h_text = text; h->n = n; h->stream = nullptr; h->host_only = false;
  h->h_packed = nullptr; h->h_packed_bytes = 0; h->pk_bits = 0; h->pk_peak_extra = 0;
  return PM_OK;
}

// `bytes` of the stream's host form go to d while init_common builds the pattern tables: with `overlap` on a second
// thread -- the stream crosses PCIe (≈0.3 s for 3 GB of pageable memory) beside the table build --, else in one copy first.
// An upload that failed is reported in `who`'s name after the table build; else the result is init_common's.  (pm_init
// makes its one-copy upload itself and passes bytes = 0: it returns before the tables when that copy fails.)  ti0: when `who` began.
static int upload_and_init(pm_handle *h, const char *who, void *d, const uint8_t *src, int64_t bytes, bool overlap,
                           const uint8_t *table, int32_t table_len, double ti0) {
  const double ti1 = now_ms();
  hipError_t copy_err = hipSuccess;
  std::thread copier;
  if (bytes > 0 && overlap) {
    const int dev = h->cfg.device;
    copier = std::thread([=, &copy_err]() {
      copy_err = hipSetDevice(dev);
      if (copy_err == hipSuccess) copy_err = upload_stream(dev, d, src, (size_t)bytes);
    });
  } else if (bytes > 0) copy_err = hipMemcpy(d, src, (size_t)bytes, hipMemcpyHostToDevice);
  const int rc = init_common(h, table, table_len);
  const double ti2 = now_ms();
  if (copier.joinable()) copier.join();
  if (h->knobs.debug) fprintf(stderr, "[pm] %s: runtime + stream buffers %.0f ms, tables %.0f ms, then %.0f ms more for the upload of %lld bytes\n", who, ti1 - ti0, ti2 - ti1, now_ms() - ti2, (long long)bytes);
  if (copy_err != hipSuccess) return fail(h, PM_E_HIP, std::string(who) + ": stream upload: " + hipGetErrorString(copy_err));
  return rc;
}

extern "C" int pm_init(pm_handle *h, const uint8_t *text, int64_t n, const uint8_t *table, int32_t table_len) {
  if (!h || (!text && n > 0) || n < 0) return fail(h, PM_E_INVALID, "pm_init: bad arguments");
  const double ti0 = now_ms();
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  PM_TRY(set_stream_source(h, n, text, nullptr, true));
  // raw streams with wildcards look at the stream on the device first, so they wait for it
  const bool overlap = n > ((int64_t)1 << 24) && !(!table && h->cfg.wildcards);
  void *d = (void *)h->d_text;
  if (!overlap && n > 0) HIP_TRY(h, hipMemcpy(d, text, (size_t)n, hipMemcpyHostToDevice));   // (a failure returns before the tables are touched)
  PM_TRY(upload_and_init(h, "pm_init", d, text, overlap ? n : 0, true, table, table_len, ti0));
  return ensure_packed(h);
}

extern "C" int pm_init_host(pm_handle *h, const uint8_t *text, int64_t n, const uint8_t *table, int32_t table_len) {
  if (!h || (!text && n > 0) || n < 0) return fail(h, PM_E_INVALID, "pm_init_host: bad arguments");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  PM_TRY(set_stream_source(h, n, text, nullptr, false));
  h->host_only = true;
  return init_common(h, table, table_len);
}

extern "C" int pm_init_device(pm_handle *h, const void *d_text, int64_t n, const uint8_t *table, int32_t table_len,
                              void *hip_stream) {
  if (!h || (!d_text && n > 0) || n < 0) return fail(h, PM_E_INVALID, "pm_init_device: bad arguments");
  if (((uintptr_t)d_text) & 3) return fail(h, PM_E_INVALID, "pm_init_device: stream must be 4-byte aligned");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  PM_TRY(set_stream_source(h, n, nullptr, d_text, false));
  h->stream = (hipStream_t)hip_stream;
  PM_TRY(init_common(h, table, table_len));
  return ensure_packed(h);
}

// the part pm_init_windowed and the windowed form of pm_init_packed share: the stream's source is set by the caller
static int init_window_ring(pm_handle *h, const uint8_t *table, int32_t table_len, int64_t window_bytes);

extern "C" int pm_init_windowed(pm_handle *h, const uint8_t *text, int64_t n, const uint8_t *table, int32_t table_len,
                                int64_t window_bytes) {
  if (!h || (!text && n > 0) || n < 0 || window_bytes <= 0) return fail(h, PM_E_INVALID, "pm_init_windowed: bad arguments");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  PM_TRY(set_stream_source(h, n, text, nullptr, false));
  return init_window_ring(h, table, table_len, window_bytes);
}

static int init_window_ring(pm_handle *h, const uint8_t *table, int32_t table_len, int64_t window_bytes) {
  if (h->d_packed) (void)hipFree(h->d_packed);                      // (a resident init's 2-bit copy)
  h->d_packed = nullptr; h->packed_cap = 0;
  stream_halo(h, &h->win_back, &h->win_fwd);
  // guard: the halo plus the longest aligned run a kernel starts in front of `begin` (bit-parallel segment: 4 Mi positions,
  // seed / pair chunk: 2 Mi, or what the test knobs set) and the seed kernels' prefetch of four blocks of 1024 bases ahead
  const int64_t run = std::max<int64_t>({(int64_t)1 << 22, h->knobs.seed_chunk, 64 * h->knobs.bitpar_seglen});
  h->win_guard = (std::max(h->win_back, h->win_fwd) + run + 512 + 16384 + 63) / 64 * 64;
  const int64_t minimum = 4 * (h->win_back + h->win_fwd);
  h->win = std::max(minimum, (window_bytes + 63) / 64 * 64);
  h->bound = -1;
  return init_common(h, table, table_len);
}

extern "C" int pm_init_packed(pm_handle *h, const uint8_t *packed, int64_t packed_bytes, int32_t bits, int64_t n,
                              const uint8_t *table, int32_t table_len, int64_t window_bytes) {
  if (!h) return PM_E_INVALID;
  if (bits < 1 || bits > 8) return fail(h, PM_E_INVALID, "pm_init_packed: bits per code must be 1..8");
  if (n < 0 || packed_bytes < 0 || window_bytes < 0 || packed_bytes > ((int64_t)1 << 59)) return fail(h, PM_E_INVALID, "pm_init_packed: negative size");
  if (n > packed_bytes * 8 / bits) return fail(h, PM_E_INVALID, "pm_init_packed: n codes do not fit packed_bytes");
  if (!packed && n > 0) return fail(h, PM_E_INVALID, "pm_init_packed: no packed bytes");
  if (!table || table_len <= 0) return fail(h, PM_E_INVALID, "pm_init_packed: a packed stream is a normalized one and needs its table");
  if (table_len > (1 << bits)) return fail(h, PM_E_INVALID, "pm_init_packed: the table has more symbols than codes of this width");
  const double ti0 = now_ms();
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  PM_TRY(set_stream_source(h, n, nullptr, nullptr, window_bytes == 0));
  h->h_packed = packed; h->h_packed_bytes = packed_bytes; h->pk_bits = bits;
  if (window_bytes > 0) return init_window_ring(h, table, table_len, window_bytes);
  // resident: the packed bytes cross PCIe as they are (upload_stream, beside the pattern-table build) into a staging buffer
  // in HBM; one kernel on the handle's stream unpacks them into the owned text and, for the seed family, its 2-bit words
  const int64_t up = (n * bits + 7) / 8;
  void *d = (void *)h->d_text, *d_pk = nullptr;
  HIP_TRY(h, hipMalloc(&d_pk, (size_t)up + 8));
  int rc = upload_and_init(h, "pm_init_packed", d_pk, packed, up, up > ((int64_t)1 << 24), table, table_len, ti0);
  const bool words = h->kern == PM_KERNEL_SEED;
  if (!rc && words) rc = ensure_words(h);
  if (rc) { (void)hipFree(d_pk); return rc; }
  h->pk_peak_extra = up + 8;
  auto unpack = [&]() -> int {
    const size_t nw = (size_t)((n + 15) / 16);
    if (n >= 16) HIP_TRY(h, unpack_stream(d_pk, up, bits, 16, h->sd.ascii, d, words ? h->d_packed + nw + 64 : nullptr, h->stream));   // the kernel's code is resident before the timed pass
    HIP_TRY(h, hipStreamSynchronize(h->stream));                    // table uploads of this init are not part of the figure
    HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
    if (words) HIP_TRY(h, hipMemsetAsync(h->d_packed + nw, 0, 128 * sizeof(uint32_t), h->stream));
    HIP_TRY(h, unpack_stream(d_pk, up, bits, n, h->sd.ascii, d, words ? h->d_packed : nullptr, h->stream));
    HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
    HIP_TRY(h, hipEventSynchronize(h->ev1));
    (void)hipEventElapsedTime(&h->pack_ms, h->ev0, h->ev1);
    return PM_OK;
  };
  rc = unpack();
  (void)hipFree(d_pk);
  return rc;
}

extern "C" int pm_stream_residency(const pm_handle *h, int64_t *out, int n) {
  if (!h || !h->inited || !out || n < 0) return PM_E_INVALID;
  int64_t v[6] = {0, 0, 0, 0, 0, h->pk_bits};
  if (h->win) {
    v[0] = h->win; v[1] = h->win_held; v[2] = h->win_peak; v[3] = h->win_uploaded; v[4] = h->win_loads;
  } else if (!h->host_only) {                                       // the whole stream (pm_init: uploaded once; pm_init_device: the caller's)
    v[1] = (h->d_text ? (h->own_d_text ? h->n + 16 : h->n) : 0) + (h->d_packed ? (int64_t)(h->packed_cap + 128) * 4 : 0);
    v[2] = v[1] + h->pk_peak_extra;
    v[3] = !h->own_d_text ? 0 : h->pk_bits ? (h->n * h->pk_bits + 7) / 8 : h->n;
    v[4] = h->own_d_text ? 1 : 0;
  }
  for (int i = 0; i < n && i < 6; ++i) out[i] = v[i];
  return PM_OK;
}

extern "C" int pm_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes) {
  if (!free_bytes || !total_bytes) return PM_E_INVALID;
  if (hipSetDevice(device) != hipSuccess) return PM_E_HIP;
  size_t fr = 0, tot = 0;
  if (hipMemGetInfo(&fr, &tot) != hipSuccess) return PM_E_HIP;
  *free_bytes = (int64_t)fr; *total_bytes = (int64_t)tot;
  return PM_OK;
}

extern "C" int pm_set_capacity(pm_handle *h, size_t max_candidates) {
  if (!h || max_candidates == 0) return PM_E_INVALID;
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  drain_spec(h);
  return ensure_capacity(h, max_candidates, true);
}

extern "C" int pm_reset(pm_handle *h) {
  if (!h) return PM_E_INVALID;
  drain_spec(h);
  if (h->scan_pending) { (void)hipStreamSynchronize(h->stream); h->scan_pending = false; }
  h->carry.clear(); h->land_n = h->land_pos = 0; h->next_begin = 0;
  std::fill(h->lasthit.begin(), h->lasthit.end(), 0);
  h->halves_fresh = true;
  h->last_count = 0;
  h->scan_mode = 0;
  h->held_n = 0; h->pcr_fed = 0; h->pcr_scanning = false;
  for (uint64_t &v : h->pcr_stat) v = 0;
  return count_clear(h);
}

extern "C" void pm_destroy(pm_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device);
  free_device(h);
  delete h;
}

extern "C" const char *pm_last_error(const pm_handle *h) { return h ? h->err.c_str() : g_create_error.c_str(); }
extern "C" int pm_selected_semantics(const pm_handle *h) { return h && h->inited ? h->sem : PM_E_INVALID; }
extern "C" int pm_selected_kernel(const pm_handle *h) { return h && h->inited ? h->kern : PM_E_INVALID; }

// workgroup -> (field pair, chunk) of the pair kernels (pm_workmap.h): "xcd" = every XCD walks its share of the chunks one
// field pair after the other; "superchunk" = runs of 256 chunks per field pair over the whole grid
static const char *pair_schedule_name(const ScanGeometry &g) {
  return g.work_map == PAIR_MAP_XCD_SUPERCHUNK ? "xcd-superchunk" : g.work_map == PAIR_MAP_XCD ? "xcd" : "superchunk";
}

extern "C" int pm_describe(const pm_handle *h, char *buf, size_t buflen) {
  if (!h || !buf || !h->inited) return PM_E_INVALID;
  char wild_long[96] = "";                                          // the wild class's primers of 33..64 characters; none: the text it always had
  if (h->nwild_long) snprintf(wild_long, sizeof(wild_long), ", %zu of them of 33..64 characters: pm_wild_sub_verify_wide", h->nwild_long);
  if (h->kern == PM_KERNEL_SEED && h->wild_only) {
    snprintf(buf, buflen, "kernel=pm_wild_sub_scan+pm_wild_sub_verify for %zu patterns with more than 16 concrete variants (entries=%zu, pairs=%d%s) fields=2-of-4 x 4 bases window=16 chunk=%lld nchunks=%d grid=%d block=%d",
             h->nwild, h->wd.max_entries, h->wd.ncombos, wild_long, (long long)h->geo.seg_len, h->geo.nseg, h->geo.blocks, h->geo.threads);
    if (h->nrest) {
      const size_t at = strlen(buf);
      if (at < buflen) snprintf(buf + at, buflen - at, " + %s for %zu patterns the seed plan does not take", bitpar_kernel_name(h->scan_k, h->scan_indels), h->nrest);
    }
  }
  else if (h->kern == PM_KERNEL_SEED && h->short_only)
    snprintf(buf, buflen, "kernel=pm_short_edit_scan+pm_edits_verify for %zu patterns of 16..19 characters (tiles=%d, tests=%d) fields=2-of-4 x 4 bases, displaced by |d| <= %d window=16 chunk=%lld nchunks=%d grid=%d block=%d",
             h->nshort, (int)h->shd.tiles.size(), h->shd.k == 2 ? SHORT_NTESTS : 2, h->shd.k, (long long)h->geo.seg_len, h->geo.nseg, h->geo.blocks, h->geo.threads);
  else if (h->kern == PM_KERNEL_SEED && !h->pair.empty()) {
    snprintf(buf, buflen, "kernel=pm_pair_scan tiles=%d combos=%d fields=2-of-4 x 5 bases window=20 row_slots=%d chunk=%lld nchunks=%d grid=%d block=%d lds=%d schedule=%s",
             (int)h->pair.size(), h->pair[0].ncombos, h->pair[0].stride, (long long)h->geo.seg_len, h->geo.nseg, h->geo.blocks, h->geo.threads, PAIR_LDS_BYTES,
             pair_schedule_name(h->geo));
    if (h->nlong) {
      int wide = 0;
      for (const PairDevice &d : h->pair) wide += d.wide ? 1 : 0;
      const size_t at = strlen(buf);
      if (at < buflen) snprintf(buf + at, buflen - at, " with %zu patterns of 33..64 characters (pm_pair_verify_wide, wide tiles=%d)", h->nlong, wide);
    }
    if (h->nrest) {
      const size_t at = strlen(buf);
      if (at < buflen) snprintf(buf + at, buflen - at, " + %s for %zu patterns the seed plan does not take", bitpar_kernel_name(h->scan_k, h->scan_indels), h->nrest);
    }
  }
  else if (h->kern == PM_KERNEL_SEED && h->edits_dev && h->epair_on) {
    // (-k 1: the two undisplaced tests of pm_pair_edit_scan_k1; exact_bases: pm_bases_verify reads the seed records)
    snprintf(buf, buflen, "kernel=pm_pair_edit_scan+pm_pair_edit_resolve+%s tiles=%d tests=%d fields=2-of-4 x 5 bases, displaced by |d| <= %d window=20 row_slots=%d slot_patterns=2 chunk=%lld nchunks=%d grid=%d block=%d lds=%d schedule=%s",
             h->bases_edits ? "pm_bases_verify" : "pm_edits_verify", (int)h->epair.size(), h->epair[0].k == 1 ? 2 : 14, h->epair[0].k == 1 ? 0 : 2, h->epair[0].stride, (long long)h->geo.seg_len, h->geo.nseg, h->geo.blocks, h->geo.threads, PAIR_LDS_BYTES, pair_schedule_name(h->geo));
    if (h->nlong_edits) {
      const size_t at = strlen(buf);
      int wide = h->sd.wide ? 1 : 0;
      for (const SeedDevice &d : h->sd_more) wide += d.wide ? 1 : 0;
      if (at < buflen) snprintf(buf + at, buflen - at, " with %zu patterns of 33..64 characters (pm_edits_verify_wide, wide tiles=%d)", h->nlong_edits, wide);
    }
    if (h->nrest) {
      const size_t at = strlen(buf);
      if (at < buflen) snprintf(buf + at, buflen - at, " + %s for %zu patterns the seed plan does not take", bitpar_kernel_name(h->scan_k, h->scan_indels), h->nrest);
    }
  }
  else if (h->kern == PM_KERNEL_SEED) {
    snprintf(buf, buflen, "kernel=%s tiles=%d combos=%d pieces=%d-of-%d x %d bases window=%d slots=%zu chunk=%lld nchunks=%d grid=%d block=%d lds=%d",
             h->sd.edits && h->sd.edit_tabulated ? "pm_edit_scan+pm_edits_verify" : h->sd.edits ? "pm_seed_scan+pm_edits_verify" :
             h->sd.halves && h->sd.half_ranked ? "pm_half_scan+pm_half_verify" : "pm_seed_scan", 1 + (int)h->sd_more.size(), h->sd.ncombos, h->sd.r, h->sd.k + h->sd.r, h->sd.pb, h->sd.Lw, h->sd.nslots, (long long)h->geo.seg_len, h->geo.nseg,
             h->geo.blocks, h->geo.threads, SEED_LDS_BYTES);
    if (h->nlong_exact) {
      int wide = h->sd.wide ? 1 : 0;
      for (const SeedDevice &d : h->sd_more) wide += d.wide ? 1 : 0;
      const size_t at = strlen(buf);
      if (at < buflen) snprintf(buf + at, buflen - at, " with %zu patterns of 33..64 characters (wide rows, wide tiles=%d)", h->nlong_exact, wide);
    }
    if (h->nlong_edits) {
      int wide = h->sd.wide ? 1 : 0;
      for (const SeedDevice &d : h->sd_more) wide += d.wide ? 1 : 0;
      const size_t at = strlen(buf);
      if (at < buflen) snprintf(buf + at, buflen - at, " with %zu patterns of 33..64 characters (pm_edits_verify_wide, wide tiles=%d)", h->nlong_edits, wide);
    }
    if (h->nlong_halves) {
      int wide = h->sd.wide ? 1 : 0;
      for (const SeedDevice &d : h->sd_more) wide += d.wide ? 1 : 0;
      const size_t at = strlen(buf);
      if (at < buflen) snprintf(buf + at, buflen - at, " with %zu patterns of 33..64 characters (pm_half_verify_wide, wide tiles=%d)", h->nlong_halves, wide);
    }
    if (h->nrest) {
      const size_t at = strlen(buf);
      if (at < buflen) snprintf(buf + at, buflen - at, " + %s for %zu patterns the seed plan does not take", bitpar_kernel_name(h->scan_k, h->scan_indels), h->nrest);
    }
  }
  if (h->kern == PM_KERNEL_SEED && h->nshort && !h->short_only) {
    const size_t at = strlen(buf);
    if (at < buflen) snprintf(buf + at, buflen - at, " + pm_short_edit_scan for %zu patterns of 16..19 characters (tiles=%d, tests=%d)", h->nshort, (int)h->shd.tiles.size(), h->shd.k == 2 ? SHORT_NTESTS : 2);
  }
  if (h->kern == PM_KERNEL_SEED && h->nssub) {
    const size_t at = strlen(buf);
    if (at < buflen) snprintf(buf + at, buflen - at, " + pm_short_sub_scan for %zu patterns of 16..19 characters (tiles=%d, pairs=%d)", h->nssub, (int)h->ssd.tiles.size(), h->ssd.ncombos);
  }
  if (h->kern == PM_KERNEL_SEED && h->nwild && !h->wild_only) {
    const size_t at = strlen(buf);
    if (at < buflen) snprintf(buf + at, buflen - at, " + pm_wild_sub_scan for %zu patterns with more than 16 concrete variants (entries=%zu, pairs=%d%s)", h->nwild, h->wd.max_entries, h->wd.ncombos, wild_long);
  }
  if (h->kern == PM_KERNEL_SEED) return PM_OK;
  else
    snprintf(buf, buflen, "kernel=%s tiles=%d lanes_per_tile=64 words_per_lane=%d seg_len=%lld nseg=%d grid=%d block=%d",
             bitpar_kernel_name(h->scan_k, h->scan_indels), h->bp.ntiles, BP_WPL, (long long)h->geo.seg_len, h->geo.nseg,
             h->geo.blocks, h->geo.threads);
  return PM_OK;
}

// ---- device stage ------------------------------------------------------------------------------
static int ensure_dp_tables(pm_handle *h);
static int ensure_fpat(pm_handle *h);

// The wild class into the record buffer of the scan being enqueued, behind the main class's kernels: its 8-byte suspects use
// the suspect list (which the main class's verify launches have read by then, stream order) under a counter of their own.
// own_counters: the main class runs no kernel that counts in d_seed_count, so the counters are this call's to zero and copy.
static int wild_scan(pm_handle *h, int64_t begin, int64_t end, bool own_counters) {
  const size_t want = (size_t)((end - begin) / 128) + ((size_t)1 << 20);
  if (!h->d_susp || h->susp_cap < want) {
    h->susp_cap = std::max(h->susp_cap, want);
    PM_TRY(dev_regrow(h, &h->d_susp, h->susp_cap * PAIR_SUSPECT_BYTES, "d_susp"));
  }
  if (!h->d_seed_count) HIP_TRY(h, hipMalloc((void **)&h->d_seed_count, SEEDCOUNT_WORDS * sizeof(unsigned long long)));
  if (own_counters) HIP_TRY(h, hipMemsetAsync(h->d_seed_count, 0, SEEDCOUNT_WORDS * sizeof(unsigned long long), h->stream));
  HIP_TRY(h, wild_launch(h->wd, h->d_text, h->d_packed, h->n, begin, end, h->d_cands, h->d_counter, h->cap, (uint64_t *)h->d_susp,
                         h->d_seed_count + WILD_COUNT_AT, h->susp_cap * (PAIR_SUSPECT_BYTES / sizeof(uint64_t)), h->stream, h->wild_only ? &h->geo : nullptr));
  h->last_launches += 2;
  if (own_counters) HIP_TRY(h, hipMemcpyAsync(h->h_seed_count, h->d_seed_count, SEEDCOUNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  return PM_OK;
}

extern "C" int pm_scan_candidates_async(pm_handle *h, int64_t begin, int64_t end) {
  if (!h || !h->inited) return fail(h, PM_E_INVALID, "pm_scan_candidates: handle not initialised");
  if (h->host_only) return fail(h, PM_E_INVALID, "pm_scan_candidates: this handle runs the host stage only (pm_init_host)");
  if (begin < 0 || end < begin) return fail(h, PM_E_INVALID, "pm_scan_candidates: bad range");
  if (end > h->n) end = h->n;
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  drain_spec(h);
  if (h->win) {                                                     // windowed handle: the range's text, its halo and what carried clusters need
    int64_t lo = begin - h->win_back;
    if (finalize_route(h) == Route::ClusterDp && !h->carry.empty()) lo = std::min(lo, carry_reach(h));
    const int rcw = win_need(h, lo, end + h->win_fwd, h->bound_on, "pm_scan_candidates");
    if (rcw) return rcw;
  }
  HIP_TRY(h, hipMemsetAsync(h->d_counter, 0, sizeof(unsigned long long), h->stream));
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  h->own_begin = begin; h->own_end = end;
  if (h->bases_edits) { int rcd = ensure_dp_tables(h); if (rcd) return rcd; }
  if (h->kern == PM_KERNEL_SEED && h->bases_edits) {                // a block seed comes from candidates up to maxlen + k away
    const int64_t reach = (int64_t)h->sd.maxlen + 2 * h->cfg.k + 4;
    begin = begin > reach ? begin - reach : 0;
    end = std::min<int64_t>(h->n, end + reach);
  }
  if (h->kern == PM_KERNEL_SEED && (h->edits_dev || (h->halves_dev && h->half_ranked_any)))
  {
    // per pattern tile: scan kernel -> seed records in d_ext, verify kernel -> candidates in d_cands
    // ~1 seed record per 8 bases at 200k patterns (key matches that pass the four-base-word test)
    // (sized for the range being scanned; a denser stream overflows once and the buffer grows)
    const size_t want_seeds = (size_t)((end - begin) / 6) + ((size_t)1 << 20);
    if (!h->d_seeds || h->seed_cap < want_seeds) {
      h->seed_cap = std::max(h->seed_cap, want_seeds);
      PM_TRY(dev_regrow(h, &h->d_seeds, h->seed_cap * sizeof(uint64_t), "d_seeds"));
    }
    if (!h->d_seed_count) HIP_TRY(h, hipMalloc((void **)&h->d_seed_count, SEEDCOUNT_WORDS * sizeof(unsigned long long)));
    const int ntiles = h->short_only ? 0 : 1 + (int)h->sd_more.size();
    if (ntiles > 256) return fail(h, PM_E_UNSUPPORTED, "too many pattern tiles for the edit-distance plan");
    HIP_TRY(h, hipMemsetAsync(h->d_seed_count, 0, SEEDCOUNT_WORDS * sizeof(unsigned long long), h->stream));
    for (int t = 0; t < ntiles; ++t) {
      EditStage es; es.d_seeds = h->d_seeds; es.d_seed_count = h->d_seed_count + 1 + t; es.seed_cap = h->seed_cap; es.tile = t;
      if (h->bases_edits) {
        es.bases = true; es.b_codes = h->d_dp_codes; es.b_len = h->d_fpat_len; es.b_esb = h->d_dp_esb; es.b_eeb = h->d_dp_eeb;
        es.own_lo = h->own_begin; es.own_hi = h->own_end;
      }
      const SeedDevice &d = t == 0 ? h->sd : h->sd_more[t - 1];
      if (h->epair_on && h->edits_dev) {
        // first stage on the pair geometry: windows whose frame can hold an end in (begin, end] are the positions begin - 3 .. end + 1
        // (every tile: its own tables and suspect counter; the suspect and seed lists are reused tile after tile in stream order)
        const size_t want_susp = (size_t)((end - begin) / 10) + ((size_t)1 << 20);
        if (!h->d_susp || h->susp_cap < want_susp) {
          h->susp_cap = std::max(h->susp_cap, want_susp);
          PM_TRY(dev_regrow(h, &h->d_susp, h->susp_cap * PAIR_SUSPECT_BYTES, "d_susp"));
        }
        HIP_TRY(h, pair_launch(h->epair[(size_t)t], h->d_text, h->d_packed, h->n, std::max<int64_t>(0, begin - 3), std::min<int64_t>(h->n, end + 2), h->d_cands, h->d_counter, h->cap,
                               h->d_susp, h->d_seed_count + EPAIR_COUNT_AT + t, h->susp_cap, h->stream, t == 0 ? &h->geo : nullptr, nullptr, 3, h->d_seeds, h->d_seed_count + 1 + t, h->seed_cap));
        es.skip_scan = true;
      }
      HIP_TRY(h, seed_launch(d, h->d_text, h->d_packed, h->n, begin, end, h->d_cands, h->d_counter, h->cap, h->stream, t == 0 && !es.skip_scan ? &h->geo : nullptr, &es));
    }
    h->last_launches = (h->epair_on && h->edits_dev ? 3 : 2) * ntiles;
    if (h->nshort) {
      // the short class into the same record buffer; its seed records reuse the seed list, which the main class's automaton
      // launch has read by then (stream order), under a counter of their own
      HIP_TRY(h, short_launch(h->shd, h->d_text, h->d_packed, h->n, begin, end, h->d_cands, h->d_counter, h->cap, h->d_seeds, h->d_seed_count + SHORT_COUNT_AT,
                              h->seed_cap, h->stream, h->short_only ? &h->geo : nullptr));
      h->last_launches += (int)h->shd.tiles.size() + 1;
    }
    HIP_TRY(h, hipMemcpyAsync(h->h_seed_count, h->d_seed_count, SEEDCOUNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    if (h->nrest) { HIP_TRY(h, bitpar_launch(h->bp, h->d_text, h->n, begin, end, h->d_cands, h->d_counter, h->cap, h->stream, nullptr)); ++h->last_launches; }
  }
  else if (h->kern == PM_KERNEL_SEED && !h->pair.empty())
  {
    // suspects (windows within k of a pattern on the packed bases, before the exact check): a few per
    // thousand positions on random streams; a denser stream overflows once and the buffer grows
    // (+ up to 15 unused slots per wave of the scan grid: slots are reserved 16 at a time)
    const size_t want = (size_t)((end - begin) / 128) + (size_t)((end - begin) / 8192) * h->pair[0].ncombos + ((size_t)1 << 20);
    if (!h->d_susp || h->susp_cap < want) {
      h->susp_cap = std::max(h->susp_cap, want);
      PM_TRY(dev_regrow(h, &h->d_susp, h->susp_cap * PAIR_SUSPECT_BYTES, "d_susp"));
    }
    if (!h->d_seed_count) HIP_TRY(h, hipMalloc((void **)&h->d_seed_count, SEEDCOUNT_WORDS * sizeof(unsigned long long)));
    if (h->pair.size() > 256) return fail(h, PM_E_UNSUPPORTED, "too many pattern tiles");
    HIP_TRY(h, hipMemsetAsync(h->d_seed_count, 0, SEEDCOUNT_WORDS * sizeof(unsigned long long), h->stream));
    for (size_t t = 0; t < h->pair.size(); ++t)
      HIP_TRY(h, pair_launch(h->pair[t], h->d_text, h->d_packed, h->n, begin, end, h->d_cands, h->d_counter, h->cap,
                             h->d_susp, h->d_seed_count + 1 + t, h->susp_cap, h->stream, t == 0 ? &h->geo : nullptr, h->d_seed_count + 257));
    h->last_launches = 2 * (int)h->pair.size();
    if (h->nssub) {
      // the class of 16..19 characters into the same record buffer; its 8-byte suspects reuse the suspect list, which the
      // main class's verify launches have read by then (stream order), under a counter of their own
      HIP_TRY(h, short_sub_launch(h->ssd, h->d_text, h->d_packed, h->n, begin, end, h->d_cands, h->d_counter, h->cap, (uint64_t *)h->d_susp,
                                  h->d_seed_count + SHORT_COUNT_AT, h->susp_cap * (PAIR_SUSPECT_BYTES / sizeof(uint64_t)), h->stream));
      h->last_launches += (int)h->ssd.tiles.size() + 1;
    }
    if (h->nwild) PM_TRY(wild_scan(h, begin, end, false));
    HIP_TRY(h, hipMemcpyAsync(h->h_seed_count, h->d_seed_count, SEEDCOUNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    if (h->nrest) { HIP_TRY(h, bitpar_launch(h->bp, h->d_text, h->n, begin, end, h->d_cands, h->d_counter, h->cap, h->stream, nullptr)); ++h->last_launches; }
  }
  else if (h->kern == PM_KERNEL_SEED)
  {
    if (!h->wild_only) HIP_TRY(h, seed_launch(h->sd, h->d_text, h->d_packed, h->n, begin, end, h->d_cands, h->d_counter, h->cap, h->stream, &h->geo));
    for (SeedDevice &d : h->sd_more)
      HIP_TRY(h, seed_launch(d, h->d_text, h->d_packed, h->n, begin, end, h->d_cands, h->d_counter, h->cap, h->stream, nullptr));
    h->last_launches = h->wild_only ? 0 : 1 + (int)h->sd_more.size();
    if (h->nwild) PM_TRY(wild_scan(h, begin, end, true));
    if (h->nrest) { HIP_TRY(h, bitpar_launch(h->bp, h->d_text, h->n, begin, end, h->d_cands, h->d_counter, h->cap, h->stream, nullptr)); ++h->last_launches; }
  }
  else
    HIP_TRY(h, bitpar_launch(h->bp, h->d_text, h->n, begin, end, h->d_cands, h->d_counter, h->cap, h->stream, &h->geo));
  h->scan_begin = begin; h->scan_end = end;
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->h_counter, h->d_counter, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  if (h->kern != PM_KERNEL_SEED) h->last_launches = 1;
  h->scan_pending = true;
  if (h->win && h->bound_on) win_prefetch(h, h->own_end, h->own_end - h->own_begin);   // (the upload overlaps this scan)
  return PM_OK;
}


// sort workspace shared by pm_finalize_device (clustering) and the edit-distance dedup
static int ensure_sort_workspace(pm_handle *h, size_t n, bool with_out) {
  if (h->ckeys_cap < n || !h->d_keys) {
    void *fw[] = {h->d_keys, h->d_keys_alt, h->d_ctemp, h->d_fout, h->d_fleft};
    for (void *q : fw) if (q) (void)hipFree(q);
    h->d_keys = h->d_keys_alt = nullptr; h->d_ctemp = nullptr; h->d_fout = h->d_fleft = nullptr;
    h->ckeys_cap = std::max<size_t>(n + n / 4, (size_t)1 << 16);
    HIP_TRY(h, hipMalloc((void **)&h->d_keys, h->ckeys_cap * 8));
    HIP_TRY(h, hipMalloc((void **)&h->d_keys_alt, h->ckeys_cap * 8));
    h->ctemp_bytes = cluster_temp_bytes(h->ckeys_cap);
    HIP_TRY(h, hipMalloc(&h->d_ctemp, h->ctemp_bytes ? h->ctemp_bytes : 16));
  }
  if (with_out && !h->d_fout) {
    HIP_TRY(h, hipMalloc((void **)&h->d_fout, h->ckeys_cap * sizeof(pm_hit)));
    HIP_TRY(h, hipMalloc((void **)&h->d_fleft, h->ckeys_cap * sizeof(pm_hit)));
  }
  if (!h->d_fcounts) {
    HIP_TRY(h, hipMalloc((void **)&h->d_fcounts, 4 * sizeof(unsigned long long)));
    HIP_TRY(h, hipHostMalloc((void **)&h->h_fcounts, 4 * sizeof(unsigned long long), hipHostMallocDefault));
  }
  return PM_OK;
}

// ---- records the host adds at the stream's edges (EdgeRule) --------------------------------------
// Every rule below builds its records once per init and hands out the ones that end in the caller's range
// (own_begin, own_end] -- whatever range holds the end gets the record: a first or last range may be shorter than a
// pattern; scan_wait_once puts them behind the kernels' records (append_host_records).
static void edge_owned(const pm_handle *h, const EdgeRecords &e, std::vector<pm_hit> *out) {
  for (const pm_hit &x : e.recs) if (x.end > h->own_begin && x.end <= h->own_end) out->push_back(x);
}

// inner pattern j belongs to the seed family's main class, whose edge records the host makes
static bool in_main_class(const pm_handle *h, size_t j) {
  if (j < h->in_rest.size() && h->in_rest[j]) return false;         // the residue engine reports its own
  if (j < h->in_short.size() && h->in_short[j]) return false;       // and so does pm_short_edit_scan
  return true;
}

// `extra` behind the records of the scan in HBM.  A buffer too small for both: PM_E_OVERFLOW, and *n_out is the record
// count it must hold.
static int append_host_records(pm_handle *h, const std::vector<pm_hit> &extra, size_t *n_out) {
  const size_t tot = h->last_count + extra.size();
  if (n_out) *n_out = tot;
  if (tot > h->cap) { h->last_count = 0; return fail(h, PM_E_OVERFLOW, "candidate buffer too small (pm_set_capacity)"); }
  if (!extra.empty()) HIP_TRY(h, hipMemcpy(h->d_cands + h->last_count, extra.data(), extra.size() * sizeof(pm_hit), hipMemcpyHostToDevice));
  h->last_count = tot;
  return PM_OK;
}

// The k-error automaton itself (shift_and_inexact.cc:249-352) for inner pattern j over the stream characters
// text[0, T), text[0] being stream position `base`: its ends beyond keep_after go to *out.  At the start of the stream the
// rows start with l prefix bits (:162-164), elsewhere from the empty state.
static void edit_automaton_ends(const pm_handle *h, size_t j, const uint8_t *text, int64_t T, int64_t base, int64_t keep_after, std::vector<pm_hit> *out) {
  const int k = h->cfg.k;
  const std::string &s = h->inner[j].s;
  const int L = (int)s.size();
  uint64_t R[3] = {0, 0, 0};
  if (base == 0) { R[1] = 1; R[2] = 3; }
  const uint64_t last = 1ull << (L - 1);
  uint64_t M[4] = {0, 0, 0, 0};                       // positions of A, C, G, T (the only pattern characters of the seed family)
  int code[4];
  for (int q = 0; q < 4; ++q) code[q] = h->alpha.nch[(unsigned char)"ACGT"[q]];
  for (int i = 0; i < L; ++i) for (int q = 0; q < 4; ++q)
    if (h->wild_seed ? acgt_of((unsigned char)s[i]).find("ACGT"[q]) != std::string::npos : s[i] == "ACGT"[q]) M[q] |= 1ull << i;
  for (int64_t t = 0; t < T; ++t) {
    const int c = text[t];
    if (c == h->eos_code) { R[0] = R[1] = R[2] = 0; continue; }
    const uint64_t U = c == code[0] ? M[0] : c == code[1] ? M[1] : c == code[2] ? M[2] : c == code[3] ? M[3] : 0;
    const uint64_t x0 = (R[0] << 1) | 1, m1 = x0 | R[0], n0 = x0 & U;
    const uint64_t x1 = (R[1] << 1) | 1, n1 = (x1 & U) | m1 | (n0 << 1) | 1 | n0, m2 = x1 | R[1];
    const uint64_t x2 = (R[2] << 1) | 1, n2 = (x2 & U) | m2 | (n1 << 1) | 1 | n1;
    R[0] = n0; R[1] = n1; R[2] = n2;
    const int lvl = (R[0] & last) ? 0 : (R[1] & last) ? 1 : (k >= 2 && (R[2] & last)) ? 2 : -1;
    const int64_t end = base + t + 1;
    if (lvl >= 0 && end > keep_after) {
      pm_hit x; x.end = end; x.pid = h->inner_ids[j]; x.k = (uint8_t)lvl; x.aux[0] = x.aux[1] = x.aux[2] = 0;
      out->push_back(x);
    }
  }
}

// Edit-distance seed plan: windows that do not fit in front of the stream start are not seeded, so
// every candidate that ends in the first Lw+2k+2 characters is produced here by running the
// automaton itself (edit_automaton_ends) for each pattern over those few characters; the kernel's
// records for the same ends are duplicates and leave with the dedup.  Whatever range holds such an
// end gets them -- a caller's first range may be shorter than that
// (found by scripts/fuzz_families.py --dense-bound, seed 605103, at the other end of the stream).
static int edits_start_candidates(pm_handle *h, std::vector<pm_hit> *out) {
  const int64_t T = std::min<int64_t>(h->n, h->sd.Lw + 2 * h->cfg.k + 2);
  if (T <= 0 || h->own_begin >= T) return PM_OK;
  EdgeRecords &e = h->edge[EDGE_EDITS_START];
  if (!e.built) {                                                   // same stream, same patterns: computed once
    uint8_t head[64] = {0};
    { const int rc = host_codes(h, 0, T, head); if (rc) return rc; }
    for (size_t j = 0; j < h->inner.size(); ++j)
      if (in_main_class(h, j)) edit_automaton_ends(h, j, head, T, 0, 0, &e.recs);
    e.built = true;
  }
  edge_owned(h, e, out);
  return PM_OK;
}

// Edit-distance seed plan, the other end: a match whose clean pieces are followed by deleted pattern characters is
// seeded by the window one or two positions BEHIND its end (the seed's place is where the pattern's last base
// would be), and behind the last character of the stream there are no windows.  The candidates that end in the
// last four characters are therefore produced here as well: the automaton from the empty state over the last
// L + k + 8 characters -- its last bit depends on the last L + k only -- (from the stream-start state when that
// is the whole stream); duplicates of the kernel's records leave with the dedup.  Computed once per stream.
// Found by scripts/fuzz_families.py (seed 1308).
static int edge_reach(const pm_handle *h) { return h->nlong || h->nlong_exact || h->nlong_edits || h->nlong_halves || h->nwild_long ? 64 : 32; }   // (the wild class's primers are main-class primers to the host's edge records)
static int edits_end_candidates(pm_handle *h, std::vector<pm_hit> *out) {
  const int k = h->cfg.k;
  const int64_t n = h->n;
  if (h->own_end <= n - 4 || n <= 0) return PM_OK;                  // (the range that holds such an end gets it: the last range may be shorter than four positions)
  EdgeRecords &e = h->edge[EDGE_EDITS_END];
  if (!e.built) {
    const int64_t T = std::min<int64_t>(n, edge_reach(h) + k + 8);  // (the main class's longest pattern + k + 8: at most 74)
    uint8_t tail[80] = {0};
    { const int rc = host_codes(h, n - T, T, tail); if (rc) return rc; }
    for (size_t j = 0; j < h->inner.size(); ++j) {
      if (!in_main_class(h, j)) continue;
      const int64_t Tj = std::min<int64_t>(T, (int64_t)h->inner[j].s.size() + k + 8);
      edit_automaton_ends(h, j, tail + (T - Tj), Tj, n - Tj, n - 4, &e.recs);
    }
    e.built = true;
  }
  edge_owned(h, e, out);
  return PM_OK;
}

// The k-error automaton starts with the first l bits of every pattern set in row l
// (shift_and_inexact.cc:162-164), so at the very start of the stream a pattern whose first
// d <= k characters are "missing" is reported at end = L-d with level d + mismatches.  The seed
// kernel only sees whole windows; these few records are produced here and appended in HBM.
// The longest pattern of the main class (edge_reach: 32, 64 with long primers on the pair plan, at k = 0 on the Bloom
// plan or under -k on the edit plan) sizes the piece of the stream read; nothing else here depends on the length.
static int stream_start_candidates(pm_handle *h, std::vector<pm_hit> *out) {
  const int k = h->seed_k;
  EdgeRecords &e = h->edge[EDGE_STREAM_START];
  if (!e.built) {                                                   // same stream, same patterns: computed once (0.3 ms per scan at 200k patterns)
    const int64_t need = std::min<int64_t>(h->n, edge_reach(h));
    uint8_t head[64] = {0};
    { const int rc = host_codes(h, 0, need, head); if (rc) return rc; }
    for (size_t j = 0; j < h->inner.size(); ++j) {
      if (!in_main_class(h, j)) continue;
      const std::string &s = h->inner[j].s;
      const int L = (int)s.size();
      for (int d = 1; d <= k && d < L; ++d) {
        const int end = L - d;
        if (end > h->n) continue;
        int lvl = d;
        bool dead = false;
        for (int i = 0; i < end && !dead; ++i) {
          if ((int)head[i] == h->eos_code) dead = true;              // EOS clears every row
          else if (h->wild_seed) { if (acgt_of((unsigned char)s[d + i]).find((char)h->alpha.ch[head[i]]) == std::string::npos) ++lvl; }
          else if ((int)head[i] != h->alpha.nch[(unsigned char)s[d + i]]) ++lvl;
        }
        if (!dead && lvl <= k) {
          pm_hit x; x.end = end; x.pid = h->inner_ids[j]; x.k = (uint8_t)lvl; x.aux[0] = x.aux[1] = x.aux[2] = 0;
          e.recs.push_back(x);
        }
      }
    }
    e.built = true;
  }
  edge_owned(h, e, out);
  return PM_OK;
}

// exact_halves reads past the end of the stream: a left half found as an exact seed right at the end is
// extended by primer_alignment_lmatch over len2 + k characters from the seed on (primer_alignment.cc:573-574)
// whether or not the stream still has them, and what char_io hands out there is the zero padding of the
// mapped file's last page (mapFile.h:49-57) -- code 0, the table's first character on a normalized stream.
// So a pattern hangs over the end by t <= len2 characters when its first L - t characters are the stream's
// last ones (left half exact, the rest within k substitutions, none in an exact zone) and its last t
// characters against code 0 keep the total within k: hit at end n + t.  The whole-pattern windows of the
// seed kernels end inside the stream; these few records (flag 1: found through the left seed) are made here
// and appended in HBM, like the records of the stream start.  With indels the half seeds are extended by
// pm_seed_extend, which reads code 0 past the end itself.  exact_bases -K is the same with the mandated first
// block in the left half's place (its records are final: the primer's id, no flag).
// (All of them end beyond the stream: they go to the range that reaches its end, own_end >= n.)
// `reach` = edge_reach: the characters of the stream's end that are looked at, as many as the longest pattern has (a
// pattern of 64 hangs over by up to len2 = 32); nothing else here depends on the length.
static int stream_end_overhang_candidates(pm_handle *h, bool bases, std::vector<pm_hit> *out) {
  const int k = h->cfg.k;
  const int64_t n = h->n;
  EdgeRecords &e = h->edge[EDGE_OVERHANG];
  if (!e.built) {                                                   // same stream, same patterns: computed once
    const int reach = edge_reach(h);
    const int64_t need = std::min<int64_t>(n, reach);
    uint8_t tail[64] = {0};                                         // tail[reach - need .. reach) = the last `need` characters
    { const int rc = host_codes(h, n - need, need, tail + reach - need); if (rc) return rc; }
    auto differs = [&](unsigned char pc, int code) -> bool {
      if (h->cfg.wildcards) return acgt_of(pc).find((char)h->alpha.ch[code]) == std::string::npos;
      return code != h->alpha.nch[pc];
    };
    if (h->eos_code != 0) {                                         // (code 0 = EOS: the extension's first character past the end is a violation)
      for (size_t j = 0; j < h->pats.size(); ++j) {
        const Pattern &p = h->pats[j];
        const int L = (int)p.s.size();
        const int es = std::max(0, std::min(L, p.esb)), ee = std::max(0, std::min(L, p.eeb));
        // the part found as an exact seed inside the stream: the left half (exact_halves), the mandated first block
        // (exact_bases with esb >= eeb, exact_bases.cc:139-150; a last block lies on the stream with all of its pattern)
        if (bases && (es < ee || es == 0)) continue;
        const int len1 = bases ? es : L / 2, len2 = L - len1;
        for (int t = 1; t <= len2; ++t) {
          const int inside = L - t;                                 // pattern characters 0 .. inside-1 lie on the stream's last ones
          if (inside > need) continue;                              // (more of the pattern than the stream holds: a larger overhang may still fit)
          int lvl = 0;
          bool dead = false;
          for (int i = 0; i < L && !dead; ++i) {
            const int code = i < inside ? (int)tail[reach - inside + i] : 0;
            if (i < inside && code == h->eos_code) dead = true;
            else if (differs((unsigned char)p.s[i], code)) {
              if (i < len1 || i < es || i >= L - ee) dead = true;   // the seed part is exact; a substitution in an exact zone is a violation
              else ++lvl;
            }
          }
          if (!dead && lvl <= k) {
            pm_hit x; x.end = n + t; x.pid = bases ? (uint32_t)p.id : (uint32_t)(j + 1); x.k = (uint8_t)lvl; x.aux[0] = bases ? 0 : 1; x.aux[1] = x.aux[2] = 0;
            e.recs.push_back(x);
          }
        }
      }
    }
    e.built = true;
  }
  out->insert(out->end(), e.recs.begin(), e.recs.end());
  return PM_OK;
}

// exact_bases -k: the records are occurrences of the mandated block, found through windows within k edits of
// the whole pattern.  A pattern that hangs over the end of the stream has no such window (the extension DP reads
// code 0 there, see stream_end_overhang_candidates), and at the start of the stream the windows that do not
// fit are not seeded (a pattern whose first characters are deleted there ends in them).  Every block occurrence
// in the first and last 56 characters therefore comes from the host as well -- more than needed: the
// reference extends EVERY occurrence, the records are verified by the same DP, duplicates leave with the dedup.
static int bases_edge_candidates(pm_handle *h, std::vector<pm_hit> *out) {
  const int64_t n = h->n, E = std::min<int64_t>(n, 56);
  if (h->own_begin >= 56 && h->own_end <= n - 56) return PM_OK;
  EdgeRecords &e = h->edge[EDGE_BLOCKS];
  if (!e.built) {                                                   // same stream, same patterns: computed once
    uint8_t edge[2][64] = {{0}, {0}};
    { int rc = host_codes(h, 0, E, edge[0]); if (!rc) rc = host_codes(h, n - E, E, edge[1]); if (rc) return rc; }
    for (size_t j = 0; j < h->pats.size(); ++j) {
      const Pattern &p = h->pats[j];
      const int L = (int)p.s.size();
      const int es = std::max(0, std::min(L, p.esb)), ee = std::max(0, std::min(L, p.eeb));
      const bool prefix = es >= ee;                                 // exact_bases.cc:139-150: the larger block decides
      const int blk = prefix ? es : ee;
      if (blk <= 0) continue;
      const char *bs = p.s.data() + (prefix ? 0 : L - blk);
      for (int side = 0; side < 2; ++side) {
        const int64_t base = side == 0 ? 0 : n - E;                 // stream index of edge[side][0]
        for (int64_t o = 0; o + blk <= E; ++o) {
          if (side == 1 && base + o + blk <= E) continue;           // (a short stream: already taken from its start)
          bool ok = true;
          for (int q = 0; q < blk && ok; ++q) ok = (int)edge[side][o + q] == h->alpha.nch[(unsigned char)bs[q]];
          if (ok) { pm_hit x; x.end = base + o + blk; x.pid = (uint32_t)(j + 1); x.k = 0; x.aux[0] = x.aux[1] = x.aux[2] = 0; e.recs.push_back(x); }
        }
      }
    }
    e.built = true;
  }
  edge_owned(h, e, out);
  return PM_OK;
}

// per pattern (index = position in the pattern list): 32 stream codes, length, exact zones -- what the
// device-side DPs (pm_cluster_dp) and pm_bases_seeds read.  With long primers on the edit plan (nlong_edits) the rows hold
// 64 codes: dp_row is the stride, and pm_cluster_dp<64> the one reader (cluster_dp_device's `wide`).
static size_t dp_row(const pm_handle *h) { return h->nlong_edits ? 64 : 32; }
static int ensure_dp_tables(pm_handle *h) {
  const size_t np = h->pats.size(), row = dp_row(h);
  if (!h->d_dp_codes) {
    std::vector<uint8_t> codes(np * row, 0);
    std::vector<int32_t> es(np), ee(np);
    for (size_t i = 0; i < np; ++i) {
      for (size_t q = 0; q < h->pats[i].s.size() && q < row; ++q) codes[i * row + q] = (uint8_t)h->alpha.nch[(unsigned char)h->pats[i].s[q]];
      es[i] = h->pats[i].esb; ee[i] = h->pats[i].eeb;
    }
    PM_TRY(dev_upload(h, &h->d_dp_codes, codes, 32, "d_dp_codes"));
    PM_TRY(dev_upload(h, &h->d_dp_esb, es, 4, "d_dp_esb"));
    PM_TRY(dev_upload(h, &h->d_dp_eeb, ee, 4, "d_dp_eeb"));
  }
  return ensure_fpat(h);
}

// An internal buffer between two kernels of one scan (seed records, suspects) was too small: it has
// been enlarged and the same range must be scanned again.  That is the library's own business --
// pm_scan_wait does it -- and never reaches the caller, whose record buffer (pm_set_capacity) was
// not the problem and must not be reallocated for it.
static const int SCAN_AGAIN = 1000;

// Records one list of a scan may hold before pm_scan cuts the range in two instead of growing it (candidates 16 B, suspects
// 16 B, seed records 8 B, and the finalize stage's sort workspace of ~70 B per candidate): 2^30 by default, PM_DENSE_BOUND
// for tests.  Always below the 2^31 items the device sorts count in an int.
static size_t dense_bound(const pm_handle *h) {
  const long long v = h->knobs.dense_bound;
  return v > 0 ? (size_t)std::min<long long>(v, (1ll << 31) - 1) : (size_t)1 << 30;
}
static int dense_fail(pm_handle *h, const char *what, unsigned long long n) {
  h->too_dense = true;
  h->last_count = 0;
  return fail(h, PM_E_UNSUPPORTED, std::string(what) + ": " + std::to_string(n) + " records in one range -- scan the stream in smaller ranges");
}

// Waiting for the handle's stream.  (Polling hipStreamQuery instead of hipStreamSynchronize measured no difference
// around the 15 ms scan kernels: 15.47 against 15.49 ms per step.)
static hipError_t stream_wait(pm_handle *h) { return hipStreamSynchronize(h->stream); }

static int scan_wait_once(pm_handle *h, size_t *n_out) {
  HIP_TRY(h, stream_wait(h));
  h->scan_pending = false;
  (void)hipEventElapsedTime(&h->last_ms, h->ev0, h->ev1);
  const size_t cnt = (size_t)*h->h_counter;
  if (n_out) *n_out = cnt;
  h->last_peak = cnt;
  if (h->h_seed_count && h->kern == PM_KERNEL_SEED && (h->edits_dev || (h->halves_dev && h->half_ranked_any) || !h->pair.empty())) {
    const size_t tiles = !h->pair.empty() ? h->pair.size() : 1 + h->sd_more.size();
    for (size_t t = 0; t < tiles && t < 256; ++t) h->last_peak = std::max(h->last_peak, h->h_seed_count[1 + t]);
    for (size_t t = 0; t < h->epair.size() && t < 256; ++t) h->last_peak = std::max(h->last_peak, h->h_seed_count[EPAIR_COUNT_AT + t]);
    if (h->nshort || h->nssub) h->last_peak = std::max(h->last_peak, h->h_seed_count[SHORT_COUNT_AT]);
  }
  if (h->bound_on && cnt > dense_bound(h)) return dense_fail(h, "candidate records", cnt);
  if (cnt > h->cap) { h->last_count = 0; return fail(h, PM_E_OVERFLOW, "candidate buffer too small (pm_set_capacity)"); }
  h->last_count = cnt;
  if (h->edits_dev || (h->halves_dev && h->half_ranked_any)) {
    // the seed buffer of a tile must have held all its seed records
    unsigned long long worst = 0;
    for (int t = 0; t < 1 + (int)h->sd_more.size(); ++t) worst = std::max(worst, h->h_seed_count[1 + t]);
    if (h->nshort) worst = std::max(worst, h->h_seed_count[SHORT_COUNT_AT]);
    if (h->knobs.debug) fprintf(stderr, "[pm] %s: %llu seed records (tile with most), seed cap %zu, candidates %zu\n", h->edits_dev ? "edits" : "halves", worst, h->seed_cap, cnt);
    if (h->bound_on && worst > dense_bound(h)) return dense_fail(h, "seed records of the edit-distance plan", worst);
    if (worst > h->seed_cap) {                                     // grow the seed buffer and tell the caller to scan again
      h->seed_cap = (size_t)worst + (size_t)worst / 8 + 1024;
      h->last_count = 0;
      PM_TRY(dev_regrow(h, &h->d_seeds, h->seed_cap * sizeof(uint64_t), "d_seeds"));
      return SCAN_AGAIN;
    }
    unsigned long long worst_susp = 0;                             // the pair geometry's suspect list between its two kernels: the tile with most
    if (h->epair_on && h->edits_dev) for (size_t t = 0; t < h->epair.size() && t < 256; ++t) worst_susp = std::max(worst_susp, h->h_seed_count[EPAIR_COUNT_AT + t]);
    h->last_suspects = worst_susp;
    if (h->bound_on && worst_susp > dense_bound(h))
      return dense_fail(h, "suspects of the edit-distance plan", worst_susp);
    if (worst_susp > h->susp_cap) {
      h->susp_cap = (size_t)worst_susp + (size_t)worst_susp / 8 + 1024;
      h->last_count = 0;
      PM_TRY(dev_regrow(h, &h->d_susp, h->susp_cap * PAIR_SUSPECT_BYTES, "d_susp"));
      return SCAN_AGAIN;
    }
  }
  if (h->halves_dev) {
    // second device pass: banded DP next to every surviving seed (pm_extend.hip); the records
    // handed on are the successful extensions
    if (!h->d_ext) HIP_TRY(h, hipMalloc((void **)&h->d_ext, h->cap * sizeof(pm_hit)));
    HIP_TRY(h, extend_seeds(h->d_text, h->n, h->d_cands, cnt, h->d_half_codes, h->d_half_len, h->d_hesb, h->d_heeb,
                            h->cfg.k, h->eos_code, h->d_ext, h->d_counter, h->cap, h->stream, (int)half_row(h)));
    HIP_TRY(h, hipMemcpyAsync(h->h_counter, h->d_counter, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, stream_wait(h));
    std::swap(h->d_cands, h->d_ext);
    h->last_count = (size_t)*h->h_counter;
    if (n_out) *n_out = h->last_count;
    h->last_launches += 1;
  }
  if (h->kern == PM_KERNEL_SEED && !h->pair.empty()) {
    // the suspect buffer must have held every tile's suspects
    unsigned long long worst = 0;
    for (size_t t = 0; t < h->pair.size(); ++t) worst = std::max(worst, h->h_seed_count[1 + t]);
    if (h->nssub) worst = std::max(worst, (h->h_seed_count[SHORT_COUNT_AT] + 1) / 2);   // (8-byte suspects in the 16-byte slots)
    if (h->knobs.debug) fprintf(stderr, "[pm] pair plan: %llu suspects (tile with most), capacity %zu, candidates %zu\n", worst, h->susp_cap, cnt);
    if (h->bound_on && worst > dense_bound(h)) return dense_fail(h, "suspects of the pair plan", worst);
    if (worst > h->susp_cap) {                                     // grow it and tell the caller to scan again
      h->susp_cap = (size_t)worst + (size_t)worst / 8 + 1024;
      h->last_count = 0;
      PM_TRY(dev_regrow(h, &h->d_susp, h->susp_cap * PAIR_SUSPECT_BYTES, "d_susp"));
      return SCAN_AGAIN;
    }
  }
  if (h->kern == PM_KERNEL_SEED && h->nwild) {
    // the suspect buffer must have held the wild class's suspects (8-byte suspects in the 16-byte slots)
    const unsigned long long worst = (h->h_seed_count[WILD_COUNT_AT] + 1) / 2;
    h->last_peak = std::max(h->last_peak, h->h_seed_count[WILD_COUNT_AT]);
    if (h->knobs.debug) fprintf(stderr, "[pm] wild class: %llu suspects, capacity %zu, candidates %zu\n", h->h_seed_count[WILD_COUNT_AT], 2 * h->susp_cap, cnt);
    if (h->bound_on && worst > dense_bound(h)) return dense_fail(h, "suspects of the wild class", worst);
    if (worst > h->susp_cap) {                                     // grow it and tell the caller to scan again
      h->susp_cap = (size_t)worst + (size_t)worst / 8 + 1024;
      h->last_count = 0;
      PM_TRY(dev_regrow(h, &h->d_susp, h->susp_cap * PAIR_SUSPECT_BYTES, "d_susp"));
      return SCAN_AGAIN;
    }
  }
  if (h->edits_dev) {
    // records of the stream's edges (host), then sort + unique on the device: several seeds report each candidate
    std::vector<pm_hit> extra;
    int rc;
    if (h->bases_edits) rc = bases_edge_candidates(h, &extra);      // (exact_bases: the records are block seeds, not automaton ends)
    else {
      rc = edits_start_candidates(h, &extra);
      if (!rc) rc = edits_end_candidates(h, &extra);
    }
    if (!rc) rc = append_host_records(h, extra, n_out);
    if (rc) return rc;
    const size_t tot = h->last_count;
    if (tot >= ((size_t)1 << 31)) return dense_fail(h, "edit-distance plan, 2^31 or more candidate", tot);
    rc = ensure_sort_workspace(h, tot, false);
    if (rc) return rc;
    const double td0 = now_ms();
    HIP_TRY(h, dedup_device(h->d_cands, tot, h->d_keys, h->d_keys_alt, h->d_ctemp, h->ctemp_bytes, h->d_cands, h->d_fcounts, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->h_fcounts, h->d_fcounts, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, stream_wait(h));
    h->last_count = (size_t)h->h_fcounts[0];
    if (h->knobs.debug) fprintf(stderr, "[pm] edits: %zu raw records (with holes) -> %zu unique candidates, dedup %.1f ms\n", tot, h->last_count, now_ms() - td0);
    if (n_out) *n_out = h->last_count;
    h->last_launches += 3;
    return PM_OK;
  }
  std::vector<pm_hit> extra;
  if (h->kern == PM_KERNEL_SEED && h->own_begin < edge_reach(h) && h->seed_k > 0 &&
      (h->sem == PM_SEM_FILTER_BITVEC || h->sem == PM_SEM_SHIFT_AND_INEXACT)) {
    const int rc = stream_start_candidates(h, &extra);
    if (rc) return rc;
  }
  if (h->kern == PM_KERNEL_SEED && (h->seed_flags || h->bases_flags) && h->own_end >= h->n) {
    const int rc = stream_end_overhang_candidates(h, h->bases_flags, &extra);
    if (rc) return rc;
  }
  return extra.empty() ? PM_OK : append_host_records(h, extra, n_out);
}

extern "C" int pm_scan_wait(pm_handle *h, size_t *n_out) {
  if (!h || !h->scan_pending) return fail(h, PM_E_INVALID, "pm_scan_wait: no scan in flight");
  float spent_ms = 0.f;                                             // kernel time of the attempts that had to be repeated
  for (int tries = 0;; ++tries) {
    const int rc = scan_wait_once(h, n_out);
    if (rc != SCAN_AGAIN) { h->last_ms += spent_ms; return rc; }
    spent_ms += h->last_ms;
    ++h->internal_rescans;
    if (tries >= 8) return fail(h, PM_E_NOMEM, "pm_scan_wait: the scan's internal record buffers keep overflowing");
    const int ra = pm_scan_candidates_async(h, h->own_begin, h->own_end);   // the caller's range, with the enlarged buffer
    if (ra) return ra;
  }
}

// The scan pm_scan enqueued for the range it expected next, and nobody asked for after all (another range, pm_reset,
// a direct scan or finalize call, pm_destroy): let it finish and forget it.
static void drain_spec(pm_handle *h) {
  if (!h->spec) return;
  h->spec = false;
  if (h->scan_pending) { (void)hipStreamSynchronize(h->stream); h->scan_pending = false; }
  h->last_count = 0;
}

extern "C" int pm_scan_candidates(pm_handle *h, int64_t begin, int64_t end, pm_hit *out, size_t cap, size_t *n_out) {
  int rc = pm_scan_candidates_async(h, begin, end);
  if (rc) return rc;
  size_t cnt = 0;
  rc = pm_scan_wait(h, &cnt);
  if (n_out) *n_out = cnt;
  if (rc) return rc;
  if (out) {
    if (cnt > cap) return fail(h, PM_E_OVERFLOW, "pm_scan_candidates: out buffer too small");
    if (cnt) HIP_TRY(h, hipMemcpy(out, h->d_cands, cnt * sizeof(pm_hit), hipMemcpyDeviceToHost));
  }
  return PM_OK;
}

extern "C" int pm_candidates_device(pm_handle *h, void **d_records, size_t *n) {
  if (!h || !h->inited) return PM_E_INVALID;
  drain_spec(h);                                                    // (after pm_scan: the buffer belongs to the next range's scan -- no records)
  if (d_records) *d_records = h->d_cands;
  if (n) *n = h->last_count;
  return PM_OK;
}

extern "C" int pm_scan_stats(pm_handle *h, uint64_t *out, int n) {
  if (!h || !h->inited || !out || n < 0) return PM_E_INVALID;
  uint64_t v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // pm_scan's look-ahead scan copies its counters into h_seed_count when it ends: wait for it (it stays pm_scan's to collect)
  if (h->spec && h->scan_pending) (void)hipStreamSynchronize(h->stream);
  v[0] = h->last_count;
  if (h->h_seed_count) {
    const size_t tiles = !h->pair.empty() ? h->pair.size() : 1 + h->sd_more.size();
    for (size_t t = 0; t < tiles && t < 256; ++t) v[1] = std::max<uint64_t>(v[1], h->h_seed_count[1 + t]);
    if (h->nshort || h->nssub) v[1] += h->h_seed_count[SHORT_COUNT_AT];   // (+ the short class's seed records / suspects)
    if (h->nwild) v[1] += h->h_seed_count[WILD_COUNT_AT];             // (+ the wild class's suspects)
    v[3] = h->h_seed_count[257]; v[4] = h->h_seed_count[258]; v[5] = h->h_seed_count[259];
  }
  v[2] = h->internal_rescans;
  v[6] = h->range_splits;
  v[7] = h->lookaheads;
  v[8] = h->last_suspects;
  for (int i = 0; i < n && i < 9; ++i) out[i] = v[i];
  return PM_OK;
}

// Measurement (no reference counterpart): time the pair geometry as the FIRST STAGE of an edit-distance
// plan on this handle's tables -- a -K 2 handle on the pair plan -- over the whole stream: 14 (field pair, displacement)
// tests per window (scripts/edit_pair_cover.py), mode 1 = with the substitution compare (a lower bound of such a kernel),
// mode 2 = with the five-shift necessary condition for "<= 2 edits on the other ten bases" on two patterns per slot.
// Produces no hits: *ms is the kernel's duration, *suspects the records it would hand to a verify kernel.
extern "C" int pm_measure_pair_edit_floor(pm_handle *h, int mode, float *ms, uint64_t *suspects) {
  if (!h || !h->inited || !ms || !suspects || (mode != 1 && mode != 2)) return fail(h, PM_E_INVALID, "pm_measure_pair_edit_floor: bad arguments");
  if (h->win) return fail(h, PM_E_INVALID, "pm_measure_pair_edit_floor: needs the whole stream resident (not pm_init_windowed)");
  if (h->kern != PM_KERNEL_SEED || h->pair.size() != 1 || h->cfg.k != 2 || h->cfg.indels)
    return fail(h, PM_E_UNSUPPORTED, "pm_measure_pair_edit_floor: needs a -K 2 handle on the pair plan (one pattern tile)");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  drain_spec(h);
  const size_t want = (size_t)(h->n / 16) + ((size_t)1 << 20);
  if (!h->d_susp || h->susp_cap < want) {
    if (h->d_susp) { (void)hipFree(h->d_susp); h->d_susp = nullptr; }
    h->susp_cap = want;
    HIP_TRY(h, hipMalloc(&h->d_susp, h->susp_cap * PAIR_SUSPECT_BYTES));
  }
  if (!h->d_seed_count) HIP_TRY(h, hipMalloc((void **)&h->d_seed_count, SEEDCOUNT_WORDS * sizeof(unsigned long long)));
  HIP_TRY(h, hipMemsetAsync(h->d_seed_count, 0, SEEDCOUNT_WORDS * sizeof(unsigned long long), h->stream));
  HIP_TRY(h, hipMemsetAsync(h->d_counter, 0, sizeof(unsigned long long), h->stream));
  HIP_TRY(h, hipEventRecord(h->ev0, h->stream));
  HIP_TRY(h, pair_launch(h->pair[0], h->d_text, h->d_packed, h->n, 0, h->n, h->d_cands, h->d_counter, h->cap, h->d_susp, h->d_seed_count + 1, h->susp_cap,
                         h->stream, nullptr, nullptr, mode));
  HIP_TRY(h, hipEventRecord(h->ev1, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->h_seed_count, h->d_seed_count, SEEDCOUNT_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  (void)hipEventElapsedTime(ms, h->ev0, h->ev1);
  *suspects = h->h_seed_count[1];
  return PM_OK;
}

extern "C" int pm_pack_time(pm_handle *h, float *ms) {
  if (!h || !h->inited || !ms) return PM_E_INVALID;
  *ms = (h->kern == PM_KERNEL_SEED || (h->pk_bits && !h->win)) ? h->pack_ms : 0.f;   // (a resident packed handle: its unpack kernel)
  return PM_OK;
}

extern "C" int pm_final_hits_device(pm_handle *h, void **d_hits, size_t *n) {
  if (!h || !h->inited) return PM_E_INVALID;
  if (d_hits) *d_hits = const_cast<pm_hit *>(h->d_final);
  if (n) *n = h->n_final;
  return PM_OK;
}

extern "C" int pm_copy_records(pm_handle *h, const void *d_src, size_t n, pm_hit *out) {
  if (!h || !h->inited || (n && (!d_src || !out))) return fail(h, PM_E_INVALID, "pm_copy_records: bad arguments");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  if (n) HIP_TRY(h, hipMemcpyAsync(out, d_src, n * sizeof(pm_hit), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, stream_wait(h));
  return PM_OK;
}

extern "C" int pm_last_kernel_time(pm_handle *h, float *ms, int *launches) {
  if (!h) return PM_E_INVALID;
  if (ms) *ms = h->last_ms;
  if (launches) *launches = h->last_launches;
  return PM_OK;
}

// ---- host stage --------------------------------------------------------------------------------
namespace {

struct Window { int64_t start; int32_t len; int64_t off; };

// Raw characters (cp.getch()) of a batch of stream windows, from the host copy of the stream
// when there is one, else gathered from HBM by one kernel + one copy.  Bytes outside [0,n) read
// as code 0, like the reference's unchecked mmap reads of the zero-padded last page.
int fetch_windows(pm_handle *h, std::vector<Window> &wins) {
  int64_t total = 0;
  for (Window &w : wins) { w.off = total; total += w.len; }
  h->winbuf.resize((size_t)total + 1);
  if (wins.empty()) return PM_OK;
  if (has_host_form(h)) {
    // host copy of the stream: copy (or decode, from the packed form) + code -> character in one pass, slices of windows per thread
    auto copy = [&](size_t lo, size_t hi) {
      for (size_t wi = lo; wi < hi; ++wi) {
        const Window &w = wins[wi];
        uint8_t *dst = h->winbuf.data() + w.off;
        if (h->h_text) {
          for (int i = 0; i < w.len; ++i) {
            const int64_t p = w.start + i;
            dst[i] = h->alpha.ch[(p >= 0 && p < h->n) ? h->h_text[p] : 0];
          }
        } else {
          const int64_t a = std::min(h->n, std::max<int64_t>(0, w.start)), b = std::max(a, std::min(h->n, w.start + w.len));
          memset(dst, 0, (size_t)w.len);
          if (b > a) (void)pm_unpack_codes(h->h_packed, h->h_packed_bytes, h->pk_bits, a, b - a, dst + (a - w.start));
          for (int i = 0; i < w.len; ++i) dst[i] = h->alpha.ch[dst[i]];
        }
      }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nthreads = wins.size() < 4096 ? 1 : std::min<size_t>(hw ? hw : 1, 16);
    if (nthreads <= 1) copy(0, wins.size());
    else {
      std::vector<std::thread> pool;
      const size_t per = (wins.size() + nthreads - 1) / nthreads;
      for (size_t t = 0; t < nthreads; ++t)
        pool.emplace_back([&, t]() { copy(std::min(wins.size(), t * per), std::min(wins.size(), (t + 1) * per)); });
      for (std::thread &th : pool) th.join();
    }
    return PM_OK;
  } else {
    const size_t cnt = wins.size();
    if (h->d_wcap < cnt) {
      if (h->d_wstart) { (void)hipFree(h->d_wstart); (void)hipFree(h->d_wlen); (void)hipFree(h->d_woff); }
      h->d_wcap = cnt * 2;
      HIP_TRY(h, hipMalloc((void **)&h->d_wstart, h->d_wcap * 8));
      HIP_TRY(h, hipMalloc((void **)&h->d_wlen, h->d_wcap * 4));
      HIP_TRY(h, hipMalloc((void **)&h->d_woff, h->d_wcap * 8));
    }
    if (h->d_woutcap < (size_t)total) {
      if (h->d_wout) (void)hipFree(h->d_wout);
      h->d_woutcap = (size_t)total * 2;
      HIP_TRY(h, hipMalloc((void **)&h->d_wout, h->d_woutcap));
    }
    std::vector<int64_t> st(cnt), of(cnt); std::vector<int32_t> ln(cnt);
    for (size_t i = 0; i < cnt; ++i) { st[i] = wins[i].start; ln[i] = wins[i].len; of[i] = wins[i].off; }
    // (while pm_scan has the next range's scan on the handle's stream, the windows go through the copy stream: the
    // stream text is read-only and the staging buffers are used by this function alone)
    hipStream_t ws = h->spec && h->copy_stream ? h->copy_stream : h->stream;
    HIP_TRY(h, hipMemcpyAsync(h->d_wstart, st.data(), cnt * 8, hipMemcpyHostToDevice, ws));
    HIP_TRY(h, hipMemcpyAsync(h->d_wlen, ln.data(), cnt * 4, hipMemcpyHostToDevice, ws));
    HIP_TRY(h, hipMemcpyAsync(h->d_woff, of.data(), cnt * 8, hipMemcpyHostToDevice, ws));
    HIP_TRY(h, gather_windows(h->d_text, h->n, h->d_wstart, h->d_wlen, h->d_woff, (int)cnt, h->d_wout, ws));
    HIP_TRY(h, hipMemcpyAsync(h->winbuf.data(), h->d_wout, (size_t)total, hipMemcpyDeviceToHost, ws));
    HIP_TRY(h, hipStreamSynchronize(ws));
  }
  for (int64_t i = 0; i < total; ++i) h->winbuf[i] = h->alpha.ch[h->winbuf[i]];
  return PM_OK;
}

bool by_end_pid(const pm_hit &a, const pm_hit &b) {
  if (a.end != b.end) return a.end < b.end;
  if (a.pid != b.pid) return a.pid < b.pid;
  return a.k < b.k;
}

// (end, pid, k) order for large hit lists: ends are spread over the scanned range, so split the
// range of ends into equal slices, one thread per slice (std::sort of 10^6 records took 25 ms)
void sort_hits(pm_hit *v, size_t n) {
  if (n < ((size_t)1 << 16)) { std::sort(v, v + n, by_end_pid); return; }
  int64_t lo = v[0].end, hi = v[0].end;
  for (size_t i = 1; i < n; ++i) { lo = std::min(lo, v[i].end); hi = std::max(hi, v[i].end); }
  const int T = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const int64_t span = (hi - lo) / T + 1;
  std::vector<size_t> cnt((size_t)T + 1, 0);
  for (size_t i = 0; i < n; ++i) ++cnt[(size_t)((v[i].end - lo) / span) + 1];
  for (int t = 0; t < T; ++t) cnt[(size_t)t + 1] += cnt[(size_t)t];
  std::vector<pm_hit> tmp(n);
  std::vector<size_t> at(cnt.begin(), cnt.end() - 1);
  for (size_t i = 0; i < n; ++i) tmp[at[(size_t)((v[i].end - lo) / span)]++] = v[i];
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back([&, t]() {
    std::sort(tmp.begin() + (ptrdiff_t)cnt[(size_t)t], tmp.begin() + (ptrdiff_t)cnt[(size_t)t + 1], by_end_pid);
    std::copy(tmp.begin() + (ptrdiff_t)cnt[(size_t)t], tmp.begin() + (ptrdiff_t)cnt[(size_t)t + 1], v + cnt[(size_t)t]);
  });
  for (std::thread &x : th) x.join();
}

pm_hit make_hit(int64_t end, uint64_t pid, int k) {
  pm_hit x; x.end = end; x.pid = (uint32_t)pid; x.k = (uint8_t)k; x.aux[0] = x.aux[1] = x.aux[2] = 0;
  return x;
}

// filter_bitvec::find_patterns (filter_bitvec.cc:88-177) over carried + new candidates.
// The reference sorts all candidates by position and, for every still-live candidate, chains
// later candidates of the same pattern while they lie within 2k+1 of the last one chained
// (:103-116).  Chains never mix patterns, so the same clusters fall out of grouping the
// candidates by pattern (counting sort, O(n)) and cutting each pattern's ends at gaps > 2k+1.
int finalize_filter_bitvec(pm_handle *h, const pm_hit *cands, size_t n, int64_t scanned_to, bool last,
                           std::vector<pm_hit> &outv) {
  const double tf0 = now_ms();
  const size_t np = h->pats.size();
  const int k = h->cfg.k, win = 2 * k + 1;
  const bool indels = h->cfg.indels != 0;
  const size_t total = h->carry.size() + n;
  if (total == 0) return PM_OK;
  // group by inner pattern id (1..np)
  std::vector<uint32_t> first(np + 2, 0);
  for (const pm_hit &c : h->carry) ++first[c.pid + 1];
  for (size_t i = 0; i < n; ++i) ++first[cands[i].pid + 1];
  for (size_t j = 1; j <= np + 1; ++j) first[j] += first[j - 1];
  std::vector<pm_hit> g(total);
  {
    std::vector<uint32_t> at(first.begin(), first.end() - 1);
    for (const pm_hit &c : h->carry) g[at[c.pid]++] = c;
    for (size_t i = 0; i < n; ++i) g[at[cands[i].pid]++] = cands[i];
  }
  std::vector<pm_hit> keep;
  struct Cluster { int64_t first, last; uint32_t pid; };
  std::vector<Cluster> need_dp;
  for (size_t pid = 1; pid <= np; ++pid) {
    const size_t lo = first[pid], hi = first[pid + 1];
    if (lo == hi) continue;
    if (hi - lo > 1) std::sort(g.begin() + lo, g.begin() + hi, [](const pm_hit &a, const pm_hit &b) { return a.end < b.end; });
    const Pattern &p = h->pats[pid - 1];
    const int L = (int)p.s.size();
    size_t i = lo;
    while (i < hi) {
      size_t j = i + 1;
      int best_lvl = g[i].k; int64_t best_end = g[i].end;
      while (j < hi && g[j].end <= g[j - 1].end + win) {
        if (g[j].k < best_lvl) { best_lvl = g[j].k; best_end = g[j].end; }
        ++j;
      }
      const int64_t c_first = g[i].end, c_last = g[j - 1].end;
      if (!last && scanned_to < c_last + win) {                     // :118-121: the cluster may still grow
        keep.insert(keep.end(), g.begin() + i, g.begin() + j);
      } else if (!indels && p.esb == 0 && p.eeb == 0 && c_first >= L && !(h->nn_quirk && pattern_n_quirk(h, p))) {
        // Substitution-only search without exact-base constraints needs no text: the DP
        // (pattern_alignment.cc with b = 0) walks diagonals only, so the cluster's value is the
        // smallest Hamming distance among its windows -- the smallest candidate level, windows that
        // are not candidates having distance > k -- and the column rule (:461-475) keeps the
        // left-most such window.
        outv.push_back(make_hit(best_end, p.id, best_lvl));
      } else need_dp.push_back(Cluster{c_first, c_last, (uint32_t)pid});
      i = j;
    }
  }
  h->carry.swap(keep);
  if (need_dp.empty()) return PM_OK;
  std::vector<Window> wins;
  wins.reserve(need_dp.size());
  for (const Cluster &c : need_dp) {
    const int L = (int)h->pats[c.pid - 1].s.size();
    int64_t ws = 0;
    if (c.first > (int64_t)L + k) ws = c.first - L - k;             // pattern_alignment.cc:137-139
    wins.push_back(Window{ws, (int32_t)(c.last - ws), 0});
  }
  const double tf1 = now_ms();
  int rc = fetch_windows(h, wins);
  if (rc) return rc;
  const double tf2 = now_ms();
  AlignParams prm; prm.k = k; prm.indels = indels; prm.eos = (uint8_t)h->cfg.eos;
  prm.wc = h->cfg.wildcards != 0; prm.tn = h->cfg.text_n != 0;
  // one DP per cluster; the clusters are independent: slices per host thread, results kept in order
  std::vector<AlignResult> res(need_dp.size());
  auto run = [&](size_t lo, size_t hi, AlignScratch &scratch) {
    for (size_t wi = lo; wi < hi; ++wi) {
      const Cluster &c = need_dp[wi];
      const Pattern &p = h->pats[c.pid - 1];
      res[wi] = editdist_align(h->winbuf.data() + wins[wi].off, wins[wi].start, c.first, c.last,
                               p.s.data(), (int)p.s.size(), p.esb, p.eeb, prm, scratch);
    }
  };
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t nthreads = need_dp.size() < 4096 ? 1 : std::min<size_t>(hw ? hw : 1, 16);
  if (nthreads <= 1) run(0, need_dp.size(), h->scratch);
  else {
    std::vector<std::thread> pool;
    const size_t per = (need_dp.size() + nthreads - 1) / nthreads;
    for (size_t t = 0; t < nthreads; ++t)
      pool.emplace_back([&, t]() { AlignScratch sc; run(std::min(need_dp.size(), t * per), std::min(need_dp.size(), (t + 1) * per), sc); });
    for (std::thread &th : pool) th.join();
  }
  for (size_t wi = 0; wi < need_dp.size(); ++wi)
    if (res[wi].ok) outv.push_back(make_hit(res[wi].end, h->pats[need_dp[wi].pid - 1].id, res[wi].value));   // :135
  if (h->knobs.debug) fprintf(stderr, "[pm] filter_bitvec host stage: cluster %.1f ms, windows %.1f ms, %zu DPs %.1f ms\n", tf1 - tf0, tf2 - tf1, need_dp.size(), now_ms() - tf2);
  return PM_OK;
}

bool seed_order(const pm_hit &a, const pm_hit &b) {                  // exact_halves.cc:114-118
  if (a.end != b.end) return a.end < b.end;
  return a.pid > b.pid;
}

// Sort records into seed_order.  std::sort on 16-byte records was most of the host stage
// (5 ms per 80k records); positions < 2^40 and ids < 2^24 make one 64-bit key, sorted by an LSD
// radix sort of (key, index) pairs.
void sort_seed_order(std::vector<pm_hit> &v) {
  const size_t n = v.size();
  bool fits = n < ((size_t)1 << 31);
  for (size_t i = 0; i < n && fits; ++i) fits = v[i].end >= 0 && v[i].end < ((int64_t)1 << 40) && v[i].pid < (1u << 24);
  if (!fits || n < 64) { std::sort(v.begin(), v.end(), seed_order); return; }
  struct KI { uint64_t key; uint32_t idx; };
  std::vector<KI> a(n), b(n);
  uint64_t all_or = 0;
  for (size_t i = 0; i < n; ++i) {
    a[i].key = ((uint64_t)v[i].end << 24) | (uint64_t)(0xffffffu - v[i].pid);   // id descending
    a[i].idx = (uint32_t)i;
    all_or |= a[i].key;
  }
  constexpr int BITS = 11;
  std::vector<uint32_t> cnt((size_t)1 << BITS);
  for (int shift = 0; shift < 64 && (all_or >> shift) != 0; shift += BITS) {
    std::fill(cnt.begin(), cnt.end(), 0u);
    for (size_t i = 0; i < n; ++i) ++cnt[(a[i].key >> shift) & ((1u << BITS) - 1)];
    uint32_t run = 0;
    for (uint32_t &c : cnt) { const uint32_t t = c; c = run; run += t; }
    for (size_t i = 0; i < n; ++i) b[cnt[(a[i].key >> shift) & ((1u << BITS) - 1)]++] = a[i];
    a.swap(b);
  }
  std::vector<pm_hit> out(n);
  for (size_t i = 0; i < n; ++i) out[i] = v[a[i].idx];
  v.swap(out);
}

// exact_halves::find_patterns (exact_halves.cc:140-190) / exact_bases (exact_bases.cc:92-121)
int finalize_seeds(pm_handle *h, const pm_hit *cands, size_t n, bool halves, std::vector<pm_hit> &outv) {
  std::vector<pm_hit> seeds(cands, cands + n);
  if (halves) sort_seed_order(seeds);
  else std::sort(seeds.begin(), seeds.end(), by_end_pid);
  const int k = h->cfg.k;
  const bool indels = h->cfg.indels != 0;
  struct Job { int pat; bool left; int len1, len2; };
  std::vector<Job> jobs(seeds.size());
  std::vector<Window> wins(seeds.size());
  for (size_t i = 0; i < seeds.size(); ++i) {
    const uint32_t hid = seeds[i].pid;
    Job j;
    if (halves) {
      j.pat = (int)((hid - 1) / 2);
      const int L = (int)h->pats[j.pat].s.size();
      j.len1 = L / 2; j.len2 = L - j.len1; j.left = (hid % 2) == 1;
    } else {
      j.pat = (int)hid - 1;
      const Pattern &p = h->pats[j.pat];
      const int L = (int)p.s.size();
      j.left = p.esb >= p.eeb;
      j.len1 = j.left ? p.esb : L - p.eeb; j.len2 = L - j.len1;
    }
    jobs[i] = j;
    if (j.left) wins[i] = Window{seeds[i].end, j.len2 + k, 0};                       // primer_alignment.cc:573-574
    else {
      int64_t ws = 0;
      const int plen = j.len1 + j.len2 + k;
      if (seeds[i].end > (int64_t)plen) ws = seeds[i].end - plen;                      // :657-662
      wins[i] = Window{ws, (int32_t)std::max<int64_t>(0, seeds[i].end - j.len2 - ws), 0};
    }
  }
  int rc = fetch_windows(h, wins);
  if (rc) return rc;
  AlignParams prm; prm.k = k; prm.indels = indels; prm.eos = (uint8_t)h->cfg.eos;
  prm.wc = h->cfg.wildcards != 0; prm.tn = h->cfg.text_n != 0;
  for (size_t i = 0; i < seeds.size(); ++i) {
    const Job &j = jobs[i];
    const Pattern &p = h->pats[j.pat];
    int64_t end = 0; int val = 0; bool ok;
    if (j.left) ok = lmatch_extend(h->winbuf.data() + wins[i].off, seeds[i].end, j.len1, p.s.data() + j.len1, j.len2,
                                   p.esb, p.eeb, prm, h->scratch, &end, &val);
    else ok = rmatch_extend(h->winbuf.data() + wins[i].off, wins[i].len, seeds[i].end, p.s.data(), j.len1, j.len2,
                            p.esb, p.eeb, prm, h->scratch, &end, &val);
    if (!ok) continue;
    if (halves) {
      if (end > h->lasthit[j.pat + 1] + (indels ? 2 * k : 0)) {      // exact_halves.cc:163,178
        outv.push_back(make_hit(end, p.id, val));
        h->lasthit[j.pat + 1] = end;
      }
    } else outv.push_back(make_hit(end, p.id, val));
  }
  return PM_OK;
}

// exact_halves on whole-pattern Hamming candidates (seed family, -K only): a candidate whose left
// half is clean was found by the reference through the left seed at end-len2 (inner id 2j-1), one
// whose right half is clean through the right seed at end (inner id 2j); both report
// (end, distance) (primer_alignment.cc:568-617, 651-704 with indels off).  Seeds are then
// replayed in the reference's order (position asc, inner id desc) through the per-pattern
// "end > last kept end" rule (exact_halves.cc:114-118,163,178).
int finalize_halves_flags(pm_handle *h, const pm_hit *cands, size_t n, int64_t scanned_to, bool last,
                          std::vector<pm_hit> &outv) {
  // a seed is kept in h->carry as {end = seed position, pid = inner id, k = value, aux[0] = end - position}
  std::vector<pm_hit> &seeds = h->carry;
  for (size_t i = 0; i < n; ++i) {
    const uint32_t j = cands[i].pid;                                // 1-based pattern index
    const int L = (int)h->pats[j - 1].s.size();
    const int len2 = L - L / 2;
    if (cands[i].aux[0] & 1) { pm_hit x = make_hit(cands[i].end - len2, 2 * j - 1, cands[i].k); x.aux[0] = (uint8_t)len2; seeds.push_back(x); }
    if (cands[i].aux[0] & 2) seeds.push_back(make_hit(cands[i].end, 2 * j, cands[i].k));
  }
  sort_seed_order(seeds);
  // candidates still to come end beyond scanned_to, so their seeds lie beyond scanned_to - maxlen:
  // everything at or before that is in its final order
  const int64_t safe = last ? INT64_MAX : scanned_to - h->sd.maxlen;
  size_t i = 0;
  for (; i < seeds.size() && seeds[i].end <= safe; ++i) {
    const uint32_t j = (seeds[i].pid + 1) / 2;
    const int64_t end = seeds[i].end + seeds[i].aux[0];
    if (end > h->lasthit[j]) {
      outv.push_back(make_hit(end, h->pats[j - 1].id, seeds[i].k));
      h->lasthit[j] = end;
    }
  }
  seeds.erase(seeds.begin(), seeds.begin() + i);
  return PM_OK;
}

// exact_halves -k with the extension done on the GPU (pm_extend.hip): records are
// {end = seed position, pid = inner id, k = value, aux[0] = hit end - seed position}.  What is left
// is the reference's sequential rule (exact_halves.cc:142,163,178): seeds in (position asc, inner id
// desc) order, a hit is kept if its end exceeds the pattern's last kept end by more than 2k.
int finalize_extended(pm_handle *h, const pm_hit *cands, size_t n, std::vector<pm_hit> &outv) {
  std::vector<pm_hit> seeds(cands, cands + n);
  sort_seed_order(seeds);
  const int slack = h->cfg.indels ? 2 * h->cfg.k : 0;
  for (const pm_hit &s : seeds) {
    const uint32_t j = (s.pid + 1) / 2;
    const int64_t end = s.end + s.aux[0];
    if (end > h->lasthit[j] + slack) {
      outv.push_back(make_hit(end, h->pats[j - 1].id, s.k));
      h->lasthit[j] = end;
    }
  }
  return PM_OK;
}

}  // namespace

static int finalize_into(pm_handle *h, const pm_hit *cands, size_t n, int64_t scanned_to, bool last,
                         std::vector<pm_hit> &outv) {
  int rc = PM_OK;
  switch (h->sem) {
    case PM_SEM_KEYWORD_TREE: case PM_SEM_SHIFT_AND: case PM_SEM_SHIFT_AND_INEXACT:
      outv.insert(outv.end(), cands, cands + n);
      for (size_t i = outv.size() - n; i < outv.size(); ++i) outv[i].aux[0] = outv[i].aux[1] = outv[i].aux[2] = 0;   // engine-private bytes
      break;
    case PM_SEM_FILTER_BITVEC: rc = finalize_filter_bitvec(h, cands, n, scanned_to, last, outv); break;
    case PM_SEM_EXACT_HALVES:
      h->halves_fresh = false;
      rc = h->seed_flags ? finalize_halves_flags(h, cands, n, scanned_to, last, outv)
         : h->halves_dev ? finalize_extended(h, cands, n, outv) : finalize_seeds(h, cands, n, true, outv);
      break;
    case PM_SEM_EXACT_BASES:
      if (h->bases_flags) {                                          // seed family: the records are the hits
        outv.insert(outv.end(), cands, cands + n);
        for (size_t i = outv.size() - n; i < outv.size(); ++i) outv[i].aux[0] = outv[i].aux[1] = outv[i].aux[2] = 0;
      }
      else rc = finalize_seeds(h, cands, n, false, outv);
      break;
    default: return fail(h, PM_E_INVALID, "finalize: bad semantics");
  }
  return rc;
}

extern "C" int pm_finalize(pm_handle *h, const pm_hit *cands, size_t n, int64_t scanned_to, int flags,
                           pm_hit *out, size_t cap, size_t *n_out) {
  const int last = flags & PM_FINALIZE_LAST;
  if (!h || !h->inited || (!cands && n)) return fail(h, PM_E_INVALID, "pm_finalize: bad arguments");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  std::vector<pm_hit> outv;
  int rc = finalize_into(h, cands, n, scanned_to, last != 0, outv);
  if (rc) return rc;
  if (flags & PM_FINALIZE_SORTED) sort_hits(outv.data(), outv.size());
  if (n_out) *n_out = outv.size();
  if (outv.size() > cap) return fail(h, PM_E_OVERFLOW, "pm_finalize: out buffer too small");
  if (!outv.empty()) memcpy(out, outv.data(), outv.size() * sizeof(pm_hit));
  return PM_OK;
}

// Device form of pm_finalize for the option sets whose host stage needs no stream text and no
// order-dependent state: exact engines and bare shift_and_inexact (pass-through) and
// filter_bitvec with -K and no exact-base constraints (sort + segmented pass, pm_cluster.hip).
// d_cands == NULL means "the records of the last pm_scan_candidates".  Final hits are copied to
// `out` (host).  The few clusters the device cannot decide (still growing at scanned_to, or
// starting inside the first L characters) go through the host stage.
// `next` != NULL is pm_scan's form: the final hits are sorted on the device and land, in (end, pid, k) order, behind the
// records the handle's landing buffer already holds; with next->on the scan of the range (next->b, next->e] is enqueued
// behind the finalize kernels before the host waits for them, so that the copies out of HBM and everything the caller
// does with the hits run beside it.
struct ScanNext { bool on; int64_t b, e; };
static int finalize_device_impl(pm_handle *h, const void *d_cands, size_t n, int64_t scanned_to, int flags,
                                const OwnedRange &own, pm_hit *out, size_t cap, size_t *n_out, const ScanNext *next = nullptr);

// filter_bitvec with -K and no exact-base constraints: its verify is "smallest level, left-most end"
// (pm_cluster.hip), no stream text needed
static bool device_cluster_plain(const pm_handle *h) {
  if (!(h->sem == PM_SEM_FILTER_BITVEC && !h->cfg.indels && h->cfg.k <= 3 && h->pats.size() < ((size_t)1 << 22))) return false;
  if (h->nn_quirk) return false;                                    // pattern N at a stream N under -w: the value is the DP's (pattern_n_quirk)
  // with exact-base constraints only on the pair plan, whose records mark zone violations (level 3, k <= 2)
  if (h->zoned) return h->kern == PM_KERNEL_SEED && !h->pair.empty() && h->nrest == 0 && h->cfg.k <= 2;
  return true;
}

extern "C" int pm_finalize_device(pm_handle *h, const void *d_cands, size_t n, int64_t scanned_to, int flags,
                                  pm_hit *out, size_t cap, size_t *n_out) {
  const OwnedRange all = {0, 0, 0, 0, 0};
  if (h) drain_spec(h);
  return finalize_device_impl(h, d_cands, n, scanned_to, flags, all, out, cap, n_out);
}

// One shard of a position-sharded scan: the records hold every candidate that ends
// in (guard_lo, guard_hi] and this call reports the hits that end in (own_lo, own_hi], so the shards'
// outputs concatenate to the single-scan result without a merge stage and each shard's cluster DPs
// read the text the shard itself holds.  guard_lo <= 0 / guard_hi == INT64_MAX: the stream really
// starts / ends there.  A same-pattern chain of candidates that reaches from a guard edge into the
// owned range (a tandem repeat longer than the guard band) cannot be decided here: PM_E_UNSUPPORTED.
extern "C" int pm_finalize_device_owned(pm_handle *h, const void *d_cands, size_t n, int64_t own_lo, int64_t own_hi,
                                        int64_t guard_lo, int64_t guard_hi, int flags, pm_hit *out, size_t cap, size_t *n_out) {
  if (!(guard_lo <= own_lo && own_lo <= own_hi && own_hi <= guard_hi))
    return fail(h, PM_E_INVALID, "pm_finalize_device_owned: need guard_lo <= own_lo <= own_hi <= guard_hi");
  // the shard that holds the true end of the stream also owns the hits that end beyond it (extensions that read
  // past the end, stream_end_overhang_candidates)
  if (h) drain_spec(h);
  const bool to_the_end = h && guard_hi == INT64_MAX && own_hi >= h->n;
  const OwnedRange own = {own_lo, to_the_end ? INT64_MAX : own_hi, guard_lo, guard_hi, 1};
  return finalize_device_impl(h, d_cands, n, guard_hi == INT64_MAX ? h->n : guard_hi, flags | PM_FINALIZE_LAST, own, out, cap, n_out);
}

// room for `need` records in the landing buffer, the ones not handed out yet moved to its front
static int ensure_landing(pm_handle *h, size_t need_more) {
  const size_t live = h->land_n - h->land_pos;
  if (h->land_cap >= live + need_more) {
    if (h->land_pos) { if (live) memmove(h->land, h->land + h->land_pos, live * sizeof(pm_hit)); h->land_n = live; h->land_pos = 0; }
    return PM_OK;
  }
  const size_t want = live + need_more;
  const size_t cap = std::max<size_t>(want + want / 2, (size_t)1 << 16);
  pm_hit *p = nullptr;
  HIP_TRY(h, hipHostMalloc((void **)&p, cap * sizeof(pm_hit), hipHostMallocDefault));
  if (live) memcpy(p, h->land + h->land_pos, live * sizeof(pm_hit));
  if (h->land) (void)hipHostFree(h->land);
  h->land = p; h->land_cap = cap; h->land_n = live; h->land_pos = 0;
  return PM_OK;
}

// Can the device put final hits in (end, pid, k) order with one keys-only radix sort (pm_cluster.hip sort_final_device)?
// key = end | pattern index | k in <= 63 bits, pattern ids growing with the index.  Decided once per init.
static void device_sort_plan(pm_handle *h) {
  h->sort_dev = false;
  if (h->cfg.k > 3 || h->pats.empty() || h->pats.size() >= ((size_t)1 << 22)) return;
  for (size_t i = 1; i < h->pats.size(); ++i) if (h->pats[i].id <= h->pats[i - 1].id) return;
  int ib = 1, eb = 0;
  while (((size_t)1 << ib) < h->pats.size()) ++ib;
  const uint64_t maxend = (uint64_t)h->n + 512;                     // (extensions may end a few characters beyond the stream)
  while (eb < 64 && (maxend >> eb)) ++eb;
  h->sort_idxbits = ib; h->sort_keybits = eb + ib + 2;
  h->sort_dev = h->sort_keybits <= 63;
}

// pattern lengths and ids by pattern index, on the device (clustering, the halves rule, the final sort)
static int ensure_fpat(pm_handle *h) {
  if (h->d_fpat_len) return PM_OK;
  std::vector<uint8_t> pl(h->pats.size()); std::vector<uint32_t> pi(h->pats.size());
  for (size_t i = 0; i < h->pats.size(); ++i) { pl[i] = (uint8_t)std::min<size_t>(h->pats[i].s.size(), 255); pi[i] = (uint32_t)h->pats[i].id; }
  PM_TRY(dev_upload(h, &h->d_fpat_len, pl, 1, "d_fpat_len"));
  return dev_upload(h, &h->d_fpat_id, pi, 4, "d_fpat_id");
}

// room for n records in d_fsorted, where pm_scan's final hits wait for their copy to the host
static int ensure_fsorted(pm_handle *h, size_t n) {
  if (h->fsorted_cap >= n) return PM_OK;
  h->fsorted_cap = std::max<size_t>(n + n / 4, (size_t)1 << 16);
  return dev_regrow(h, &h->d_fsorted, h->fsorted_cap * sizeof(pm_hit), "d_fsorted");
}

// pm_scan's landing: n_upper bounds the number of final hits at d_hits (their count is d_count on the device when the
// kernels in front produce it, else n_upper itself).  Enqueues the sort; *sorted tells whether the device could.
static int land_enqueue_sort(pm_handle *h, const pm_hit *d_hits, const unsigned long long *d_count, size_t n_upper, bool *sorted) {
  *sorted = false;
  if (h->counting) return count_feed_device(h, d_hits, d_count, n_upper);   // pm_count_scan: the finals are re-aligned where they are
  if (h->pcr_scanning) return pcr_land_device(h, d_hits, n_upper);         // pm_pcr_scan: the finals join the held list in HBM
  if (n_upper == 0 || n_upper > (size_t)INT_MAX / 2 || !h->sort_dev) return PM_OK;
  { int rcw = ensure_sort_workspace(h, n_upper, false); if (rcw) return rcw; }
  { int rcp = ensure_fpat(h); if (rcp) return rcp; }
  { int rcf = ensure_fsorted(h, n_upper); if (rcf) return rcf; }
  HIP_TRY(h, sort_final_device(d_hits, d_count, n_upper, h->d_fpat_id, (uint32_t)h->pats.size(), h->sort_idxbits, h->sort_keybits,
                               h->d_keys, h->d_keys_alt, h->d_fsorted, h->d_ctemp, h->ctemp_bytes, h->stream));
  *sorted = true;
  return PM_OK;
}

// Wait for the finalize kernels enqueued so far.  pm_scan's form (next): the scan of the next range goes in behind them first.
static int finalize_sync(pm_handle *h, const ScanNext *next) {
  if (!next) { HIP_TRY(h, stream_wait(h)); return PM_OK; }
  HIP_TRY(h, hipEventRecord(h->ev_fin, h->stream));
  if (next->on && !h->spec) {
    if (pm_scan_candidates_async(h, next->b, next->e) == PM_OK) { h->spec = true; h->spec_b = next->b; h->spec_e = next->e; ++h->lookaheads; }
  }
  HIP_TRY(h, hipEventSynchronize(h->ev_fin));
  return PM_OK;
}

// nfin final hits (sorted on the device: d_sorted, else as they are at d_hits) + the host-decided `extra` -> landing buffer,
// in (end, pid, k) order.  The copy runs on the copy stream: the handle's stream may hold the next range's scan.
static int land_collect(pm_handle *h, const pm_hit *d_hits, bool sorted, size_t nfin, std::vector<pm_hit> &extra, size_t *n_out) {
  if (h->counting) return count_collect(h, nfin, extra, n_out);
  if (h->pcr_scanning) return pcr_collect(h, nfin, extra, n_out);
  { int rcl = ensure_landing(h, nfin + extra.size()); if (rcl) return rcl; }
  pm_hit *dst = h->land + h->land_n;
  if (nfin) {
    HIP_TRY(h, hipMemcpyAsync(dst, sorted ? h->d_fsorted : d_hits, nfin * sizeof(pm_hit), hipMemcpyDeviceToHost, h->copy_stream));
    HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
    if (!sorted) {
      for (size_t i = 0; i < nfin; ++i) dst[i].aux[0] = dst[i].aux[1] = dst[i].aux[2] = 0;
      sort_hits(dst, nfin);
    }
  }
  if (!extra.empty()) {
    sort_hits(extra.data(), extra.size());
    memcpy(dst + nfin, extra.data(), extra.size() * sizeof(pm_hit));
    std::inplace_merge(dst, dst + nfin, dst + nfin + extra.size(), by_end_pid);
  }
  h->land_n += nfin + extra.size();
  if (n_out) *n_out = nfin + extra.size();
  return PM_OK;
}

// The end of a device finalize: nfin final hits at d_fout and the host-decided `extra` go to pm_scan's landing (land), stay
// in HBM (out == NULL: pm_final_hits_device), or are copied to the caller's buffer.
static int deliver_finals(pm_handle *h, bool land, bool sorted, size_t nfin, std::vector<pm_hit> &extra, int flags, pm_hit *out, size_t cap, size_t *n_out) {
  if (land) return land_collect(h, h->d_fout, sorted, nfin, extra, n_out);
  const size_t tot = nfin + extra.size();
  if (!out) {                                                       // the few host-decided hits join the device's in HBM
    if (tot > h->ckeys_cap) return fail(h, PM_E_OVERFLOW, "pm_finalize_device: device output buffer too small");
    if (!extra.empty()) HIP_TRY(h, hipMemcpy(h->d_fout + nfin, extra.data(), extra.size() * sizeof(pm_hit), hipMemcpyHostToDevice));
    h->d_final = h->d_fout; h->n_final = tot;
  } else {
    if (tot > cap) return fail(h, PM_E_OVERFLOW, "pm_finalize_device: out buffer too small");
    if (nfin) HIP_TRY(h, hipMemcpy(out, h->d_fout, nfin * sizeof(pm_hit), hipMemcpyDeviceToHost));
    if (!extra.empty()) memcpy(out + nfin, extra.data(), extra.size() * sizeof(pm_hit));
    if (flags & PM_FINALIZE_SORTED) sort_hits(out, tot);
  }
  if (n_out) *n_out = tot;
  return PM_OK;
}

static int finalize_device_impl(pm_handle *h, const void *d_cands, size_t n, int64_t scanned_to, int flags,
                                const OwnedRange &own, pm_hit *out, size_t cap, size_t *n_out, const ScanNext *next) {
  if (!h || !h->inited) return fail(h, PM_E_INVALID, "pm_finalize_device: handle not initialised");
  if (h->host_only) return fail(h, PM_E_UNSUPPORTED, "pm_finalize_device: this handle runs the host stage only (use pm_finalize)");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  const pm_hit *src = d_cands ? (const pm_hit *)d_cands : h->d_cands;
  if (!d_cands) n = h->last_count;
  const bool last = flags & PM_FINALIZE_LAST;
  if (n_out) *n_out = 0;
  // out == NULL: the final hits stay in HBM (pm_final_hits_device) for the exchange step of a sharded scan
  const bool land = next != nullptr;
  const bool keep = out == nullptr && !land;
  h->d_final = nullptr; h->n_final = 0;
  if (keep && (flags & PM_FINALIZE_SORTED)) return fail(h, PM_E_INVALID, "pm_finalize_device: PM_FINALIZE_SORTED needs a host buffer");
  const Route route = finalize_route(h);
  const bool passthrough = route == Route::Passthrough, cluster_dp = route == Route::ClusterDp;
  std::vector<pm_hit> none;
  if (route == Route::Halves) {                                     // stateless, so only for a complete range on a fresh engine state
    if (!last || own.on || !h->halves_fresh || !h->carry.empty())
      return fail(h, PM_E_UNSUPPORTED, "pm_finalize_device: exact_halves on the device needs the whole range in one call after pm_reset (use pm_finalize)");
    const size_t m = h->seed_flags ? 2 * n : n;
    { int rcw = ensure_sort_workspace(h, m, true); if (rcw) return rcw; }
    if (h->vals_cap < h->ckeys_cap) {
      void *old[] = {h->d_vals, h->d_vals_alt, h->d_htemp};           // (all three go before the first is allocated again)
      for (void *q : old) if (q) (void)hipFree(q);
      h->d_vals = h->d_vals_alt = nullptr; h->d_htemp = nullptr;
      h->vals_cap = h->ckeys_cap;
      HIP_TRY(h, hipMalloc((void **)&h->d_vals, h->vals_cap * 4));
      HIP_TRY(h, hipMalloc((void **)&h->d_vals_alt, h->vals_cap * 4));
      h->htemp_bytes = halves_temp_bytes(h->vals_cap);
      HIP_TRY(h, hipMalloc(&h->d_htemp, h->htemp_bytes ? h->htemp_bytes : 16));
    }
    { int rcp = ensure_fpat(h); if (rcp) return rcp; }
    HIP_TRY(h, halves_rule_device(src, n, h->seed_flags, h->cfg.indels ? 2 * h->cfg.k : 0, h->d_fpat_len, h->d_fpat_id, h->d_keys, h->d_keys_alt,
                                  h->d_vals, h->d_vals_alt, h->d_htemp, h->htemp_bytes, h->d_fout, h->d_fcounts, h->stream));
    bool sorted = false;
    if (land) { int rcs = land_enqueue_sort(h, h->d_fout, h->d_fcounts, m, &sorted); if (rcs) return rcs; }
    HIP_TRY(h, hipMemcpyAsync(h->h_fcounts, h->d_fcounts, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    { int rcy = finalize_sync(h, next); if (rcy) return rcy; }
    const size_t nfin = (size_t)h->h_fcounts[0];
    if (n_out) *n_out = nfin;
    return deliver_finals(h, land, sorted, nfin, none, flags, out, cap, n_out);
  }
  if (route == Route::Host) return fail(h, PM_E_UNSUPPORTED, "pm_finalize_device: this option set needs the host stage (pm_finalize)");
  if (passthrough && land) {                                        // the records are the hits: sort, [next scan], copy
    bool sorted = false;
    { int rcs = land_enqueue_sort(h, src, nullptr, n, &sorted); if (rcs) return rcs; }
    // Not sorted on the device (pattern ids in any order, 2^22 patterns, 2^30 hits): the copy to the host would read the
    // record buffer itself, which the next range's scan refills from slot 0.  The records move to d_fsorted on the handle's
    // stream, in front of that scan, and land from there; a list too long for that keeps the buffer: no scan behind it.
    ScanNext after = *next;
    if (!sorted && !h->counting && !h->pcr_scanning && n) {
      if (n <= (size_t)INT_MAX / 2) {
        { int rcf = ensure_fsorted(h, n); if (rcf) return rcf; }
        HIP_TRY(h, hipMemcpyAsync(h->d_fsorted, src, n * sizeof(pm_hit), hipMemcpyDeviceToDevice, h->stream));
        src = h->d_fsorted;
      } else after.on = false;
    }
    { int rcy = finalize_sync(h, &after); if (rcy) return rcy; }
    return land_collect(h, src, sorted, n, none, n_out);
  }
  if (passthrough && keep) {
    if (own.on) {                                                   // the records that end in the owned range, compacted on the device
      { int rcw = ensure_sort_workspace(h, n, true); if (rcw) return rcw; }
      HIP_TRY(h, owned_filter_device(src, n, own, h->d_fout, h->d_fcounts, h->stream));
      HIP_TRY(h, hipMemcpyAsync(h->h_fcounts, h->d_fcounts, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
      HIP_TRY(h, stream_wait(h));
      h->d_final = h->d_fout; h->n_final = (size_t)h->h_fcounts[0];
    } else { h->d_final = src; h->n_final = n; }
    if (n_out) *n_out = h->n_final;
    return PM_OK;
  }
  if (passthrough) {
    if (n > cap) return fail(h, PM_E_OVERFLOW, "pm_finalize_device: out buffer too small");
    if (n) HIP_TRY(h, hipMemcpyAsync(out, src, n * sizeof(pm_hit), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, stream_wait(h));
    if (own.on) n = (size_t)(std::remove_if(out, out + n, [&](const pm_hit &x) { return !(x.end > own.own_lo && x.end <= own.own_hi); }) - out);
    if (flags & PM_FINALIZE_SORTED) sort_hits(out, n);
    if (n_out) *n_out = n;
    return PM_OK;
  }
  // (the device sorts count their items in an int: a hit-dense stream can hand one range more records than that)
  if (n + h->carry.size() >= ((size_t)1 << 31)) return dense_fail(h, "pm_finalize_device, 2^31 or more candidate", n + h->carry.size());
  { int rcw = ensure_sort_workspace(h, n + h->carry.size(), true); if (rcw) return rcw; }
  { int rcp = ensure_fpat(h); if (rcp) return rcp; }
  if (cluster_dp) { int rcd = ensure_dp_tables(h); if (rcd) return rcd; }
  // candidates an earlier range left undecided (clusters that could still grow) join this batch on
  // the device: their chains continue here
  std::vector<pm_hit> hostpart;
  if (cluster_dp && h->win && !h->carry.empty()) {                 // the cluster DPs of carried records read text behind the scanned range
    const int rcw = win_need(h, carry_reach(h), h->own_end + h->win_fwd, h->bound_on, "pm_finalize_device");
    if (rcw) return rcw;
  }
  const size_t ncarry = h->carry.size();
  if (ncarry) {
    if (h->d_carry_cap < ncarry) {
      h->d_carry_cap = ncarry + ncarry / 2 + 1024;
      PM_TRY(dev_regrow(h, &h->d_carry, h->d_carry_cap * sizeof(pm_hit), "d_carry"));
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_carry, h->carry.data(), ncarry * sizeof(pm_hit), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, stream_wait(h));
    h->carry.clear();
  }
  const double tfd0 = now_ms();
  if (cluster_dp)
    HIP_TRY(h, cluster_dp_device(src, n, h->d_carry, ncarry, h->cfg.k, true, scanned_to, last, h->d_text, h->n, h->eos_code, h->d_dp_codes, h->d_fpat_len,
                                 h->d_dp_esb, h->d_dp_eeb, h->d_fpat_id, own, h->d_keys, h->d_keys_alt, h->d_ctemp, h->ctemp_bytes,
                                 h->d_fout, h->d_fleft, h->d_fcounts, h->stream, dp_row(h) == 64));
  else
  HIP_TRY(h, cluster_device(src, n, h->d_carry, ncarry, h->cfg.k, scanned_to, last, h->zoned ? 3 : -1, h->d_fpat_len, h->d_fpat_id, own, h->d_keys, h->d_keys_alt,
                            h->d_ctemp, h->ctemp_bytes, h->d_fout, h->d_fleft, h->d_fcounts, h->stream));
  bool sorted = false;
  if (land) { int rcs = land_enqueue_sort(h, h->d_fout, h->d_fcounts, n + ncarry, &sorted); if (rcs) return rcs; }
  h->h_fcounts[2] = 0;
  HIP_TRY(h, hipMemcpyAsync(h->h_fcounts, h->d_fcounts, ((n + ncarry) ? 3 : 2) * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  { int rcy = finalize_sync(h, next); if (rcy) return rcy; }
  const size_t nfin = (size_t)h->h_fcounts[0], nleft = (size_t)h->h_fcounts[1];
  if (own.on && h->h_fcounts[2])
    return fail(h, PM_E_UNSUPPORTED, "pm_finalize_device_owned: a chain of candidates reaches from the guard edge into the owned range (repeat longer than the guard band)");
  const double tfd1 = now_ms();
  if (nleft) {
    if (h->counting) h->cinfo.record_bytes_to_host += nleft * sizeof(pm_hit);
    const size_t at = hostpart.size();
    hostpart.resize(at + nleft);
    if (land) {                                                     // (the handle's stream may hold the next range's scan)
      HIP_TRY(h, hipMemcpyAsync(hostpart.data() + at, h->d_fleft, nleft * sizeof(pm_hit), hipMemcpyDeviceToHost, h->copy_stream));
      HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
    } else
    HIP_TRY(h, hipMemcpy(hostpart.data() + at, h->d_fleft, nleft * sizeof(pm_hit), hipMemcpyDeviceToHost));
  }
  std::vector<pm_hit> extra;
  if (!hostpart.empty()) {
    int rc = finalize_into(h, hostpart.data(), hostpart.size(), scanned_to, last, extra);
    if (rc) return rc;
    if (own.on) extra.erase(std::remove_if(extra.begin(), extra.end(), [&](const pm_hit &x) { return !(x.end > own.own_lo && x.end <= own.own_hi); }), extra.end());
  }
  const int rcd = deliver_finals(h, land, sorted, nfin, extra, flags, out, cap, n_out);
  if (h->knobs.debug && (land || (out && !rcd)))
    fprintf(stderr, "[pm] finalize_device%s: %zu records, device %.1f ms (%zu finals, %zu left for the host), host part + copies %.1f ms%s\n",
            land ? " (pm_scan)" : "", n, tfd1 - tfd0, nfin, nleft, now_ms() - tfd1, land && h->spec ? ", next range's scan in flight" : "");
  return rcd;
}

// primer_match's per-hit re-alignment (reference primer_match.cc:1135-1151): exact_alignment
// (pattern_alignment.cc:29-43) for k == 0, else editdist_alignment(key, key, k, eos, wc, tn,
// indels, dm, esb, eeb, yesno=false) with its traceback; editdist == INT32_MAX is the CLI's
// "Bogus hit" (constraint violation).
// none_empty: a record whose DP gives up at a row (no alignment: start = 0, editdist = INT32_MAX, value = 0) gets two empty
// strings, as pm_align_hits_kernel writes them -- the form pm_align_hits_device needs for the records it hands to the host;
// without it such a record cannot be asked for strings and the call fails (pm_align_hits_text).
static int align_hits_impl(pm_handle *h, const pm_hit *hits, size_t n, pm_alignment *out, char *ops, char *text, size_t stride, bool none_empty = false);

extern "C" int pm_align_hits(pm_handle *h, const pm_hit *hits, size_t n, pm_alignment *out) {
  return align_hits_impl(h, hits, n, out, nullptr, nullptr, 0);
}

extern "C" int pm_align_hits_text(pm_handle *h, const pm_hit *hits, size_t n, pm_alignment *out, char *ops, char *text, size_t stride) {
  if (!ops || !text || stride == 0) return fail(h, PM_E_INVALID, "pm_align_hits_text: bad arguments");
  return align_hits_impl(h, hits, n, out, ops, text, stride);
}

static int align_hits_impl(pm_handle *h, const pm_hit *hits, size_t n, pm_alignment *out, char *ops, char *text, size_t stride, bool none_empty) {
  if (!h || !h->inited || (!hits && n) || (!out && n)) return fail(h, PM_E_INVALID, "pm_align_hits: bad arguments");
  const bool wc_exact = h->cfg.wildcards && h->cfg.k == 0;      // exact_wc_alignment (pattern_alignment.cc:70-93) reads the text
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  const int k = h->cfg.k;
  std::vector<Window> wins(n);
  std::vector<const Pattern *> pp(n);
  for (size_t i = 0; i < n; ++i) {
    auto it = h->id2idx.find(hits[i].pid);
    if (it == h->id2idx.end()) return fail(h, PM_E_INVALID, "pm_align_hits: unknown pattern id");
    pp[i] = &h->pats[it->second];
    const int L = (int)pp[i]->s.size();
    int64_t ws = 0;
    if (hits[i].end > (int64_t)L + k) ws = hits[i].end - L - k;       // pattern_alignment.cc:137-139
    wins[i] = Window{ws, (k == 0 && !wc_exact) ? 0 : (int32_t)(hits[i].end - ws), 0};
  }
  if (k > 0 || wc_exact) { int rc = fetch_windows(h, wins); if (rc) return rc; }
  AlignParams prm; prm.k = k; prm.indels = h->cfg.indels != 0; prm.eos = (uint8_t)h->cfg.eos;
  prm.wc = h->cfg.wildcards != 0; prm.tn = h->cfg.text_n != 0;
  // the hits are independent: worker threads take contiguous slices (own DP scratch each)
  auto run = [&](size_t lo, size_t hi, AlignScratch &scratch) -> bool {
  for (size_t i = lo; i < hi; ++i) {
    const int L = (int)pp[i]->s.size();
    if (wc_exact) {
      // start = end - L; per character: equal, IUPAC-compatible (text N only with -W), or substitution
      const int64_t st = hits[i].end - L;
      if ((size_t)L + 1 > stride && ops) return false;
      int subs = 0;
      for (int q = 0; q < L; ++q) {
        const int64_t tp = st + q;
        const unsigned char tc = tp >= wins[i].start && tp < hits[i].end ? h->winbuf[wins[i].off + (tp - wins[i].start)] : 0;
        const unsigned char pc = (unsigned char)pp[i]->s[q];
        char op;
        if (tc == pc) op = '|';
        else {
          const char *set = tc < 128 ? iupac_compatible_set(tc) : nullptr;
          if (set && pc && strchr(set, pc) && (h->cfg.text_n || tc != 'N')) op = '+';
          else { op = '*'; ++subs; }
        }
        if (ops) { ops[i * stride + q] = op; text[i * stride + q] = (char)tc; }
      }
      if (ops) { ops[i * stride + L] = 0; text[i * stride + L] = 0; }
      out[i].start = st; out[i].end = hits[i].end; out[i].editdist = subs; out[i].value = 0;
      continue;
    }
    if (k == 0) {                                                    // exact_alignment (pattern_alignment.cc:29-43)
      out[i].start = hits[i].end - L; out[i].end = hits[i].end; out[i].editdist = 0; out[i].value = 0;
      if (ops) {
        if ((size_t)L + 1 > stride) return false;
        memset(ops + i * stride, '|', (size_t)L); ops[i * stride + L] = 0;
        memcpy(text + i * stride, pp[i]->s.data(), (size_t)L); text[i * stride + L] = 0;
      }
      continue;
    }
    std::string opstr;
    AlignResult r = editdist_align(h->winbuf.data() + wins[i].off, wins[i].start, hits[i].end, hits[i].end,
                                   pp[i]->s.data(), L, pp[i]->esb, pp[i]->eeb, prm, scratch, ops ? &opstr : nullptr);
    out[i].start = r.start; out[i].end = r.end; out[i].editdist = r.editdist; out[i].value = r.value;
    if (ops && none_empty && r.editdist == INT32_MAX && r.start == 0 && r.value == 0) {
      ops[i * stride] = 0; text[i * stride] = 0;
    } else if (ops) {
      const int64_t tl = r.end - r.start;                              // matching text (pattern_alignment.cc:603-606)
      if (opstr.size() + 1 > stride || tl < 0 || (size_t)tl + 1 > stride) return false;
      memcpy(ops + i * stride, opstr.data(), opstr.size()); ops[i * stride + opstr.size()] = 0;
      for (int64_t q = 0; q < tl; ++q) text[i * stride + q] = (char)h->winbuf[wins[i].off + (r.start - wins[i].start) + q];
      text[i * stride + tl] = 0;
    }
  }
  return true;
  };
  bool ok = true;
  const unsigned hw = std::thread::hardware_concurrency();
  const size_t nthreads = n < 4096 ? 1 : std::min<size_t>(hw ? hw : 1, 16);
  if (nthreads <= 1) ok = run(0, n, h->scratch);
  else {
    std::vector<std::thread> pool;
    std::vector<char> good(nthreads, 1);
    const size_t per = (n + nthreads - 1) / nthreads;
    for (size_t t = 0; t < nthreads; ++t)
      pool.emplace_back([&, t]() { AlignScratch sc; good[t] = run(std::min(n, t * per), std::min(n, (t + 1) * per), sc) ? 1 : 0; });
    for (std::thread &th : pool) th.join();
    for (char g : good) ok = ok && g;
  }
  if (!ok) return fail(h, PM_E_INVALID, "pm_align_hits_text: stride too small");
  return PM_OK;
}

static int scan_range(pm_handle *h, int64_t begin, int64_t end);

// ---- counts on the device ----------------------------------------------------------------------
// pm_align_hits_device re-aligns records that lie in HBM (pm_align.hip); pm_count_scan is pm_scan with the landing
// replaced: the range's final hits are re-aligned where the finalize stage left them, turned into one 64-bit key each
// (pattern index | end | re-aligned distance), and the tally kernels add them to the handle's tallies under the rule of
// primer_match.cc:1123-1247.  What the host decides (clusters at range seams and at the stream start, patterns beyond
// the device limit of the DP) is aligned by align_hits_impl and joins the same key list before the tally.

static void count_free(pm_handle *h) {
  for (void *&q : h->ad_mem) { if (q) (void)hipFree(q); q = nullptr; }
  h->ad = AlignDevice(); h->ad_ready = false; h->ad_any_long = false; h->ad_any_wide = false;
  void *cw[] = {h->d_ck, h->d_ck_alt, h->d_ck_scan, h->d_cktemp, h->d_cnt, h->d_cinfo, h->d_actr, h->d_hostq, h->d_hostq_idx, h->d_hostq2, h->d_extra};
  h->d_extra = nullptr; h->d_extra_cap = 0;
  for (void *q : cw) if (q) (void)hipFree(q);
  if (h->h_actr) (void)hipHostFree(h->h_actr);
  h->d_ck = h->d_ck_alt = h->d_ck_scan = nullptr; h->d_cktemp = nullptr; h->d_cnt = h->d_cinfo = h->d_actr = h->h_actr = nullptr;
  h->d_hostq = nullptr; h->d_hostq_idx = nullptr; h->d_hostq2 = nullptr; h->ck_cap = h->cktemp_bytes = h->cktemp_for = h->cnt_words = h->hostq_cap = 0;
  h->cnt_host.clear(); h->cnt_dev = false; h->counting = false;
}

// pm_reset: the tallies start again
static int count_clear(pm_handle *h) {
  h->cinfo = pm_count_info(); h->cnt_has_bogus = false; h->cnt_max = 0; h->counting = false; h->cnt_fed = 0;
  std::fill(h->cnt_host.begin(), h->cnt_host.end(), 0);
  if (h->d_cnt) {
    HIP_TRY(h, hipMemsetAsync(h->d_cnt, 0, h->cnt_words * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_cinfo, 0, 3 * sizeof(unsigned long long), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->d_cinfo + 3, 0xff, sizeof(unsigned long long), h->stream));
    HIP_TRY(h, stream_wait(h));
  }
  return PM_OK;
}

// is the whole stream in HBM (pm_init, pm_init_device, pm_init_packed resident)?
static bool stream_resident(const pm_handle *h) { return !h->host_only && h->win == 0 && (h->d_text || h->n == 0); }

static int ensure_align_tables(pm_handle *h) {
  if (h->ad_ready) return PM_OK;
  const size_t np = h->pats.size();
  std::vector<uint8_t> tab(ALIGN_TAB_BYTES), chars;
  std::vector<uint32_t> off(np + 1, 0), ids(np), perm(np), rank(np);
  std::vector<int32_t> esb(np), eeb(np);
  align_tables(h->alpha, tab.data());
  h->ad_any_long = false;
  bool any_wide = false;                                            // a pattern in reach of pm_align_hits_wide_kernel
  for (size_t i = 0; i < np; ++i) {
    const Pattern &p = h->pats[i];
    chars.insert(chars.end(), p.s.begin(), p.s.end());
    off[i + 1] = (uint32_t)chars.size();
    esb[i] = p.esb; eeb[i] = p.eeb; perm[i] = (uint32_t)i;
    if (h->cfg.k > 0 && (p.s.size() > (size_t)AL_MAXL || p.s.empty())) h->ad_any_long = true;
    if (p.s.size() > (size_t)AL_MAXL && p.s.size() <= (size_t)AL_MAXL_WIDE) any_wide = true;
  }
  if (h->cfg.k > AL_MAXK) h->ad_any_long = true;
  h->ad_any_wide = any_wide && (h->cfg.long_patterns & PM_LONG_ALIGN) && h->cfg.indels && h->cfg.k >= 1 && h->cfg.k <= AL_MAXK;
  const size_t nctr = h->ad_any_wide ? 4 : 3;
  // pattern ids in increasing order; of equal ids the pattern added last, as id2idx resolves them
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return h->pats[x].id < h->pats[y].id; });
  for (size_t r = 0; r < np; ++r) {
    ids[r] = (uint32_t)h->pats[perm[r]].id;
    const auto it = h->id2idx.find(ids[r]);
    if (it != h->id2idx.end()) perm[r] = it->second;
  }
  for (size_t r = 0; r < np; ++r) rank[perm[r]] = (uint32_t)r;
  const void *src[8] = {tab.data(), chars.data(), off.data(), esb.data(), eeb.data(), ids.data(), perm.data(), rank.data()};
  const size_t bytes[8] = {tab.size(), chars.size(), off.size() * 4, np * 4, np * 4, np * 4, np * 4, np * 4};
  for (int i = 0; i < 8; ++i) PM_TRY(dev_upload(h, &h->ad_mem[i], src[i], bytes[i], 4, "ad_mem"));
  AlignDevice &a = h->ad;
  a.tab = (const uint8_t *)h->ad_mem[0]; a.pchars = (const uint8_t *)h->ad_mem[1]; a.poff = (const uint32_t *)h->ad_mem[2];
  a.esb = (const int32_t *)h->ad_mem[3]; a.eeb = (const int32_t *)h->ad_mem[4];
  a.ids_sorted = (const uint32_t *)h->ad_mem[5]; a.perm = (const uint32_t *)h->ad_mem[6]; a.idrank = (const uint32_t *)h->ad_mem[7];
  a.npat = (uint32_t)np; a.k = h->cfg.k; a.indels = h->cfg.indels != 0; a.eos = (uint8_t)h->cfg.eos;
  a.wc = h->cfg.wildcards != 0; a.tn = h->cfg.text_n != 0;
  if (!h->d_actr) HIP_TRY(h, hipMalloc((void **)&h->d_actr, nctr * sizeof(unsigned long long)));
  if (!h->h_actr) HIP_TRY(h, hipHostMalloc((void **)&h->h_actr, nctr * sizeof(unsigned long long), hipHostMallocDefault));
  h->ad_ready = true;
  return PM_OK;
}

extern "C" int pm_align_hits_device(pm_handle *h, const void *d_hits, size_t n, void *d_out, void *d_ops, void *d_text, size_t stride) {
  if (!h || !h->inited || (n && (!d_hits || !d_out))) return fail(h, PM_E_INVALID, "pm_align_hits_device: bad arguments");
  if ((d_ops != nullptr) != (d_text != nullptr) || (d_ops && stride == 0)) return fail(h, PM_E_INVALID, "pm_align_hits_device: d_ops and d_text come together, with a stride");
  if (n == 0) return PM_OK;
  if (n >= ((size_t)1 << 31)) return fail(h, PM_E_INVALID, "pm_align_hits_device: 2^31 records or more in one call");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  const bool strings = d_ops != nullptr;
  if (!stream_resident(h)) {                                        // the stream is not in HBM as a whole: the host aligns every record
    std::vector<pm_hit> all(n);
    HIP_TRY(h, hipMemcpy(all.data(), d_hits, n * sizeof(pm_hit), hipMemcpyDeviceToHost));
    h->cinfo.record_bytes_to_host += n * sizeof(pm_hit);
    std::vector<pm_alignment> al(n);
    std::vector<char> ho, ht;
    if (strings) { ho.assign(n * stride, 0); ht.assign(n * stride, 0); }
    { int rc = align_hits_impl(h, all.data(), n, al.data(), strings ? ho.data() : nullptr, strings ? ht.data() : nullptr, stride, true); if (rc) return rc; }
    h->cinfo.aligned_host += n;
    HIP_TRY(h, hipMemcpy(d_out, al.data(), n * sizeof(pm_alignment), hipMemcpyHostToDevice));
    if (strings) {
      HIP_TRY(h, hipMemcpy(d_ops, ho.data(), n * stride, hipMemcpyHostToDevice));
      HIP_TRY(h, hipMemcpy(d_text, ht.data(), n * stride, hipMemcpyHostToDevice));
    }
    return PM_OK;
  }
  { int rc = ensure_align_tables(h); if (rc) return rc; }
  // records of patterns beyond the device limit: the kernel compacts them and their indices; only they cross to the host
  // and only their results are written back (pm_align_scatter)
  // (PM_LONG_ALIGN: that list is the wide kernel's input, still on the device, and the list the wide kernel leaves -- d_rec2 /
  // d_idx2, counted in d_actr[3] -- is what crosses)
  const bool wide = h->ad_any_wide;
  uint64_t *d_idx = nullptr, *d_idx2 = nullptr;
  pm_hit *d_rec = nullptr, *d_rec2 = nullptr;
  void *d_back = nullptr;
  auto release = [&]() { void *q[] = {d_idx, d_rec, d_idx2, d_rec2, d_back}; for (void *x : q) if (x) (void)hipFree(x); };
  if (h->ad_any_long) {
    hipError_t ea = hipMalloc((void **)&d_idx, n * sizeof(uint64_t));
    if (ea == hipSuccess) ea = hipMalloc((void **)&d_rec, n * sizeof(pm_hit));
    if (ea == hipSuccess && wide) ea = hipMalloc((void **)&d_idx2, n * sizeof(uint64_t));
    if (ea == hipSuccess && wide) ea = hipMalloc((void **)&d_rec2, n * sizeof(pm_hit));
    if (ea != hipSuccess) { release(); return hipfail(h, ea, "pm_align_hits_device"); }
  }
  hipError_t e = align_hits_device(h->ad, h->d_text, h->n, (const pm_hit *)d_hits, nullptr, n, (pm_alignment *)d_out, (char *)d_ops, (char *)d_text, stride,
                                   nullptr, d_rec, d_idx, h->d_actr, h->stream);
  if (e == hipSuccess && wide)
    e = align_hits_wide_device(h->ad, h->d_text, h->n, d_rec, d_idx, n, (pm_alignment *)d_out, (char *)d_ops, (char *)d_text, stride, nullptr, d_rec2, d_idx2,
                               h->d_actr, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(h->h_actr, h->d_actr, (wide ? 4 : 3) * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = stream_wait(h);
  if (e != hipSuccess) { release(); return hipfail(h, e, "pm_align_hits_device"); }
  const size_t m = (size_t)h->h_actr[wide ? 3 : 0];
  if (wide) { std::swap(d_rec, d_rec2); std::swap(d_idx, d_idx2); }   // the list that crosses
  int rc = PM_OK;
  if (h->h_actr[1]) rc = fail(h, PM_E_INVALID, "pm_align_hits_device: unknown pattern id");
  else if (h->h_actr[2]) rc = fail(h, PM_E_INVALID, "pm_align_hits_device: stride too small");
  h->cinfo.aligned_device += n - m;
  if (rc == PM_OK && m) {
    std::vector<pm_hit> hh(m);
    std::vector<pm_alignment> al(m);
    std::vector<char> ho, ht;
    if (strings) { ho.assign(m * stride, 0); ht.assign(m * stride, 0); }
    e = hipMemcpy(hh.data(), d_rec, m * sizeof(pm_hit), hipMemcpyDeviceToHost);
    h->cinfo.record_bytes_to_host += m * sizeof(pm_hit);
    if (e == hipSuccess) rc = align_hits_impl(h, hh.data(), m, al.data(), strings ? ho.data() : nullptr, strings ? ht.data() : nullptr, stride, true);
    if (e == hipSuccess && rc == PM_OK) {
      h->cinfo.aligned_host += m;
      const size_t ab = m * sizeof(pm_alignment), sb = strings ? m * stride : 0;
      e = hipMalloc(&d_back, ab + 2 * sb);
      char *back = (char *)d_back;
      if (e == hipSuccess) e = hipMemcpy(back, al.data(), ab, hipMemcpyHostToDevice);
      if (e == hipSuccess && strings) e = hipMemcpy(back + ab, ho.data(), sb, hipMemcpyHostToDevice);
      if (e == hipSuccess && strings) e = hipMemcpy(back + ab + sb, ht.data(), sb, hipMemcpyHostToDevice);
      if (e == hipSuccess) e = align_scatter_device(d_idx, m, (const pm_alignment *)back, strings ? back + ab : nullptr, strings ? back + ab + sb : nullptr, stride,
                                                    (pm_alignment *)d_out, (char *)d_ops, (char *)d_text, h->stream);
      if (e == hipSuccess) e = stream_wait(h);
    }
    if (e != hipSuccess) rc = hipfail(h, e, "pm_align_hits_device");
  }
  release();
  return rc;
}

static bool count_tally_on_device(const pm_handle *h) {
  return !h->host_only && h->cfg.k <= AL_MAXK && h->pats.size() < (size_t)TALLY_MAXPAT && (uint64_t)h->n + 512 < (1ull << 39);
}

// room for `need` tally keys (the first `keep` stay) and the workspaces of a tally over that many
static int ensure_count_keys(pm_handle *h, size_t need, size_t keep) {
  if (h->ck_cap < need) {
    const size_t cap = std::max<size_t>(need + need / 4, (size_t)1 << 16);
    uint64_t *nk = nullptr;
    HIP_TRY(h, hipMalloc((void **)&nk, cap * 8));
    if (keep) HIP_TRY(h, hipMemcpy(nk, h->d_ck, keep * 8, hipMemcpyDeviceToDevice));
    void *old[] = {h->d_ck, h->d_ck_alt, h->d_ck_scan};
    for (void *q : old) if (q) (void)hipFree(q);
    h->d_ck = nk; h->d_ck_alt = h->d_ck_scan = nullptr; h->ck_cap = cap;
    HIP_TRY(h, hipMalloc((void **)&h->d_ck_alt, cap * 8));
    HIP_TRY(h, hipMalloc((void **)&h->d_ck_scan, cap * 8));
  }
  if (h->cktemp_for < h->ck_cap) {
    h->cktemp_bytes = tally_temp_bytes(h->ck_cap);
    PM_TRY(dev_regrow(h, &h->d_cktemp, h->cktemp_bytes ? h->cktemp_bytes : 16, "d_cktemp"));
    h->cktemp_for = h->ck_cap;
  }
  return PM_OK;
}

static int ensure_count_state(pm_handle *h) {
  const size_t words = std::max<size_t>(h->pats.size() * (size_t)(h->cfg.k + 1), 1);
  h->cnt_dev = count_tally_on_device(h);
  if (!h->cnt_dev) { if (h->cnt_host.size() != words) h->cnt_host.assign(words, 0); return PM_OK; }
  { int rc = ensure_align_tables(h); if (rc) return rc; }
  if (!h->d_cnt) {
    HIP_TRY(h, hipMalloc((void **)&h->d_cnt, words * sizeof(unsigned long long)));
    HIP_TRY(h, hipMalloc((void **)&h->d_cinfo, 4 * sizeof(unsigned long long)));
    h->cnt_words = words;
    const pm_count_info keep = h->cinfo;                            // (count_clear also clears the host's share)
    const uint64_t keep_max = h->cnt_max;
    const int rc = count_clear(h);
    h->cinfo = keep; h->cnt_max = keep_max;
    if (rc) return rc;
  }
  return PM_OK;
}

// room for `need` records in the list the feed kernel leaves (and, with the wide kernel behind it, for their indices and
// for the list that kernel leaves in its turn)
static int ensure_hostq(pm_handle *h, size_t need, size_t cap) {
  if (!h->ad_any_long || h->hostq_cap >= need) return PM_OK;
  h->hostq_cap = 0;
  PM_TRY(dev_regrow(h, &h->d_hostq, cap * sizeof(pm_hit), "d_hostq"));
  if (h->ad_any_wide) {
    PM_TRY(dev_regrow(h, &h->d_hostq_idx, cap * sizeof(uint64_t), "d_hostq_idx"));
    PM_TRY(dev_regrow(h, &h->d_hostq2, cap * sizeof(pm_hit), "d_hostq2"));
  }
  h->hostq_cap = cap;
  return PM_OK;
}

// the records' tally keys -> d_keys[0 .. n_upper), on the handle's stream: the feed kernel, behind it the wide kernel over the
// list the feed kernel left (PM_LONG_ALIGN; no host step in between), then the counters' copy to h_actr.  The records for
// the host are count_hostq(h) records at count_hostq_list(h) once the stream has got there.
static int count_align(pm_handle *h, const pm_hit *d_hits, const unsigned long long *d_count, size_t n_upper, uint64_t *d_keys) {
  const bool wide = h->ad_any_wide;
  HIP_TRY(h, align_hits_device(h->ad, h->d_text, h->n, d_hits, d_count, n_upper, nullptr, nullptr, nullptr, 0, d_keys,
                               h->ad_any_long ? h->d_hostq : nullptr, wide ? h->d_hostq_idx : nullptr, h->d_actr, h->stream));
  if (wide)
    HIP_TRY(h, align_hits_wide_device(h->ad, h->d_text, h->n, h->d_hostq, h->d_hostq_idx, n_upper, nullptr, nullptr, nullptr, 0, d_keys,
                                      h->d_hostq2, nullptr, h->d_actr, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->h_actr, h->d_actr, (wide ? 4 : 3) * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  return PM_OK;
}
static size_t count_hostq(const pm_handle *h) { return (size_t)h->h_actr[h->ad_any_wide ? 3 : 0]; }
static const pm_hit *count_hostq_list(const pm_handle *h) { return h->ad_any_wide ? h->d_hostq2 : h->d_hostq; }

// the device's finals of one range -> tally keys d_ck[0 .. count), before the host knows their number
static int count_feed_device(pm_handle *h, const pm_hit *d_hits, const unsigned long long *d_count, size_t n_upper) {
  h->cnt_fed = 0;
  if (n_upper == 0) return PM_OK;
  // (cannot happen: the finalize stage in front refuses 2^31 records before it touches the engine's state; not a reason to cut the range)
  if (n_upper >= ((size_t)1 << 31)) return fail(h, PM_E_INVALID, "pm_count_scan: internal: 2^31 or more final hits in one range");
  { int rc = ensure_count_keys(h, n_upper + ((size_t)1 << 12), 0); if (rc) return rc; }
  { int rc = ensure_hostq(h, n_upper, n_upper + n_upper / 4); if (rc) return rc; }
  { int rc = count_align(h, d_hits, d_count, n_upper, h->d_ck); if (rc) return rc; }
  h->cnt_fed = n_upper;
  return PM_OK;
}

static uint64_t host_tally_key(uint32_t idx, int64_t end, int code) {
  return ((uint64_t)idx << 42) | (((uint64_t)end & ((1ull << 39) - 1ull)) << 3) | (uint64_t)code;
}

// The tally of primer_match.cc:1123-1247 on the host, for handles whose tallies do not fit the device keys: hits of one
// pattern in order of stream end (the list is in (end, pid, k) order)
static void count_host_tally(pm_handle *h, const pm_hit *hits, const pm_alignment *al, size_t m) {
  const int k = h->cfg.k;
  for (size_t j = 0; j < m; ++j) {
    const size_t idx = h->id2idx.find(hits[j].pid)->second;
    uint64_t total = 0;
    for (int d = 0; d <= k; ++d) total += h->cnt_host[idx * (k + 1) + d];
    if (h->cnt_max && total >= h->cnt_max) { ++h->cinfo.skipped; continue; }
    if (al[j].editdist < 0 || al[j].editdist > k) {
      ++h->cinfo.bogus;
      if (!h->cnt_has_bogus || by_end_pid(hits[j], h->cinfo.first_bogus)) { h->cinfo.first_bogus = make_hit(hits[j].end, hits[j].pid, 0); h->cnt_has_bogus = true; }
      continue;
    }
    ++h->cnt_host[idx * (k + 1) + al[j].editdist];
    ++h->cinfo.tallied;
  }
}

// records the host aligns (in (end, pid, k) order) -> keys behind the `at` keys the device made, or the host tally
static int count_host_records(pm_handle *h, const pm_hit *hits, size_t m, size_t at) {
  if (m == 0) return PM_OK;
  std::vector<pm_alignment> al(m);
  { int rc = align_hits_impl(h, hits, m, al.data(), nullptr, nullptr, 0); if (rc) return rc; }
  h->cinfo.aligned_host += m;
  if (!h->cnt_dev) { count_host_tally(h, hits, al.data(), m); return PM_OK; }
  std::vector<uint64_t> keys(m);
  for (size_t j = 0; j < m; ++j)
    keys[j] = host_tally_key(h->id2idx.find(hits[j].pid)->second, hits[j].end, (al[j].editdist < 0 || al[j].editdist > h->cfg.k) ? TALLY_BOGUS : al[j].editdist);
  { int rc = ensure_count_keys(h, at + m, at); if (rc) return rc; }
  HIP_TRY(h, hipMemcpy(h->d_ck + at, keys.data(), m * 8, hipMemcpyHostToDevice));
  return PM_OK;
}

// sort + tally of the `n` keys at d_ck on the handle's stream (behind the next range's scan when pm_scan's pipeline has
// enqueued it: nothing the tally reads or writes is touched by a scan)
static int count_flush(pm_handle *h, size_t n) {
  if (n == 0 || !h->cnt_dev) return PM_OK;
  if (n >= ((size_t)1 << 31)) return fail(h, PM_E_INVALID, "pm_count_scan: internal: 2^31 or more tally keys in one range");
  HIP_TRY(h, tally_device(h->ad, h->d_ck, h->d_ck_alt, h->d_ck_scan, n, h->d_cktemp, h->cktemp_bytes, h->cnt_max, h->d_cnt, h->d_cinfo, h->stream));
  return PM_OK;
}

// pm_count_scan's landing: nfin finals were turned into keys by count_feed_device (the finalize stage is done: its
// counters are on the host); `extra`, the hits of the range that the host rules decided, are uploaded and go through the
// same kernel.  Only records of patterns beyond the device limit of the DP are aligned on the host.
static int count_collect(pm_handle *h, size_t nfin, std::vector<pm_hit> &extra, size_t *n_out) {
  if (n_out) *n_out = nfin + extra.size();
  if (h->cnt_fed == 0) nfin = 0;
  h->cnt_fed = 0;
  std::vector<pm_hit> rest;
  auto take_hostq = [&](size_t nq) -> int {                         // (the handle's stream may hold the next range's scan)
    if (!nq) return PM_OK;
    const size_t at = rest.size();
    rest.resize(at + nq);
    HIP_TRY(h, hipMemcpyAsync(rest.data() + at, count_hostq_list(h), nq * sizeof(pm_hit), hipMemcpyDeviceToHost, h->copy_stream));
    HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
    h->cinfo.record_bytes_to_host += nq * sizeof(pm_hit);
    return PM_OK;
  };
  if (nfin) {
    if (h->h_actr[1]) return fail(h, PM_E_INVALID, "pm_count_scan: a final hit with an unknown pattern id");
    const size_t nq = count_hostq(h);
    { int rc = take_hostq(nq); if (rc) return rc; }
    h->cinfo.aligned_device += nfin - nq;
  }
  const size_t m = extra.size();
  if (m) {
    { int rc = ensure_count_keys(h, nfin + 2 * m + ((size_t)1 << 12), nfin); if (rc) return rc; }
    if (h->d_extra_cap < m) {
      h->d_extra_cap = std::max<size_t>(2 * m, (size_t)1 << 12);
      PM_TRY(dev_regrow(h, &h->d_extra, h->d_extra_cap * sizeof(pm_hit), "d_extra"));
    }
    { int rc = ensure_hostq(h, m, std::max<size_t>(2 * m, (size_t)1 << 12)); if (rc) return rc; }
    HIP_TRY(h, hipMemcpy(h->d_extra, extra.data(), m * sizeof(pm_hit), hipMemcpyHostToDevice));
    { int rc = count_align(h, h->d_extra, nullptr, m, h->d_ck + nfin); if (rc) return rc; }
    HIP_TRY(h, stream_wait(h));
    if (h->h_actr[1]) return fail(h, PM_E_INVALID, "pm_count_scan: a final hit with an unknown pattern id");
    const size_t nq = count_hostq(h);
    { int rc = take_hostq(nq); if (rc) return rc; }
    h->cinfo.aligned_device += m - nq;
  }
  for (pm_hit &x : rest) x.aux[0] = x.aux[1] = x.aux[2] = 0;
  sort_hits(rest.data(), rest.size());
  { int rc = count_host_records(h, rest.data(), rest.size(), nfin + m); if (rc) return rc; }
  return count_flush(h, nfin + m + rest.size());
}

extern "C" int pm_count_scan(pm_handle *h, int64_t begin, int64_t end, uint64_t max_count) {
  if (!h || !h->inited) return fail(h, PM_E_INVALID, "pm_count_scan: handle not initialised");
  if (h->host_only) return fail(h, PM_E_INVALID, "pm_count_scan: this handle runs the host stage only");
  if (h->scan_mode == 1) return fail(h, PM_E_INVALID, "pm_count_scan after pm_scan (pm_reset first)");
  if (h->scan_mode == 3) return fail(h, PM_E_INVALID, "pm_count_scan after pm_pcr_scan (pm_reset first)");
  if (h->scan_mode == 2 && max_count != h->cnt_max) return fail(h, PM_E_INVALID, "pm_count_scan: max_count changed between two pm_reset()s");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  h->scan_mode = 2; h->cnt_max = max_count;
  { int rc = ensure_count_state(h); if (rc) return rc; }
  if (end > h->n) end = h->n;
  if (end <= begin) return PM_OK;
  // the finals stay on the device when the whole stream is there for the re-alignment; otherwise the range lands as for
  // pm_scan and the host aligns its hits (the tally is the same)
  h->counting = h->cnt_dev && stream_resident(h);
  const bool on_device = h->counting;
  const int rc = scan_range(h, begin, end);
  h->counting = false;
  if (rc) return rc;
  if (!on_device) {
    const pm_hit *hits = h->land + h->land_pos;
    const size_t m = h->land_n - h->land_pos;
    h->cinfo.record_bytes_to_host += m * sizeof(pm_hit);
    { int rc2 = count_host_records(h, hits, m, 0); if (rc2) return rc2; }
    h->land_pos = h->land_n = 0;
    { int rc2 = count_flush(h, m); if (rc2) return rc2; }
  }
  HIP_TRY(h, stream_wait(h));
  return PM_OK;
}

extern "C" int pm_counts(pm_handle *h, uint64_t *counts, uint8_t *capped, size_t npat, pm_count_info *info) {
  if (!h || !h->inited) return fail(h, PM_E_INVALID, "pm_counts: handle not initialised");
  if (!counts || npat != h->pats.size()) return fail(h, PM_E_INVALID, "pm_counts: counts must hold (k + 1) values for every added pattern");
  const int k = h->cfg.k;
  const size_t words = npat * (size_t)(k + 1);
  pm_count_info out = h->cinfo;
  if (!h->cnt_has_bogus) out.first_bogus = make_hit(0, 0, 0);
  memset(counts, 0, words * sizeof(uint64_t));
  if (h->d_cnt && h->cnt_dev) {
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    unsigned long long di[4];
    HIP_TRY(h, stream_wait(h));
    if (words) HIP_TRY(h, hipMemcpy(counts, h->d_cnt, words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(di, h->d_cinfo, sizeof(di), hipMemcpyDeviceToHost));
    out.tallied += di[0]; out.skipped += di[1]; out.bogus += di[2];
    if (di[3] != ~0ull) {
      uint32_t pid = 0;
      HIP_TRY(h, hipMemcpy(&pid, h->ad.ids_sorted + (di[3] & 0x3fffffu), 4, hipMemcpyDeviceToHost));
      out.first_bogus = make_hit((int64_t)(di[3] >> 22), pid, 0);
    }
  } else if (h->cnt_host.size() == words) {
    for (size_t i = 0; i < words; ++i) counts[i] = h->cnt_host[i];
  }
  if (capped)
    for (size_t i = 0; i < npat; ++i) {
      uint64_t total = 0;
      for (int d = 0; d <= k; ++d) total += counts[i * (k + 1) + d];
      capped[i] = h->cnt_max && total >= h->cnt_max ? 1 : 0;
    }
  if (info) *info = out;
  return PM_OK;
}

// One range of PatternMatch::find_patterns: scan, finalize, final hits in (end, pid, k) order behind whatever the landing
// buffer still holds.  With a device finalize stage the scan of the range expected next -- the same number of stream
// bytes, the way the reference's callers walk a stream chunk by chunk -- is already on the GPU when this returns.
static int scan_piece(pm_handle *h, int64_t begin, int64_t end) {
  if (begin != h->next_begin) return fail(h, PM_E_INVALID, "pm_scan: ranges must be consecutive (pm_reset to restart)");
  size_t cnt = 0;
  int rc;
  h->too_dense = false;
  if (h->spec && h->spec_b == begin && h->spec_e == end && h->scan_pending) { h->spec = false; rc = pm_scan_wait(h, &cnt); }
  else rc = pm_scan_candidates(h, begin, end, nullptr, 0, &cnt);       // (drains a speculative scan of another range)
  while (rc == PM_E_OVERFLOW && cnt > h->cap) {                     // grow and redo this range
    if (cnt > dense_bound(h)) return dense_fail(h, "candidate records", cnt);
    rc = ensure_capacity(h, cnt + cnt / 4 + 1024);
    if (rc) return rc;
    rc = pm_scan_candidates(h, begin, end, nullptr, 0, &cnt);
  }
  if (rc) return rc;
  // pm_scan's own conditions: the halves rule needs the whole stream on a fresh state, plain clustering the seed kernels' records
  const Route route = finalize_route(h);
  const bool halves_whole = begin == 0 && end >= h->n && h->halves_fresh && h->carry.empty();
  if (route == Route::Passthrough || route == Route::ClusterDp || (route == Route::Halves && halves_whole) ||
      (route == Route::Cluster && h->kern == PM_KERNEL_SEED)) {
    // sort, clusters and their DPs on the device; only what it hands back goes through the host stage
    ScanNext next = {end < h->n && !h->dense_mode, end, std::min<int64_t>(h->n, end + (end - begin))};   // (no guess after a cut: the pieces are not the caller's ranges)
    const OwnedRange all = {0, 0, 0, 0, 0};
    rc = finalize_device_impl(h, nullptr, 0, end, end >= h->n ? PM_FINALIZE_LAST : 0, all, nullptr, 0, nullptr, &next);
    if (rc) return rc;
  } else {
    std::vector<pm_hit> cands(cnt), outv;
    if (cnt) HIP_TRY(h, hipMemcpy(cands.data(), h->d_cands, cnt * sizeof(pm_hit), hipMemcpyDeviceToHost));
    rc = finalize_into(h, cands.data(), cnt, end, end >= h->n, outv);
    if (rc) return rc;
    sort_hits(outv.data(), outv.size());
    if (h->counting) {                                                // (the records were finalized on the host: all of them are `extra`)
      h->cinfo.record_bytes_to_host += cnt * sizeof(pm_hit);
      h->cnt_fed = 0;
      rc = count_collect(h, 0, outv, nullptr);
      if (rc) return rc;
      h->next_begin = end;
      return PM_OK;
    }
    if (h->pcr_scanning) {                                            // (finalized on the host: the hits are uploaded to the held list)
      h->pcr_fed = 0;
      rc = pcr_collect(h, 0, outv, nullptr);
      if (rc) return rc;
      h->next_begin = end;
      return PM_OK;
    }
    rc = ensure_landing(h, outv.size());
    if (rc) return rc;
    if (!outv.empty()) memcpy(h->land + h->land_n, outv.data(), outv.size() * sizeof(pm_hit));
    h->land_n += outv.size();
  }
  h->next_begin = end;
  return PM_OK;
}

// A range whose lists would outgrow the bound (hit-dense text: DESIGN 7c) is not grown for but scanned in pieces: consecutive
// ranges give the hits of the whole (filter_bitvec.cc:118-121: what a range cannot decide yet waits for the next), so the
// answer does not change; memory stays bounded and so does the 2^31-item limit of the device sorts.  The piece length halves
// when a piece was too dense (that attempt is thrown away: every check sits before the finalize stage touches the engine's
// state), stays for the ranges that follow -- text that was dense a moment ago mostly still is -- and doubles again after
// a piece whose lists stayed under a quarter of the bound.
static int scan_range(pm_handle *h, int64_t begin, int64_t end) {
  const size_t before = h->land_n - h->land_pos;                    // (ensure_landing may move the live hits to the front of the buffer)
  int pieces = 0;
  for (int64_t pos = begin; pos < end;) {
    int64_t len = h->piece_len ? std::min<int64_t>(h->piece_len, end - pos) : end - pos;
    if (h->win) len = std::min(len, win_piece_cap(h));             // windowed: a piece and its halo fit one window
    h->dense_mode = len < end - begin;                              // (no guess of the next range while in pieces: they are not the caller's ranges)
    h->bound_on = true;
    const int rc = scan_piece(h, pos, pos + len);
    h->bound_on = false;
    if (rc != PM_OK) {
      if (!h->too_dense || len <= 256) return rc;                   // (the message says what was too many)
      h->piece_len = std::max<int64_t>(256, len / 2);
      ++h->range_splits;
      drain_spec(h);
      if (h->knobs.debug) fprintf(stderr, "[pm] pm_scan: (%lld, %lld] in pieces of %lld: %s\n", (long long)pos, (long long)(pos + len), (long long)h->piece_len, h->err.c_str());
      continue;
    }
    pos += len;
    ++pieces;
    if (h->piece_len && len == h->piece_len && h->last_peak < dense_bound(h) / 4) {   // (a full piece: the short one at the end of a range says nothing)
      h->piece_len *= 2;
      if (h->piece_len >= end - begin) h->piece_len = 0;            // whole ranges again
    }
  }
  if (pieces > 1)                                                   // the pieces' hits, each in order, as one run in (end, pid, k) order
    sort_hits(h->land + h->land_pos + before, h->land_n - h->land_pos - before);
  h->dense_mode = false;
  return PM_OK;
}

extern "C" int pm_scan(pm_handle *h, int64_t begin, int64_t end, pm_hit *out, size_t cap, size_t *n_out, int *more) {
  if (!h || !h->inited) return fail(h, PM_E_INVALID, "pm_scan: handle not initialised");
  if (n_out) *n_out = 0;
  if (more) *more = 0;
  if (h->scan_mode == 2) return fail(h, PM_E_INVALID, "pm_scan after pm_count_scan (pm_reset first)");
  if (h->scan_mode == 3) return fail(h, PM_E_INVALID, "pm_scan after pm_pcr_scan (pm_reset first)");
  h->scan_mode = 1;
  if (end > h->n) end = h->n;
  if (end > begin) { const int rc = scan_range(h, begin, end); if (rc) return rc; }
  const size_t avail = h->land_n - h->land_pos;
  const size_t take = out ? std::min(avail, cap) : 0;
  if (take) memcpy(out, h->land + h->land_pos, take * sizeof(pm_hit));
  h->land_pos += take;
  if (h->land_pos == h->land_n) h->land_pos = h->land_n = 0;
  if (n_out) *n_out = take;
  if (more) *more = h->land_pos < h->land_n;
  return PM_OK;
}

extern "C" int pm_scan_view(pm_handle *h, int64_t begin, int64_t end, const pm_hit **hits, size_t *n) {
  if (!h || !h->inited || !hits || !n) return fail(h, PM_E_INVALID, "pm_scan_view: bad arguments");
  *hits = nullptr; *n = 0;
  if (h->scan_mode == 2) return fail(h, PM_E_INVALID, "pm_scan_view after pm_count_scan (pm_reset first)");
  if (h->scan_mode == 3) return fail(h, PM_E_INVALID, "pm_scan_view after pm_pcr_scan (pm_reset first)");
  h->scan_mode = 1;
  if (end > h->n) end = h->n;
  if (h->land_pos == h->land_n) h->land_pos = h->land_n = 0;       // the span of the last call is given up
  if (end > begin) { const int rc = scan_range(h, begin, end); if (rc) return rc; }
  *hits = h->land + h->land_pos;
  *n = h->land_n - h->land_pos;
  h->land_pos = h->land_n;                                          // handed out; the memory stays valid until the next call
  return PM_OK;
}

// ---- pcr_match's pairing stage on the device ---------------------------------------------------
// The held list d_held[0 .. held_n) is what the host loop keeps in its pattern_hit_vector: pm_pcr_scan lands a range's
// finals behind it (one more landing beside pm_scan's and pm_count_scan's), pm_pcr_feed uploads records, pm_pcr_pair runs
// one round of pcr_match.cc:987-1259 over it and leaves the deferred hits at its front.

// (the records cross the ABI and ctypes by layout: tests/test_pcr_abi.py pins the same numbers on the Python side)
static_assert(sizeof(pm_pcr_amplicon) == 96 && sizeof(pm_pcr_params) == 64, "pm_gpu.h: the layout of pm_pcr_amplicon / pm_pcr_params is part of ABI v1");

static void pcr_free(pm_handle *h) {
  for (void *&q : h->pcr_mem) { if (q) (void)hipFree(q); q = nullptr; }
  void *dv[] = {h->d_held, h->d_pcr_a, h->d_pcr_b, h->d_pcr_c};
  for (void *q : dv) if (q) (void)hipFree(q);
  if (h->pcr_out) (void)hipHostFree(h->pcr_out);
  if (h->pcr_h_tot) (void)hipHostFree(h->pcr_h_tot);
  h->d_held = nullptr; h->d_pcr_a = h->d_pcr_b = h->d_pcr_c = nullptr; h->pcr_out = nullptr; h->pcr_h_tot = nullptr;
  h->held_cap = h->held_n = h->pcr_fed = h->pcr_a_bytes = h->pcr_b_bytes = h->pcr_c_bytes = h->pcr_out_bytes = 0;
  h->pcr = PcrDevice(); h->pcr_on = false; h->pcr_scanning = false;
}

static int bits_for(uint64_t v) { int b = 1; while (b < 64 && (v >> b)) ++b; return b; }

extern "C" int pm_pcr_setup(pm_handle *h, const pm_pcr_params *p) {
  if (!h || !p) return fail(h, PM_E_INVALID, "pm_pcr_setup: no handle or no parameters");
  // (what the patterns and the parameters alone decide comes first: these answers need no device)
  const size_t np = h->pats.size();
  if (np == 0 || np % 4 != 0) return fail(h, PM_E_INVALID, "pm_pcr_setup: needs 2n patterns with n even: the primers of the pairs, then their reverse complements");
  for (size_t i = 0; i < np; ++i)
    if (h->pats[i].id != i + 1) return fail(h, PM_E_INVALID, "pm_pcr_setup: the patterns must have been added with ids 1..2n in order");
  if (p->amplicon_min < 0) return fail(h, PM_E_INVALID, "pm_pcr_setup: amplicon_min must not be negative");
  if ((p->size_lb != nullptr) != (p->size_ub != nullptr)) return fail(h, PM_E_INVALID, "pm_pcr_setup: size_lb and size_ub come together");
  if (p->n_entries < 0 || (p->n_entries && !p->entry_starts)) return fail(h, PM_E_INVALID, "pm_pcr_setup: entry_starts missing");
  for (int64_t i = 1; i < p->n_entries; ++i)
    if (p->entry_starts[i] < p->entry_starts[i - 1]) return fail(h, PM_E_INVALID, "pm_pcr_setup: entry_starts must not decrease");
  if (!h->inited) return fail(h, PM_E_INVALID, "pm_pcr_setup: handle not initialised (call it after pm_init)");
  if (h->host_only || h->win != 0 || !(h->d_text || h->n == 0))
    return fail(h, PM_E_UNSUPPORTED, "pm_pcr_setup: the pairing stage needs the whole stream in HBM (not a windowed or host-only handle)");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  const int cur_mode = h->scan_mode;
  pcr_free(h);
  PcrDevice &d = h->pcr;
  d.rule.n = np / 2;
  d.rule.any_orientation = p->any_orientation != 0; d.rule.length_between = p->length_between != 0;
  d.rule.amplicon_min = p->amplicon_min; d.rule.amplicon_max = p->amplicon_max;
  d.rule.size_slack = p->size_slack; d.rule.has_sizes = p->size_lb != nullptr;
  d.rule.k = h->cfg.k; d.rule.slack = h->cfg.indels ? h->cfg.k : 1;
  d.endbits = bits_for((uint64_t)h->n + 512); d.idbits = bits_for(np); d.kbits = 8;
  if (d.endbits + d.idbits + d.kbits > 64) return fail(h, PM_E_UNSUPPORTED, "pm_pcr_setup: stream positions and pattern ids do not fit the 64-bit sort key");
  std::vector<int32_t> patlen(np + 1, 0);
  for (size_t i = 0; i < np; ++i) patlen[i + 1] = (int32_t)h->pats[i].s.size();
  const size_t npairs = np / 4;
  PM_TRY(dev_upload(h, &h->pcr_mem[0], patlen.data(), patlen.size() * 4, 4, "pcr patlen"));
  if (p->size_lb) {
    PM_TRY(dev_upload(h, &h->pcr_mem[1], p->size_lb, npairs * 8, 8, "pcr size_lb"));
    PM_TRY(dev_upload(h, &h->pcr_mem[2], p->size_ub, npairs * 8, 8, "pcr size_ub"));
  }
  PM_TRY(dev_upload(h, &h->pcr_mem[3], p->entry_starts, (size_t)p->n_entries * 8, 8, "pcr entry_starts"));
  d.patlen = (const int32_t *)h->pcr_mem[0]; d.size_lb = (const uint64_t *)h->pcr_mem[1]; d.size_ub = (const uint64_t *)h->pcr_mem[2];
  d.entry_starts = (const int64_t *)h->pcr_mem[3]; d.n_entries = p->n_entries;
  for (uint32_t &w : h->pcr_nmask) w = 0;
  for (int c = 0; c < std::min(h->alpha.size, 256); ++c)
    if (h->alpha.ch[c] == 'N' || h->alpha.ch[c] == 'n') h->pcr_nmask[c >> 5] |= 1u << (c & 31);
  HIP_TRY(h, hipHostMalloc((void **)&h->pcr_h_tot, 4 * sizeof(unsigned long long), hipHostMallocDefault));
  h->pcr_on = true;
  h->scan_mode = cur_mode;
  return PM_OK;
}

// room for `need` held records, the first held_n kept
static int pcr_ensure_held(pm_handle *h, size_t need) {
  if (h->held_cap >= need) return PM_OK;
  const size_t cap = std::max<size_t>(need + need / 2, (size_t)1 << 16);
  pm_hit *nh = nullptr;
  HIP_TRY(h, hipMalloc((void **)&nh, cap * sizeof(pm_hit)));
  if (h->held_n) {
    const hipError_t e = hipMemcpyAsync(nh, h->d_held, h->held_n * sizeof(pm_hit), hipMemcpyDeviceToDevice, h->stream);
    if (e != hipSuccess || stream_wait(h) != hipSuccess) { (void)hipFree(nh); return hipfail(h, e, "pm_pcr: growing the held list"); }
  }
  if (h->d_held) (void)hipFree(h->d_held);
  h->d_held = nh; h->held_cap = cap;
  return PM_OK;
}

extern "C" int pm_pcr_feed(pm_handle *h, const pm_hit *hits, size_t n) {
  if (!h || !h->inited || !h->pcr_on) return fail(h, PM_E_INVALID, "pm_pcr_feed: pm_pcr_setup first");
  if (n == 0) return PM_OK;
  if (!hits) return fail(h, PM_E_INVALID, "pm_pcr_feed: no hits");
  if (h->held_n + n >= ((size_t)1 << 31)) return fail(h, PM_E_UNSUPPORTED, "pm_pcr_feed: 2^31 or more held hits");
  for (size_t i = 0; i < n; ++i)
    if (hits[i].pid < 1 || hits[i].pid > h->pats.size() || hits[i].end < 0 || hits[i].end > h->n + 512)
      return fail(h, PM_E_INVALID, "pm_pcr_feed: a hit with an unknown pattern id or an end outside the stream");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  PM_TRY(pcr_ensure_held(h, h->held_n + n));
  HIP_TRY(h, hipMemcpyAsync(h->d_held + h->held_n, hits, n * sizeof(pm_hit), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, stream_wait(h));
  h->held_n += n;
  return PM_OK;
}

// pm_pcr_scan's landing, first half (on the handle's stream, in front of the next range's scan): the records at d_hits --
// n_upper bounds their number, which the host learns later -- are copied behind the held list
static int pcr_land_device(pm_handle *h, const pm_hit *d_hits, size_t n_upper) {
  h->pcr_fed = 0;
  if (n_upper == 0) return PM_OK;
  if (h->held_n + n_upper >= ((size_t)1 << 31)) return fail(h, PM_E_UNSUPPORTED, "pm_pcr_scan: 2^31 or more held hits");
  PM_TRY(pcr_ensure_held(h, h->held_n + n_upper));
  HIP_TRY(h, hipMemcpyAsync(h->d_held + h->held_n, d_hits, n_upper * sizeof(pm_hit), hipMemcpyDeviceToDevice, h->stream));
  h->pcr_fed = n_upper;
  return PM_OK;
}

// second half: nfin of them are hits; the host-decided `extra` are uploaded behind them
static int pcr_collect(pm_handle *h, size_t nfin, std::vector<pm_hit> &extra, size_t *n_out) {
  if (n_out) *n_out = nfin + extra.size();
  if (h->pcr_fed == 0) nfin = 0;
  h->pcr_fed = 0;
  const size_t m = extra.size();
  if (h->held_n + nfin + m >= ((size_t)1 << 31)) return fail(h, PM_E_UNSUPPORTED, "pm_pcr_scan: 2^31 or more held hits");
  h->held_n += nfin;
  if (m) {
    for (pm_hit &x : extra) x.aux[0] = x.aux[1] = x.aux[2] = 0;
    PM_TRY(pcr_ensure_held(h, h->held_n + m));
    // (the handle's stream may hold the next range's scan: the copy stream; the first half's copy is done, the finalize stage was waited for)
    HIP_TRY(h, hipMemcpyAsync(h->d_held + h->held_n, extra.data(), m * sizeof(pm_hit), hipMemcpyHostToDevice, h->copy_stream));
    HIP_TRY(h, hipStreamSynchronize(h->copy_stream));
    h->held_n += m;
  }
  return PM_OK;
}

extern "C" int pm_pcr_scan(pm_handle *h, int64_t begin, int64_t end, size_t *n_new) {
  if (n_new) *n_new = 0;
  if (!h || !h->inited || !h->pcr_on) return fail(h, PM_E_INVALID, "pm_pcr_scan: pm_pcr_setup first");
  if (h->scan_mode == 1) return fail(h, PM_E_INVALID, "pm_pcr_scan after pm_scan (pm_reset first)");
  if (h->scan_mode == 2) return fail(h, PM_E_INVALID, "pm_pcr_scan after pm_count_scan (pm_reset first)");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  h->scan_mode = 3;
  if (end > h->n) end = h->n;
  if (end <= begin) return PM_OK;
  const size_t before = h->held_n;
  h->pcr_scanning = true;
  const int rc = scan_range(h, begin, end);
  h->pcr_scanning = false;
  if (rc) { h->held_n = std::min(h->held_n, before); return rc; }
  if (n_new) *n_new = h->held_n - before;
  return PM_OK;
}

namespace {
struct Carver {                                                       // hands out 256-byte aligned pieces of one allocation
  char *base; size_t at = 0;
  explicit Carver(void *b) : base((char *)b) {}
  template <class T> T *take(size_t count) { T *p = base ? (T *)(base + at) : nullptr; at += (count * sizeof(T) + 255) & ~(size_t)255; return p; }
};
}  // namespace

static int pcr_grow(pm_handle *h, void **buf, size_t *have, size_t need, const char *what) {
  if (*have >= need) return PM_OK;
  *have = need + need / 4;
  return dev_regrow(h, buf, *have, what);
}

extern "C" int pm_pcr_pair(pm_handle *h, int64_t scanned_to, int more, int with_strings, size_t stride, const pm_pcr_amplicon **out, size_t *n_out,
                           const char **ops, const char **text) {
  if (out) *out = nullptr;
  if (n_out) *n_out = 0;
  if (ops) *ops = nullptr;
  if (text) *text = nullptr;
  if (!h || !h->inited || !h->pcr_on) return fail(h, PM_E_INVALID, "pm_pcr_pair: pm_pcr_setup first");
  if (!out || !n_out || (with_strings && (!ops || !text || stride == 0))) return fail(h, PM_E_INVALID, "pm_pcr_pair: bad arguments");
  HIP_TRY(h, hipSetDevice(h->cfg.device));
  // (pm_pcr_scan may have left the next range's look-ahead scan on the handle's stream.  The round queues behind it and
  // waits for it: at the first of its stream_waits below, or already in ensure_sort_workspace when that has to grow --
  // hipFree synchronises -- so the scan does not overlap the round as it overlaps pm_scan's host work; the round only
  // starts with that range scanned.  Growing is safe for the same reason and because the scan refills the record buffer
  // only: nothing here reads that, and a scan uses the sort workspace only when it is collected)
  const size_t n = h->held_n;
  h->pcr_stat[0] = n; h->pcr_stat[1] = h->pcr_stat[2] = 0;
  if (n == 0) return PM_OK;
  if (n >= ((size_t)1 << 31)) return fail(h, PM_E_UNSUPPORTED, "pm_pcr_pair: 2^31 or more held hits");
  PM_TRY(ensure_sort_workspace(h, n, false));
  // workspaces by held hits
  PcrRound w;
  const size_t temp_a = pcr_temp_bytes(n + 1);
  auto carve_a = [&](void *base) {
    Carver c(base);
    w.sorted = c.take<pm_hit>(n); w.gpos_in = c.take<uint32_t>(n); w.gpos = c.take<uint32_t>(n);
    w.def = c.take<uint32_t>(n + 1); w.flag = c.take<uint32_t>(n + 1); w.slot = c.take<uint32_t>(n + 1);
    w.wlo = c.take<uint32_t>(2 * n); w.whi = c.take<uint32_t>(2 * n);
    w.cnt = c.take<unsigned long long>(n + 1); w.off = c.take<unsigned long long>(n + 1);
    w.temp = c.take<char>(temp_a); w.temp_bytes = temp_a;
    return c.at;
  };
  PM_TRY(pcr_grow(h, &h->d_pcr_a, &h->pcr_a_bytes, carve_a(nullptr), "the pairing round's workspace"));
  carve_a(h->d_pcr_a);
  w.keys = h->d_keys; w.keys_alt = h->d_keys_alt;
  if (temp_a <= h->ctemp_bytes) { w.temp = h->d_ctemp; w.temp_bytes = h->ctemp_bytes; }   // the handle's sort workspace where it is large enough
  void *const temp_n = w.temp; const size_t temp_n_bytes = w.temp_bytes;
  HIP_TRY(h, pcr_join_device(h->pcr, h->d_held, n, scanned_to, more != 0, w, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->pcr_h_tot, w.off + n, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, stream_wait(h));
  const unsigned long long npairs = h->pcr_h_tot[0];
  h->pcr_stat[1] = npairs;
  if (npairs >= (1ull << 31)) return fail(h, PM_E_UNSUPPORTED, "pm_pcr_pair: 2^31 or more candidate pairs in one round (hit-dense text: pair more often, or narrow -M)");
  size_t nsurv = 0;
  if (npairs) {
    // the pair list and what is sized by it; the hits that take part are at most two per pair and at most all
    const size_t st = with_strings ? stride : 0, temp_b = pcr_temp_bytes((size_t)npairs + 1);
    const size_t mmax = (size_t)std::min<unsigned long long>(n, 2 * npairs);
    uint2 *d_pairs; uint32_t *d_keep, *d_kof; pm_hit *d_hv; pm_alignment *d_al; char *d_ops, *d_txt, *d_temp_b;
    auto carve_b = [&](void *base) {
      Carver c(base);
      d_pairs = c.take<uint2>(npairs); d_keep = c.take<uint32_t>(npairs + 1); d_kof = c.take<uint32_t>(npairs + 1);
      d_hv = c.take<pm_hit>(mmax); d_al = c.take<pm_alignment>(mmax); d_ops = c.take<char>(mmax * st); d_txt = c.take<char>(mmax * st);
      d_temp_b = c.take<char>(temp_b);
      return c.at;
    };
    PM_TRY(pcr_grow(h, &h->d_pcr_b, &h->pcr_b_bytes, carve_b(nullptr), "the pairing round's pair list"));
    carve_b(h->d_pcr_b);
    HIP_TRY(h, pcr_write_device(n, w, d_pairs, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->pcr_h_tot + 1, w.slot + n, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, pcr_gather_device(n, w, d_hv, h->stream));
    HIP_TRY(h, stream_wait(h));
    const size_t m = (size_t)*(const uint32_t *)(h->pcr_h_tot + 1);
    const pm_count_info before = h->cinfo;
    // (the strings are copied whole, stride bytes each: nothing stale behind their ends)
    if (with_strings) { HIP_TRY(h, hipMemsetAsync(d_ops, 0, m * st, h->stream)); HIP_TRY(h, hipMemsetAsync(d_txt, 0, m * st, h->stream)); }
    PM_TRY(pm_align_hits_device(h, d_hv, m, d_al, with_strings ? d_ops : nullptr, with_strings ? d_txt : nullptr, st));
    h->pcr_stat[3] += h->cinfo.aligned_device - before.aligned_device;
    h->pcr_stat[4] += h->cinfo.aligned_host - before.aligned_host;
    h->pcr_stat[5] += h->cinfo.record_bytes_to_host - before.record_bytes_to_host;
    h->cinfo = before;                                                // (pm_counts' info is pm_count_scan's)
    w.temp = d_temp_b; w.temp_bytes = temp_b;
    HIP_TRY(h, pcr_filter_device(h->pcr, w, d_pairs, (size_t)npairs, d_al, d_keep, d_kof, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->pcr_h_tot + 2, d_kof + npairs, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, stream_wait(h));
    nsurv = (size_t)*(const uint32_t *)(h->pcr_h_tot + 2);
    if (nsurv) {
      // survivors and their strings: a device buffer of their own, copied into the pinned one in one piece
      const size_t rec_bytes = (nsurv * sizeof(pm_pcr_amplicon) + 255) & ~(size_t)255, str_bytes = 2 * nsurv * st;
      PM_TRY(pcr_grow(h, &h->d_pcr_c, &h->pcr_c_bytes, rec_bytes + 2 * str_bytes + 16, "the pairing round's survivors"));
      void *const d_res = h->d_pcr_c;
      pm_pcr_amplicon *d_rec = (pm_pcr_amplicon *)d_res;
      char *d_sops = (char *)d_res + rec_bytes, *d_stxt = d_sops + str_bytes;
      hipError_t e = hipSuccess;
      if (h->pcr_out_bytes < rec_bytes + 2 * str_bytes) {
        if (h->pcr_out) (void)hipHostFree(h->pcr_out);
        h->pcr_out = nullptr; h->pcr_out_bytes = (rec_bytes + 2 * str_bytes) * 2;
        e = hipHostMalloc(&h->pcr_out, h->pcr_out_bytes, hipHostMallocDefault);
        if (e != hipSuccess) h->pcr_out_bytes = 0;
      }
      if (e == hipSuccess) e = pcr_emit_device(h->pcr, w, d_pairs, (size_t)npairs, d_keep, d_kof, nsurv, d_al, with_strings ? d_ops : nullptr, with_strings ? d_txt : nullptr, st,
                                               h->d_text, h->n, h->pcr_nmask, d_rec, d_sops, d_stxt, h->stream);
      if (e == hipSuccess) e = hipMemcpyAsync(h->pcr_out, d_res, rec_bytes + 2 * str_bytes, hipMemcpyDeviceToHost, h->stream);
      if (e == hipSuccess) e = stream_wait(h);
      if (e != hipSuccess) return hipfail(h, e, "pm_pcr_pair: survivors");
      h->pcr_stat[5] += nsurv * sizeof(pm_pcr_amplicon) + 2 * str_bytes;
      *out = (const pm_pcr_amplicon *)h->pcr_out;
      if (with_strings) { *ops = (const char *)h->pcr_out + rec_bytes; *text = *ops + str_bytes; }
    }
  }
  h->pcr_stat[2] = nsurv;
  *n_out = nsurv;
  // the deferred hits stay, at the front of the list
  w.temp = temp_n; w.temp_bytes = temp_n_bytes;
  HIP_TRY(h, pcr_carry_device(n, w, h->d_held, h->stream));
  HIP_TRY(h, hipMemcpyAsync(h->pcr_h_tot + 3, w.slot + n, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, stream_wait(h));
  h->held_n = (size_t)*(const uint32_t *)(h->pcr_h_tot + 3);
  return PM_OK;
}

extern "C" int pm_pcr_stats(pm_handle *h, uint64_t *out, int n) {
  if (!h || !h->inited || !out || n < 0) return fail(h, PM_E_INVALID, "pm_pcr_stats: bad arguments");
  for (int i = 0; i < n && i < 6; ++i) out[i] = h->pcr_stat[i];
  return PM_OK;
}
