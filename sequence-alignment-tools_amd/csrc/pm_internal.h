// pm_internal.h -- shared declarations of the product path (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pm_gpu.h"
#include "pm_align.h"
#include "pm_pcr.h"

namespace pm {

struct Pattern {
  std::string s;
  uint64_t    id;
  int         esb, eeb;
};

// The CharacterProducer facts an engine needs (reference char_io.h:18-71): ch(), nch(), size().
struct Alphabet {
  int     size = 256;
  uint8_t ch[256];
  int     nch[256];
  bool    present[256];     // false: the code is known not to occur in the stream (only narrowed for raw streams with -w/-W)
  void set_raw();
  void set_table(const uint8_t *table, int len);
};

// Test and measurement knobs (PM_SEED_CHUNK, PM_SEED_GROUP, PM_SEED_DEBUG, PM_SEED_TILE, PM_PAIR, PM_PAIR_ROW, PM_PAIR_MAP, PM_HALF_SCAN,
// PM_EDIT_SCAN, PM_EDIT_PAIR, PM_EDIT_TABLE_LOG, PM_SHORT_SCAN, PM_SHORT_TILE, PM_SHORT_SUB, PM_LONG_SUB, PM_LONG_EXACT, PM_LONG_EDITS, PM_LONG_HALVES, PM_WILD_CLASS, PM_WILD_LONG, PM_BITPAR_TP, PM_BITPAR_SEGLEN, PM_DEBUG).  The environment is read ONCE, by
// pm_create (pm_api.cpp read_knobs), into the handle: nothing on the init or launch path calls getenv, and a
// handle's behaviour does not change when its caller's environment does.  Every field's 0 / -1 / false = unset.
struct Knobs {
  long long seed_chunk = 0;          // positions per workgroup of the seed-family scan kernels
  int seed_group = 0;                // chunks per run of one combo
  int seed_debug = 0;                // stage switches (measurement builds of the scan kernels)
  long seed_tile = 0;                // keys per pattern tile
  int pair = -1;                     // 0: keep -K 1 / -K 2 off the pair plan
  int pair_row = 0;                  // PM_PAIR_ROW: slots per row of the pair plan's slot table (measurement)
  int pair_map = -1;                 // PM_PAIR_MAP: workgroup -> (field pair, chunk) of the pair kernels (pm_workmap.h PAIR_MAP_*; -1: by range size)
  bool half_bloom = false;           // exact_halves -k on the round-1 form (PM_HALF_SCAN=bloom)
  bool edit_bloom = false;           // edits: first stage = the round-1 pm_seed_scan instance (PM_EDIT_SCAN=bloom)
  bool edit_hash = false;            // edits: first stage = round 2's pm_edit_scan (PM_EDIT_SCAN=hash) wherever the pair geometry would run
  bool edit_pair_off = false;        // PM_EDIT_PAIR=off: the pair geometry runs as the edit plan's first stage only where it ran without the PM_EDIT_PAIR bit of pm_config.long_patterns (A/B runs, tests)
  int edit_table_log = 0;            // edits: log2 of the key map's bits
  int bitpar_tp = -1;                // force the text-parallel (1) / tile (0) form of the bit-parallel kernel
  long long bitpar_seglen = 0;
  long long dense_bound = 0;         // PM_DENSE_BOUND: records per list beyond which pm_scan cuts a range in two (0: 2^29)
  bool short_bitpar = false;         // PM_SHORT_SCAN=bitpar: patterns of 16..19 characters go to the bit-parallel residue, not to pm_short_edit_scan
  long short_tile = 0;               // PM_SHORT_TILE: patterns per tile of pm_short_edit_scan / pm_short_sub_scan
  bool short_sub_off = false;        // PM_SHORT_SUB=off: -K lists with patterns of 16..19 characters leave the pair plan as a whole (A/B runs, tests)
  bool long_sub_off = false;         // PM_LONG_SUB=off: -K patterns of 33..64 characters stay off the pair plan whatever pm_config.long_patterns says (A/B runs, tests)
  bool long_exact_off = false;       // PM_LONG_EXACT=off: k = 0 patterns of 33..64 characters stay off the seed plan whatever pm_config.long_patterns says (A/B runs, tests)
  bool long_edits_off = false;       // PM_LONG_EDITS=off: -k patterns of 33..64 characters stay off the edit plan whatever pm_config.long_patterns says (A/B runs, tests)
  bool long_halves_off = false;      // PM_LONG_HALVES=off: exact_halves -k lists with patterns of 33..64 characters stay off the halves plan whatever pm_config.long_patterns says (A/B runs, tests)
  bool wild_long_off = false;        // PM_WILD_LONG=off: -w primers of 33..64 characters with more than 16 concrete variants stay on the bit-parallel residue whatever pm_config.long_patterns says (A/B runs, tests)
  bool wild_off = false;             // PM_WILD_CLASS=off: -w primers with more than 16 concrete variants stay on the bit-parallel residue whatever pm_config.long_patterns says (A/B runs, tests)
  bool debug = false;                // PM_DEBUG: stage timings on stderr
};

// ---- bit-parallel family (pm_bitpar.hip) -----------------------------------------------------
constexpr int BP_WPL = 8;          // 32-bit words per lane: a lane holds a 256-bit pattern string
constexpr int BP_NC = 6;           // distinct stream codes the patterns may accept (A,C,G,T,N + one)
constexpr int BP_BLOCK = 256;      // text bytes per block step (64 lanes x 4 bytes)

struct BitparTables {              // host-built, then uploaded
  int ntiles = 0;                  // 64 lanes per tile
  int nlanes = 0;                  // lanes (256-bit pattern strings) in use, packed from lane 0 of tile 0
  int k = 0;
  int maxlen = 0;
  int nclasses = 0;                // pattern codes in use (<= BP_NC)
  uint8_t cmap[256];               // text code -> class: 0..BP_NC-1, BP_NC = other, BP_NC+1 = EOS
  std::vector<uint32_t> U;         // [tile][cls][w][lane]
  std::vector<uint32_t> S;         // [tile][w][lane]   first-char bits
  std::vector<uint32_t> LAST;      // [tile][w][lane]   last-char bits
  std::vector<uint32_t> INIT;      // [tile][l-1][w][lane]  row l start state (l = 1..k)
  std::vector<uint32_t> lane_first;// [tile*64+lane] -> first index into pid_of for that lane
  std::vector<uint32_t> pid_of;    // pattern id per packed pattern, in (tile,lane,bit) order
};

struct BitparDevice {
  uint32_t *U = nullptr, *S = nullptr, *LAST = nullptr, *INIT = nullptr, *lane_first = nullptr, *pid_of = nullptr;
  uint8_t  *cmap = nullptr;
  int ntiles = 0, nlanes = 0, k = 0, maxlen = 0;
  bool indels = false;
  Knobs knobs;                     // set by the caller after bitpar_upload
};

// Build the packed tables.  Returns "" or an error message (PM_E_UNSUPPORTED).
std::string bitpar_build(const std::vector<Pattern> &pats, const std::vector<uint32_t> &ids,
                         const Alphabet &alpha, int k, int eos_code, BitparTables *out,
                         bool wildcards = false, bool text_n = false);
hipError_t bitpar_upload(const BitparTables &t, bool indels, BitparDevice *d, hipStream_t st);
void bitpar_free(BitparDevice *d);

struct ScanGeometry { int64_t seg_len; int nseg; int blocks; int threads; int work_map = 0; };   // work_map: pair kernels, pm_workmap.h
ScanGeometry bitpar_geometry(const BitparDevice &d, int64_t begin, int64_t end);

// Enqueue the scan of stream range (begin,end] (hit end positions) on `st`.
// out/counter are device pointers; counter must be zeroed by the caller (async memset).
hipError_t bitpar_launch(const BitparDevice &d, const uint8_t *d_text, int64_t n, int64_t begin, int64_t end,
                         pm_hit *d_out, unsigned long long *d_counter, uint64_t cap, hipStream_t st,
                         ScanGeometry *geo_out);
const char *bitpar_kernel_name(int k, bool indels);

// which byte values occur in the stream (pm_util.hip); used to bound the character classes of -w/-W on raw streams
hipError_t stream_presence(const uint8_t *d_text, int64_t n, bool present[256], hipStream_t st);

// ---- bit-packed stream -> bytes + 2-bit words in HBM (pm_unpack.hip) ---------------------------
// n codes of `bits` bits from bit 0 of d_packed (8-byte aligned) -> d_text[0 .. n rounded up to 16) (16-byte aligned, zero
// past n) and, when d_words != nullptr, the words of pack_stream(d_text, n, ascii, ...)
hipError_t unpack_stream(const void *d_packed, int64_t packed_bytes, int bits, int64_t n, bool ascii, void *d_text, uint32_t *d_words, hipStream_t st);

// ---- window gather (verify stage text access when the stream lives only in HBM) -------------
hipError_t gather_windows(const uint8_t *d_text, int64_t n, const int64_t *d_starts, const int32_t *d_lens,
                          const int64_t *d_offsets, int count, uint8_t *d_out, hipStream_t st);


// ---- device clustering for -K filter_bitvec (pm_cluster.hip) ----------------------------------
// Position sharding: the records cover ends in (guard_lo, guard_hi]; this shard
// reports the clusters whose hit ends in (own_lo, own_hi].  guard_lo <= 0 / guard_hi = INT64_MAX
// mean the true start / end of the stream.
struct OwnedRange { int64_t own_lo, own_hi, guard_lo, guard_hi; int on; };

size_t cluster_temp_bytes(size_t n);
// invalid_level: records with this level chain like any other but are never a chain's hit (-1: none)
hipError_t cluster_device(const pm_hit *d_in, size_t n1, const pm_hit *d_in2, size_t n2, int k, int64_t scanned_to, bool last, int invalid_level,
                          const uint8_t *d_pat_len, const uint32_t *d_pat_id, const OwnedRange &own,
                          uint64_t *d_keys, uint64_t *d_keys_alt, void *d_temp, size_t temp_bytes,
                          pm_hit *d_out, pm_hit *d_left, unsigned long long *d_counts, hipStream_t st);


// final hits in (end, pid, k) order on the device (pm_cluster.hip): see sort_final_device
hipError_t sort_final_device(const pm_hit *d_in, const unsigned long long *d_count, size_t n_upper, const uint32_t *d_pat_id, uint32_t npat,
                             int idxbits, int keybits, uint64_t *d_keys, uint64_t *d_keys_alt, pm_hit *d_out, void *d_temp, size_t temp_bytes, hipStream_t st);

// records of d_in that end in the owned range, compacted into d_out (pass-through engines, sharded scans)
hipError_t owned_filter_device(const pm_hit *d_in, size_t n, const OwnedRange &own, pm_hit *d_out, unsigned long long *d_count, hipStream_t st);

constexpr uint32_t PM_SEED_HOLE = 0xffffffffu;   // pid of an unused slot in the half-seed record buffer
constexpr int SEED_OUT_BLOCK = 64;               // slots a wave reserves per atomic (exact_halves -k seeds)

// duplicate and hole removal for the edit-distance seed plan (pm_cluster.hip); d_out may alias d_in
hipError_t dedup_device(const pm_hit *d_in, size_t n, uint64_t *d_keys, uint64_t *d_keys_alt, void *d_temp, size_t temp_bytes,
                        pm_hit *d_out, unsigned long long *d_count, hipStream_t st);

hipError_t cluster_dp_device(const pm_hit *d_in, size_t n1, const pm_hit *d_in2, size_t n2, int k, bool indels, int64_t scanned_to, bool last,
                             const uint8_t *d_text, int64_t ntext, int eos_code,
                             const uint8_t *d_pat_codes, const uint8_t *d_pat_len, const int32_t *d_esb, const int32_t *d_eeb,
                             const uint32_t *d_pat_id, const OwnedRange &own, uint64_t *d_keys, uint64_t *d_keys_alt, void *d_temp, size_t temp_bytes,
                             pm_hit *d_out, pm_hit *d_left, unsigned long long *d_counts, hipStream_t st, bool wide = false);

// exact_halves' sequential per-pattern rule on the device (pm_cluster.hip)
size_t halves_temp_bytes(size_t n);
hipError_t halves_rule_device(const pm_hit *d_in, size_t n, bool flags, int slack, const uint8_t *d_pat_len, const uint32_t *d_pat_id,
                              uint64_t *d_keys, uint64_t *d_keys_alt, uint32_t *d_vals, uint32_t *d_vals_alt, void *d_temp, size_t temp_bytes,
                              pm_hit *d_out, unsigned long long *d_counts, hipStream_t st);

// ---- the caller's re-alignment and tally on the device (pm_align.hip) ----------------------------
constexpr int AL_MAXL = 32, AL_MAXK = 3;         // device limit of the edit-distance DP; longer patterns are aligned by the host
constexpr int AL_MAXL_SUB = 64;                  // ... but for -K (no indels: the DP is one diagonal), which the device walks up to this length
constexpr int AL_MAXL_WIDE = 64;                 // ... and with indels where pm_config.long_patterns has PM_LONG_ALIGN: pm_align_hits_wide_kernel
constexpr int AL_THREADS = 64;                   // one wave per block: every lane owns a column of the block's LDS
constexpr uint64_t TALLY_INVALID = ~0ull;        // tally key of a record the device did not align
constexpr int TALLY_BOGUS = 4;                   // distance code of a hit that re-aligns to more than k (or to a violation)
constexpr uint32_t TALLY_MAXPAT = (1u << 22) - 1;   // pattern indices fit 22 bits below the invalid key's
constexpr int ALIGN_TAB_BYTES = 256 + 128 * 4;

struct AlignDevice {                             // uploaded once per init (pm_api.cpp ensure_align_tables)
  const uint8_t *tab = nullptr;                  // align_tables()
  const uint8_t *pchars = nullptr;               // the patterns as added, one after the other
  const uint32_t *poff = nullptr;                // [npat + 1] offsets into pchars
  const int32_t *esb = nullptr, *eeb = nullptr;
  const uint32_t *ids_sorted = nullptr, *perm = nullptr;   // pattern ids in increasing order and the pattern index of each
  const uint32_t *idrank = nullptr;              // pattern index -> rank of its id
  uint32_t npat = 0;
  int k = 0, indels = 0, eos = 0, wc = 0, tn = 0;
};
void align_tables(const Alphabet &alpha, uint8_t *tab);
// One lane per record of d_hits[0 .. min(*d_count, n_upper)) (d_count may be NULL).  Any of d_out, d_ops + d_txt (strings
// at i * stride), d_keys (tally keys) may be NULL.  Records of patterns beyond the device limit go to d_hostq_hits (the
// records) / d_hostq_idx (their indices), whichever is not NULL, counted in d_ctr[0]; d_ctr[1] counts unknown pattern ids,
// d_ctr[2] strings that did not fit.
hipError_t align_hits_device(const AlignDevice &a, const uint8_t *d_text, int64_t ntext, const pm_hit *d_hits, const unsigned long long *d_count,
                             size_t n_upper, pm_alignment *d_out, char *d_ops, char *d_txt, size_t stride, uint64_t *d_keys,
                             pm_hit *d_hostq_hits, uint64_t *d_hostq_idx, unsigned long long *d_ctr, hipStream_t st);
// Behind align_hits_device on the same stream, no host step in between: one lane per record of the list that call left
// (d_side_hits, d_side_idx -- both required -- and their count d_ctr[0], n_upper as in that call).  Patterns of 33..64
// characters with indels, 1 <= a.k <= AL_MAXK: the record's results go where that call would have put them (d_out[idx],
// the strings at idx * stride, d_keys[idx]; any may be NULL).  Records it cannot take either go to d_rest_hits /
// d_rest_idx, whichever is not NULL, counted in d_ctr[3]; d_ctr[2] goes on counting strings that did not fit.
hipError_t align_hits_wide_device(const AlignDevice &a, const uint8_t *d_text, int64_t ntext, const pm_hit *d_side_hits, const uint64_t *d_side_idx,
                                  size_t n_upper, pm_alignment *d_out, char *d_ops, char *d_txt, size_t stride, uint64_t *d_keys,
                                  pm_hit *d_rest_hits, uint64_t *d_rest_idx, unsigned long long *d_ctr, hipStream_t st);
// d_src[j] (and the two strings at j * stride, when d_ops != NULL) -> place d_idx[j] of d_out / d_ops / d_txt, j < m
hipError_t align_scatter_device(const uint64_t *d_idx, size_t m, const pm_alignment *d_src, const char *d_src_ops, const char *d_src_txt, size_t stride,
                                pm_alignment *d_out, char *d_ops, char *d_txt, hipStream_t st);
size_t tally_temp_bytes(size_t n);
hipError_t tally_device(const AlignDevice &a, uint64_t *d_keys, uint64_t *d_keys_alt, uint64_t *d_scan, size_t n, void *d_temp, size_t temp_bytes,
                        uint64_t max_count, unsigned long long *d_counts, unsigned long long *d_info, hipStream_t st);

// ---- pcr_match's pairing stage on the device (pm_pcr.hip) --------------------------
struct PcrDevice {                               // uploaded by pm_pcr_setup
  pcr::Rule rule{};
  const int32_t *patlen = nullptr;               // [2n + 1] by pattern id
  const uint64_t *size_lb = nullptr, *size_ub = nullptr;   // [n / 2] by primer pair - 1, or NULL
  const int64_t *entry_starts = nullptr;
  int64_t n_entries = 0;
  int endbits = 0, idbits = 0, kbits = 0;        // sort key = end | id | k
};
struct PcrRound {                                // workspaces of one round over n held hits (n + 1 entries where a scan runs)
  uint64_t *keys = nullptr, *keys_alt = nullptr; // [n] (the handle's sort workspace); after the join keys_alt holds the id-grouped keys
  void *temp = nullptr; size_t temp_bytes = 0;   // pcr_temp_bytes(max(n, pairs) + 1)
  pm_hit *sorted = nullptr;                      // [n] the held hits in (key, id, k) order
  uint32_t *gpos_in = nullptr, *gpos = nullptr;  // [n] id-grouped order -> position in `sorted`
  uint32_t *def = nullptr, *flag = nullptr, *slot = nullptr;   // [n + 1] deferred, takes part in a pair, exclusive scan of either
  uint32_t *wlo = nullptr, *whi = nullptr;       // [2n] the alive part of the hit's two windows in the id-grouped order
  unsigned long long *cnt = nullptr, *off = nullptr;   // [n + 1] pairs per hit and their exclusive scan (off[n] = all pairs)
};
size_t pcr_temp_bytes(size_t n);
// sort, group, count pass and scan: afterwards w.off[n] is the number of candidate pairs and w.flag is zero
hipError_t pcr_join_device(const PcrDevice &d, const pm_hit *d_held, size_t n, int64_t scanned_to, int more, const PcrRound &w, hipStream_t st);
// write pass + scan of the flags: d_pairs[off[n]] = (position, partner's position); w.slot[n] = hits that take part
hipError_t pcr_write_device(size_t n, const PcrRound &w, uint2 *d_pairs, hipStream_t st);
hipError_t pcr_gather_device(size_t n, const PcrRound &w, pm_hit *d_out, hipStream_t st);
// filter pass over the pairs and the alignments of the gathered hits: d_keep / d_kof [npairs + 1], d_kof[npairs] = survivors
hipError_t pcr_filter_device(const PcrDevice &d, const PcrRound &w, const uint2 *d_pairs, size_t npairs, const pm_alignment *d_al, uint32_t *d_keep, uint32_t *d_kof, hipStream_t st);
// survivor records (and the strings of both ends at (2q, 2q + 1) * stride when d_ops != NULL) + the N count; nmask: bit c = code c decodes to N or n
hipError_t pcr_emit_device(const PcrDevice &d, const PcrRound &w, const uint2 *d_pairs, size_t npairs, const uint32_t *d_keep, const uint32_t *d_kof, size_t nsurv,
                           const pm_alignment *d_al, const char *d_ops, const char *d_txt, size_t stride, const uint8_t *d_text, int64_t ntext,
                           const uint32_t nmask[8], pm_pcr_amplicon *d_out, char *d_out_ops, char *d_out_txt, hipStream_t st);
// deferred hits -> d_held[0 .. w.slot[n])
hipError_t pcr_carry_device(size_t n, const PcrRound &w, pm_hit *d_held, hipStream_t st);

// ---- edit distance for patterns of 16..19 characters (pm_short.hip) ------------------------------
// First stage pm_short_edit_scan (field pairs of the last 16 bases, 14 tests at k = 2, 2 at k = 1) + the automaton stage of
// pm_seed.hip over its seed records.  A class is cut into tiles of at most `tile` patterns (the 16-bit key space fills up):
// one launch per tile into the same seed list, one automaton launch behind them.
constexpr int SHORT_NTESTS = 14;
constexpr size_t SHORT_TILE_DEFAULT = 32768;

// A tile's key index as both classes of 16..19 characters build it (pm_short_tables.h) and as it lies on the device
struct ShortTileIndex {
  uint32_t base = 0;               // class index of the tile's first pattern
  std::vector<uint32_t> bitmap;    // [field pair][2048]: bit = 16-bit key of some pattern
  std::vector<uint32_t> rows;      // [field pair][65537]: first entry of the key's run in runs
};
struct ShortTileDevice { uint32_t base = 0; uint32_t *bitmap = nullptr, *rows = nullptr; void *runs = nullptr; uint32_t *pat16 = nullptr; };

struct ShortTables {               // host-built, then uploaded
  int k = 0, maxlen = 0, eos_code = -1;
  bool ascii = false;
  std::vector<uint8_t> records;    // 32-byte automaton record per pattern of the class (pm_seed.h edit_record_fill)
  struct Tile : ShortTileIndex {
    std::vector<uint32_t> runs;    // [field pair][patterns of the tile]: pattern indices (inside the tile) by key
    std::vector<uint32_t> pat16;   // last 16 bases of every pattern, 2 bits each
  };
  std::vector<Tile> tiles;
};

struct ShortDevice {
  int k = 0, maxlen = 0, eos_code = -1;
  bool ascii = false;
  size_t npat = 0;
  uint8_t *records = nullptr;
  std::vector<ShortTileDevice> tiles;
};

// Build the tables of the class (`tile` = patterns per tile, 0: SHORT_TILE_DEFAULT).  Returns "" or an error message.
std::string short_build(const std::vector<Pattern> &pats, const std::vector<uint32_t> &ids, const Alphabet &alpha, int k, int eos_code,
                        size_t tile, ShortTables *out);
hipError_t short_upload(const ShortTables &t, ShortDevice *d, hipStream_t st);
void short_free(ShortDevice *d);
// Enqueue the scan of (begin, end] on `st`: candidate records are appended to d_out / d_counter like bitpar_launch's; the seed
// records in between go to d_seeds[0 .. seed_cap), counted in *d_seed_count (zeroed by the caller; it may exceed seed_cap:
// the caller grows the list and scans again).  d_packed: the stream's 2-bit words (pack_stream).
hipError_t short_launch(const ShortDevice &d, const uint8_t *d_text, const uint32_t *d_packed, int64_t n, int64_t begin, int64_t end,
                        pm_hit *d_out, unsigned long long *d_counter, uint64_t cap, uint64_t *d_seeds, unsigned long long *d_seed_count,
                        uint64_t seed_cap, hipStream_t st, ScanGeometry *geo_out);

// ---- substitutions only (-K 1, -K 2) for patterns of 16..19 characters (pm_short.hip) ---------------
// A class beside a main class on the pair plan (pm_pair.hip): pm_short_sub_scan (field pairs of the last 16 bases: six at
// k = 2, two at k = 1; 8-byte run entries {pattern, its last 16 bases}) + pm_short_sub_verify, which runs pm_verify.h's
// pair_verify<4> -- the pair plan's exact stage with fields of four bases -- so both classes write records of one meaning.
constexpr int SUB_MAX_COMBOS = 6;
// Largest class the routing takes (patterns as added, both strands counted): where the pass with the class met the
// Bloom plan's pass for the whole list (3 Gbp, 100k 20-mers x 2 strands, 12,000 18-mers x 2: 75 - 102 ms against 78 - 107 ms;
// 8,000 x 2: 57 against 75 ms; 16,000 x 2: 93 against 81 - 106 ms).  Lists above it keep the Bloom plan.
constexpr size_t SHORT_SUB_MAX_PATTERNS = 24000;

struct ShortSubTables {            // host-built, then uploaded
  int k = 0, maxlen = 0, eos_code = -1, ncombos = 0;
  bool ascii = false;
  int fa[SUB_MAX_COMBOS] = {}, fb[SUB_MAX_COMBOS] = {};   // key fields of every combo (a < b) in the order that decides who reports
  std::vector<uint8_t> pat_len;    // per pattern of the class
  std::vector<uint32_t> pat_id;
  std::vector<uint8_t> pat_codes;  // 32 stream codes per pattern
  std::vector<uint32_t> pat_zone;  // bit i: pattern character i lies in an exact zone
  struct Tile : ShortTileIndex {
    std::vector<uint64_t> runs;    // [combo][patterns of the tile] by key: pattern index inside the tile | last 16 bases << 32
  };
  std::vector<Tile> tiles;
};

struct ShortSubDevice {
  int k = 0, maxlen = 0, eos_code = -1, ncombos = 0;
  bool ascii = false;
  int fa[SUB_MAX_COMBOS] = {}, fb[SUB_MAX_COMBOS] = {};
  size_t npat = 0;
  uint8_t *pat_len = nullptr, *pat_codes = nullptr;
  uint32_t *pat_id = nullptr, *pat_zone = nullptr;
  std::vector<ShortTileDevice> tiles;            // (pat16 unused: the run entries hold the bases)
  int viol_level = 0;              // as PairDevice::viol_level (set by the caller after short_sub_upload)
};

std::string short_sub_build(const std::vector<Pattern> &pats, const std::vector<uint32_t> &ids, const Alphabet &alpha, int k, int eos_code,
                            size_t tile, ShortSubTables *out);
hipError_t short_sub_upload(const ShortSubTables &t, ShortSubDevice *d, hipStream_t st);
void short_sub_free(ShortSubDevice *d);
// Enqueue the scan of (begin, end] on `st`: candidate records are appended to d_out / d_counter like pair_launch's.  The
// 8-byte suspects in between go to d_susp[0 .. susp_cap), counted in *d_susp_count (zeroed by the caller; it may exceed
// susp_cap: the caller grows the list and scans again).
hipError_t short_sub_launch(const ShortSubDevice &d, const uint8_t *d_text, const uint32_t *d_packed, int64_t n, int64_t begin, int64_t end,
                            pm_hit *d_out, unsigned long long *d_counter, uint64_t cap, uint64_t *d_susp, unsigned long long *d_susp_count,
                            uint64_t susp_cap, hipStream_t st);

// ---- the wild class: -w primers of 16..32 (16..64: DESIGN.md 4.14) characters with more than 16 concrete variants (pm_short.hip) ----
// A class beside (or without) the seed family's main class at k = 0 (keyword_tree, shift_and) and -K 1 / -K 2 (filter_bitvec):
// pm_wild_sub_scan -- pm_short_sub_scan's scan with keys expanded per field pair and 8-byte run entries {primer, class word}
// (pm_wild_tables.h) -- + pm_wild_sub_verify, which runs pm_verify.h's wild_verify<4>: records of the main class's meaning.
// A class that holds a primer of 33..64 characters is WIDE as a whole: rows of pat_class are 32 bytes, rows of pat_zone two
// dwords, and pm_wild_sub_verify_wide (wild_verify<4, 64>) reads them; the key index and the scan are the same.
struct WildTables {                // host-built, then uploaded
  int k = 0, maxlen = 0, eos_code = -1, ncombos = 0;
  bool ascii = false, wide = false;
  int fa[SUB_MAX_COMBOS] = {}, fb[SUB_MAX_COMBOS] = {};
  std::vector<uint8_t> pat_len;    // per primer of the class
  std::vector<uint32_t> pat_id;
  std::vector<uint8_t> pat_class;  // 16 bytes per primer (wide: 32): a class nibble per character
  std::vector<uint8_t> pat_reg;    // the field pair the primer is entered under at k = 0
  std::vector<uint32_t> pat_zone;  // bit i: character i lies in an exact zone (wide: two dwords per primer, low dword first)
  size_t nlong = 0;                // primers of 33..64 characters
  std::vector<uint32_t> bitmap, rows;
  std::vector<uint64_t> runs;      // class index of the primer | class word << 32, by field pair and key
  size_t max_entries = 0;          // run entries of the fullest field pair
};

struct WildDevice {
  int k = 0, maxlen = 0, eos_code = -1, ncombos = 0;
  bool ascii = false, wide = false;
  int fa[SUB_MAX_COMBOS] = {}, fb[SUB_MAX_COMBOS] = {};
  size_t npat = 0, max_entries = 0, nlong = 0;
  uint8_t *pat_len = nullptr, *pat_class = nullptr, *pat_reg = nullptr;
  uint32_t *pat_id = nullptr, *pat_zone = nullptr;
  std::vector<ShortTileDevice> tiles;            // one tile (the entry cap keeps the class small)
  int viol_level = 0;              // as PairDevice::viol_level (set by the caller after wild_upload)
};

// The routing's two questions (pm_wild_tables.h wild_primer_fits, wild_entries_fit): a primer the class can hold -- 16..maxL
// characters (maxL: 32 or 64), a base accepted at every character, at most 256 keys in every field pair of the plan -- and a
// class whose run entries stay within SHORT_SUB_MAX_PATTERNS per field pair.
bool wild_takes(const std::string &s, int k, size_t maxL);
bool wild_class_fits(const std::vector<std::string> &pats, int k);
// Primers as added (with their letters); every one must pass wild_primer_fits (pm_wild_tables.h).  Returns "" or why the
// class is refused as a whole.
std::string wild_build(const std::vector<Pattern> &pats, const std::vector<uint32_t> &ids, const Alphabet &alpha, int k, int eos_code, WildTables *out);
hipError_t wild_upload(const WildTables &t, WildDevice *d, hipStream_t st);
void wild_free(WildDevice *d);
// As short_sub_launch: records into d_out / d_counter, the 8-byte suspects in between into d_susp under *d_susp_count.
// geo_out: the scan's geometry (a handle without a main class reports it).
hipError_t wild_launch(const WildDevice &d, const uint8_t *d_text, const uint32_t *d_packed, int64_t n, int64_t begin, int64_t end,
                       pm_hit *d_out, unsigned long long *d_counter, uint64_t cap, uint64_t *d_susp, unsigned long long *d_susp_count,
                       uint64_t susp_cap, hipStream_t st, ScanGeometry *geo_out);

// ---- seed extension DP on the GPU (pm_extend.hip) ---------------------------------------------
hipError_t extend_seeds(const uint8_t *d_text, int64_t n, const pm_hit *d_seeds, size_t nseeds,
                        const uint8_t *d_half_codes, const uint8_t *d_half_len, const int32_t *d_esb, const int32_t *d_eeb,
                        int k, int eos_code, pm_hit *d_out, unsigned long long *d_counter, size_t cap, hipStream_t st,
                        int half_row = 16);   // codes per row of d_half_codes: 16, or 32 (halves of patterns of 33..64 characters)

}  // namespace pm
