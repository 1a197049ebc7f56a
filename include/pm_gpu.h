/* include/pm_gpu.h -- C ABI of the MI355X (gfx950) multi-pattern matcher.
 *
 * This is the drop-in boundary for the reference's PatternMatch plugin surface
 * (reference: pattern_match.h:84-156) on the primer_match / pcr_match scan path.  One handle
 * replaces one PatternMatch engine instance; every entry point names the reference interface it
 * stands in for.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 * All functions return PM_OK (0) or a negative pm_status; pm_last_error() has the text.
 * A handle is owned by one host thread (the reference is single-threaded).
 *
 * Data flow:  pm_create -> pm_add_pattern xN -> pm_init[_device|_windowed|_packed] -> pm_scan ... -> pm_destroy
 * Multi-GPU:  each rank pm_scan_candidates() on its shard of the stream; filter_bitvec option sets
 *             then pm_finalize_device_owned() on the same rank and the final hits are gathered
 *             (RCCL) in rank order; for the others the candidate records are gathered and one
 *             rank pm_finalize()s them in stream order.
 */
#ifndef PM_GPU_H
#define PM_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PM_ABI_VERSION 1

typedef struct pm_handle pm_handle;

/* One hit, as the reference pushes it into pattern_hit_vector (pattern_match.h:82):
 *   end = key  = stream index after the last matched char (cp.pos() at emission),
 *   pid        = pattern_list_element::id() of value.first,
 *   k          = value.second (0 for exact engines, min level for shift_and_inexact, DP value
 *                for the seed+verify wrappers).
 * In *candidate* records (pm_scan_candidates) aux[] carries engine-private data; it is zero in
 * final hits. */
typedef struct {
  int64_t  end;
  uint32_t pid;
  uint8_t  k;
  uint8_t  aux[3];
} pm_hit;

typedef enum {
  PM_OK = 0,
  PM_E_INVALID = -1,       /* bad argument / call order */
  PM_E_UNSUPPORTED = -2,   /* valid in the reference, not implemented by this engine (message says what) */
  PM_E_NOMEM = -3,
  PM_E_HIP = -4,           /* HIP runtime error (no device, launch failure, ...) */
  PM_E_OVERFLOW = -5,      /* candidate buffer too small; *n_out holds the required count (> capacity) */
  PM_E_FATAL = -6          /* the reference would timestamp()+exit(1) here (e.g. select.cc:87-90) */
} pm_status;

/* Which reference engine's hit set to reproduce: the reference's own -N numbers
 * (select.cc:197-265).  PM_SEM_AUTO applies pick_pattern_index's automatic choice
 * (select.cc:101-141, NOPRIMEGEN build) to the patterns added. */
typedef enum {
  PM_SEM_AUTO = 0,
  PM_SEM_KEYWORD_TREE = 2,      /* keyword_tree<...>::find_patterns (keyword_tree.t:427); -N 1,2,3 */
  PM_SEM_SHIFT_AND = 4,         /* shift_and::find_patterns (shift_and.cc:208) */
  PM_SEM_FILTER_BITVEC = 5,     /* filter_bitvec::find_patterns (filter_bitvec.cc:73) */
  PM_SEM_EXACT_BASES = 8,       /* exact_bases::find_patterns (exact_bases.cc:69); -N 7..10 */
  PM_SEM_EXACT_HALVES = 12,     /* exact_halves::find_patterns (exact_halves.cc:120); -N 11..14 */
  PM_SEM_SHIFT_AND_INEXACT = 100 /* bare shift_and_inexact::find_patterns (shift_and_inexact.cc:249) */
} pm_semantics;

/* Which kernel family computes it (the "-N 16 / -N 17" of INTEGRATION.md). */
typedef enum {
  PM_KERNEL_AUTO = 0,
  PM_KERNEL_BITPAR = 16,   /* bit-parallel Shift-And / Wu-Manber rows, any alphabet, <= 6 accepted stream codes */
  PM_KERNEL_SEED = 17      /* 2-bit packed k-mer seeds (LDS filter) + verify; A,C,G,T patterns <= 32 nt (edit distance,
                              -k 1 / -k 2 on filter_bitvec or shift_and_inexact: 16..32 nt -- 20..32 on the pair / piece
                              plans, 16..19 on pm_short_edit_scan).  Under PM_KERNEL_AUTO a -K 1 / -K 2 list of 20..32
                              and 16..19 nt patterns runs on the pair plan and pm_short_sub_scan side by side; asked
                              for by name, this family keeps such a list on one plan, the Bloom plan.  Patterns of
                              33..64 nt join the pair plan (-K 1 / -K 2) or, at k = 0, the Bloom plan under
                              PM_KERNEL_AUTO where pm_config.long_patterns allows it; asked for by name, this family
                              refuses them as before */
} pm_kernel;

/* bits of pm_config.long_patterns */
#define PM_LONG_SUB   1    /* -K 1 / -K 2: patterns of 33..64 characters may run on the pair plan */
#define PM_LONG_EXACT 2    /* k = 0: patterns of 33..64 characters may run on the seed (Bloom) plan */
#define PM_LONG_EDITS 4    /* -k 1 / -k 2: patterns of 33..64 characters may run on the edit plan */
#define PM_LONG_HALVES 8   /* -k 1 / -k 2 under exact_halves: patterns of 33..64 characters may run on the halves plan */
#define PM_LONG_ALIGN 16   /* -k 1 .. -k 3 (edits): hits of patterns of 33..64 characters are re-aligned on the device */
#define PM_WILD_CLASS 32   /* -w, k = 0 / -K 1 / -K 2: patterns of 16..32 characters with more than 16 concrete variants may run on pm_wild_sub_scan */
#define PM_EDIT_PAIR  64   /* -k 1 / -k 2: the edit plan's first stage may run on the pair geometry beyond -k 2 on one tile (every tile, -k 1, exact_bases) */
#define PM_WILD_LONG  128  /* with PM_WILD_CLASS: patterns of 33..64 characters with more than 16 concrete variants may join that class (a wide class verify) */

/* Replaces the constructor arguments of the reference engines as pick_pattern_index passes them
 * (select.cc:19-30): nmismatch, indels, wildcard, textn, eos.  dna_mut is not supported. */
typedef struct {
  int32_t abi_version;     /* PM_ABI_VERSION */
  int32_t semantics;       /* pm_semantics */
  int32_t kernel;          /* pm_kernel */
  int32_t k;               /* -k / -K value */
  int32_t indels;          /* 1 = -k (edits), 0 = -K (substitutions only) */
  int32_t wildcards;       /* -w/-W: IUPAC pattern classes (bit-parallel kernel family) */
  int32_t text_n;          /* -W: a text N also matches (shift_and.cc:112) */
  int32_t eos;             /* raw end-of-sequence char, '\n' in the CLIs */
  int32_t device;          /* HIP device ordinal */
  int32_t long_patterns;   /* a bit set (PM_LONG_SUB | PM_LONG_EXACT | PM_LONG_EDITS | PM_LONG_HALVES | PM_LONG_ALIGN | PM_WILD_CLASS | PM_EDIT_PAIR | PM_WILD_LONG; 0 = the routing of
                              earlier versions).
                              PM_LONG_SUB (1) = with PM_KERNEL_AUTO, -K 1 / -K 2 (substitutions only) and filter_bitvec, bare
                              shift_and_inexact or exact_halves on an A,C,G,T-normalized or raw ASCII stream, patterns
                              of 33..64 characters (A,C,G,T; or <= 16 concrete variants under -w on a plain stream)
                              run on the pair plan beside those of 20..32: the scan reads their last 20 bases, the
                              exact stage rows of 64 characters (pm_pair_verify_wide).
                              PM_LONG_EXACT (2) = with PM_KERNEL_AUTO, k = 0 and keyword_tree or shift_and on such a
                              stream, patterns of 33..64 characters (same conditions) run on the Bloom plan beside
                              those of 10..32: pm_seed_scan reads their last 20 bases (or as many as the list's
                              shortest pattern has), the exact stage rows of 64 characters (wide tiles).
                              PM_LONG_EDITS (4) = with PM_KERNEL_AUTO, -k 1 / -k 2 (edits) and filter_bitvec or bare
                              shift_and_inexact on such a stream, patterns of 33..64 characters (same conditions) run
                              on the edit plan beside those of 20..32: its first stages read their last 20 bases, the
                              automaton runs on 64-bit rows (pm_edits_verify_wide), the cluster DP on 64 rows.
                              PM_LONG_HALVES (8) = with PM_KERNEL_AUTO, -k 1 / -k 2 (edits) and exact_halves (selected
                              or asked for) on such a stream, no wildcards, a list whose patterns are all A,C,G,T and
                              have 16..64 characters (exact_halves keeps no residue) stays on the halves plan when
                              one of them has 33..64: a half of 16..32 characters is tested by pm_half_scan on the
                              bases the lane carries, by pm_half_verify_wide on 64-byte records, and extended by
                              pm_seed_extend on rows of 32 codes.
                              A bit not set = they go to the bit-parallel kernels, as does every pattern of 65
                              characters or more either way.  Each bit acts on its own option sets only.
                              PM_LONG_ALIGN (16) is no routing bit: it changes no scan kernel and not pm_describe.  With
                              indels and 1 <= k <= 3, pm_align_hits_device, pm_count_scan and pm_pcr_pair re-align the
                              records of patterns of 33..64 characters on the device (pm_align_hits_wide_kernel), whichever
                              kernels found them; not set, the host aligns them as before.
                              PM_WILD_CLASS (32) = with PM_KERNEL_AUTO and -w on a plain stream (A,C,G,T, and N only
                              without -W; A,C,G,T-normalized or raw ASCII), substitutions only: keyword_tree or
                              shift_and at k = 0, filter_bitvec at -K 1 / -K 2.  A pattern of 16..32 characters that
                              has more than 16 concrete variants (three or more ambiguity letters), accepts a base at
                              every character, is no N pattern on an N stream under filter_bitvec and expands to at
                              most 256 keys in every field pair of its last 16 bases runs on pm_wild_sub_scan +
                              pm_wild_sub_verify, beside the main class or alone, and not on the
                              bit-parallel residue; a list whose expanded keys exceed 24,000 in some field pair keeps
                              the routing without the bit.  It has nothing to do with the pattern's length: the bit
                              lives here because this field is the one set of routing permissions.
                              PM_EDIT_PAIR (64) = -k 1 / -k 2 (edits) on the seed family's edit plan, patterns of 20..32
                              characters (20..64 with PM_LONG_EDITS): the first stage runs on the pair geometry
                              (pm_pair_edit_scan + pm_pair_edit_resolve) where it ran on the hashed-piece
                              kernel pm_edit_scan -- lists of more than one pattern tile at -k 2 (a table set per tile),
                              -k 1 under filter_bitvec or bare shift_and_inexact (pm_pair_edit_scan_k1: two tests per
                              window), and exact_bases -k 1 / -k 2 (pm_bases_verify behind it; patterns of up to 32
                              characters).  The hits are the same either way.  -k 2 on one tile without exact_bases runs
                              there with or without the bit; PM_EDIT_SCAN=hash / bloom and PM_EDIT_PAIR=off in the
                              environment pm_create reads keep the routing without the bit.  Not set = the routing of
                              earlier versions.
                              PM_WILD_LONG (128) acts only together with PM_WILD_CLASS: under that bit's conditions a
                              pattern of 33..64 characters with more than 16 concrete variants joins the class under the
                              same per-pattern rules (its keys are its last 16 characters').  A class that holds such a
                              pattern is verified by pm_wild_sub_verify_wide on rows of 64 characters;
                              the scan is the same.  It needs none of PM_LONG_SUB .. PM_LONG_ALIGN.  Alone, or with
                              PM_WILD_LONG=off in the environment pm_create reads, it changes nothing.  (The field took
                              the place of reserved[0]: same layout, same PM_ABI_VERSION.) */
  int32_t reserved[6];
} pm_config;

/* new engine (reference: `new shift_and(...)` etc. in select.cc:197-265). */
int pm_create(const pm_config *cfg, pm_handle **out);

/* PatternMatch::add_pattern (pattern_match.h:116): pattern text, caller's id (CLIs use 1..N1,
 * primer_match.cc:1105-1107), exact_start_bases / exact_end_bases. */
int pm_add_pattern(pm_handle *h, const char *pat, size_t len, uint64_t id, int32_t esb, int32_t eeb);

/* PatternMatch::init(CharacterProducer&) (pattern_match.h:130) for a host-resident stream:
 * `text` = the bytes getnch() would return (c_str() of the mmap, char_io.h:167-169), n bytes;
 * `table` = cp.ch(0..size-1) (the .tbl of a Normalized<> stream, char_io.t:216-246) or NULL for
 * a raw stream (size 256, identity).  The bytes are copied to HBM; `text` must stay valid until
 * pm_destroy (the verify stage reads windows from it). */
int pm_init(pm_handle *h, const uint8_t *text, int64_t n, const uint8_t *table, int32_t table_len);

/* Same, for a stream that is already resident in HBM (borrowed; 4-byte aligned).  `hip_stream`
 * is a hipStream_t (NULL = default stream) on which all work of this handle is enqueued.  pm_scan / pm_scan_view may
 * return with a scan of the next range in flight on it (see pm_scan_view), so d_text must stay valid and unchanged
 * until pm_reset or pm_destroy has returned, or the next scan, finalize or pm_candidates_device call on the handle has:
 * each of them waits for that scan first.  Do not free or rewrite the text straight after the last pm_scan. */
int pm_init_device(pm_handle *h, const void *d_text, int64_t n, const uint8_t *table, int32_t table_len,
                   void *hip_stream);

/* pm_init for a stream larger than HBM: `text` (borrowed, as for pm_init) stays in host memory
 * and the GPU holds only a ring of two windows of it, each window_bytes (rounded up to a multiple of 64 and to the
 * option set's minimum, four times the halo of its device stages) plus guard margins.  pm_scan / pm_scan_view give
 * exactly the hits of pm_init for any sequence of ranges: a range longer than a window is scanned in pieces, the next
 * window is uploaded while the current one is scanned, and a piece whose carried clusters reach further back than a
 * window (a long tandem-repeat chain) gets a larger window of its own.  exact_halves' one-call device rule needs the
 * whole stream in one piece, so on a stream longer than a window its hits take the host route pieces already use.
 * The lower-level calls -- pm_scan_candidates[_async], pm_finalize_device[_owned], pm_final_hits_device -- work on a
 * range whose text, with the halo and what carried clusters need, fits one window (it is uploaded first; the records
 * given to pm_finalize_device must be those of the last scan); a larger range is PM_E_INVALID, and so is
 * pm_measure_pair_edit_floor.  pm_align_hits[_text] read `text`. */
int pm_init_windowed(pm_handle *h, const uint8_t *text, int64_t n, const uint8_t *table, int32_t table_len,
                     int64_t window_bytes);

/* PatternMatch::init for a stream held bit-packed in host memory (<db>.sqz, char_io.t:18-214): n codes of `bits` bits,
 * MSB first (code c in bits [c*bits, (c+1)*bits) of the packed bytes, bit 0 being the MSB of byte 0); `table` as for
 * pm_init and mandatory (a packed stream is always a normalized one), table_len <= 2^bits.  window_bytes == 0: the
 * packed bytes are uploaded as they are and unpacked in HBM (then exactly a pm_init handle, except that it keeps no host
 * text: the host stage decodes the windows it verifies from the packed bytes).  window_bytes > 0: as pm_init_windowed
 * (window_bytes counts stream positions, as there), but every window crosses PCIe packed and is unpacked into its slot;
 * the HBM held for the stream is at most 2*(1.25 + bits/8)*(W + 2G) + 2 KiB for a window of W bytes with guard margins
 * of G (three buffers per slot: text, 2-bit words, packed bytes).  `packed` is borrowed until pm_destroy in both forms. */
int pm_init_packed(pm_handle *h, const uint8_t *packed, int64_t packed_bytes, int32_t bits, int64_t n,
                   const uint8_t *table, int32_t table_len, int64_t window_bytes);

/* Unpack the n codes that start at bit 0 of d_packed (8-byte aligned; a window that starts at code `first`, a multiple
 * of 64, passes base + first*bits/8) into d_text and, when d_words != NULL, the 2-bit words d_words[0..ceil(n/16))
 * that the seed family reads (dword i = bases 16i..16i+15, base j in bits 2j, value code & 3, zero past n).  d_text is
 * 16-byte aligned and holds n rounded up to a multiple of 16 bytes: the bytes from n up to there are written zero,
 * nothing beyond.  Loads stay inside packed_bytes.  Enqueued on hip_stream (a hipStream_t, NULL = default stream).
 * The reference's reader is Compressed<>::getnch (char_io.t:104-160). */
int pm_unpack_device(const void *d_packed, int64_t packed_bytes, int32_t bits, int64_t n,
                     void *d_text, void *d_words, void *hip_stream);

/* GPU-free helpers (the host stage's own reader, and its inverse for callers and tests), eight codes at a time:
 * pm_unpack_codes writes codes first .. first+n-1 of the packed bytes to out[0..n); pm_pack_codes writes n codes to
 * out[0..ceil(n*bits/8)), zero fill bits in the last byte and zero bytes up to out_bytes (PM_E_INVALID when a code does
 * not fit `bits` bits or out_bytes is too small). */
int pm_unpack_codes(const uint8_t *packed, int64_t packed_bytes, int32_t bits, int64_t first, int64_t n, uint8_t *out);
int pm_pack_codes(const uint8_t *codes, int64_t n, int32_t bits, uint8_t *out, int64_t out_bytes);

/* Introspection for tests and measurement: out[0] the window size in use (0: the whole stream is resident), out[1] the
 * HBM bytes held now for stream text plus its 2-bit words (and, on a pm_init_packed handle, the packed bytes in HBM while
 * they exist), out[2] the peak of out[1] since init, out[3] stream bytes that crossed PCIe since init (packed bytes for
 * a packed handle), out[4] window loads since init (pm_init: 1, pm_init_device: 0), out[5] bits per code of the host form
 * (0: one byte per code).  n <= 6 values are written. */
int pm_stream_residency(const pm_handle *h, int64_t *out, int n);

/* Free and total HBM of `device` (hipMemGetInfo), for a caller that picks between pm_init and pm_init_windowed: the
 * resident form holds 1.25 bytes per stream base (text + 2-bit words) before any record list exists. */
int pm_device_memory(int device, int64_t *free_bytes, int64_t *total_bytes);

/* PatternMatch::find_patterns (pattern_match.h:131) over the stream range [begin,end):
 * appends to out[0..cap) every final hit with begin < hit.end <= end whose cluster/dedup fate is
 * decided (filter_bitvec.cc:118-121 defers the rest to the next call), sorted by (end,pid).
 * Ranges must be consecutive and increasing between pm_reset()s; end == n flushes everything.
 * *more = 1 when out was too small: call again with begin == end to drain.
 * On hit-dense text a range whose internal record lists would outgrow 2^30 records is scanned in
 * pieces by the library (pm_scan_stats out[6] counts the halvings of the piece length); the hits are those of the
 * whole range, in the same order. */
int pm_scan(pm_handle *h, int64_t begin, int64_t end, pm_hit *out, size_t cap, size_t *n_out, int *more);

/* pm_scan without the copy: *hits points at the final hits of the range -- plus any an earlier pm_scan call left
 * undrained -- in the handle's own (pinned) buffer, *n says how many; the span stays valid until the next call on the
 * handle.  This is the form the PatternMatch plugin uses (host/plugin/gpu_pattern_match.cc): the reference's
 * find_patterns appends to the caller's pattern_hit_vector (pattern_match.h:131), so the plugin pushes the records
 * straight from this span.  Both forms share one pipeline: when the finalize stage of the option set runs on the GPU, the
 * scan of the range expected next (the same number of stream bytes, as primer_match.cc:1118's loop walks the stream) is
 * enqueued before the call returns, and the copy out of HBM, the caller's work on the hits and its next call overlap it.
 * A different next range, pm_reset or pm_destroy simply let that scan finish unused.  So both forms may return with a
 * scan in flight on the handle's stream: it reads the stream text and refills the handle's record buffer, never the
 * memory the hits were handed out in (pm_scan_stats out[7] counts these scans). */
int pm_scan_view(pm_handle *h, int64_t begin, int64_t end, const pm_hit **hits, size_t *n);

/* Device stage only, position-independent (what shards across GPUs): candidate records for
 * begin < end_pos <= end.  Records stay in HBM (pm_candidates_device) and are copied to `out`
 * when it is not NULL.  PM_E_OVERFLOW if more than the internal capacity (pm_set_capacity). */
int pm_scan_candidates(pm_handle *h, int64_t begin, int64_t end, pm_hit *out, size_t cap, size_t *n_out);

/* Asynchronous form for benchmarking and overlap: enqueue the scan on the handle's stream and
 * return; pm_scan_wait() synchronises and reports the count. */
int pm_scan_candidates_async(pm_handle *h, int64_t begin, int64_t end);
int pm_scan_wait(pm_handle *h, size_t *n_out);

/* HBM address of the records of the last pm_scan_candidates (for an RCCL gather).  After pm_scan / pm_scan_view the
 * buffer is not the caller's: the call waits for a look-ahead scan they left in flight, drops it and reports *n = 0. */
int pm_candidates_device(pm_handle *h, void **d_records, size_t *n);
int pm_set_capacity(pm_handle *h, size_t max_candidates);

/* Host stage: cluster / dedup / verify candidate records that arrive in any order within a
 * batch but batch-wise in increasing stream order (filter_bitvec.cc:88-177,
 * exact_halves.cc:140-190).  flags: PM_FINALIZE_LAST flushes deferred clusters (no more input),
 * PM_FINALIZE_SORTED orders the output by (end,pid) (otherwise unspecified, like the emission
 * order of the reference engines).  Text, where the verify needs it, comes from the host pointer
 * given to pm_init, decoded from the packed bytes given to pm_init_packed or, for pm_init_device, from
 * windows fetched out of HBM. */
#define PM_FINALIZE_LAST 1
#define PM_FINALIZE_SORTED 2
int pm_finalize(pm_handle *h, const pm_hit *cands, size_t n, int64_t scanned_to, int flags,
                pm_hit *out, size_t cap, size_t *n_out);

/* Device form of pm_finalize: the records are in HBM (d_cands, or NULL = those of the last
 * pm_scan_candidates), the sort + clustering runs on the GPU and only final hits cross PCIe into
 * `out`.  Available for: exact engines and bare shift_and_inexact (pass-through); filter_bitvec
 * with -K and no exact-base constraints (sort + segmented pass), and with -k on the seed family
 * (A,C,G,T patterns of 16..32 characters, k <= 2: clusters and their DPs on the GPU against the
 * text in HBM); exact_halves on the seed family (exact_halves.cc:142,163,178: its per-pattern
 * "end beyond the last kept end" rule as a sort + one walk per pattern -- stateless, so only with
 * PM_FINALIZE_LAST on an engine state that is fresh since pm_init / pm_reset).
 * PM_E_UNSUPPORTED otherwise: use pm_finalize. */
int pm_finalize_device(pm_handle *h, const void *d_cands, size_t n, int64_t scanned_to, int flags,
                       pm_hit *out, size_t cap, size_t *n_out);

/* One shard of a position-sharded scan (the reference has no such call, its scan is
 * one serial pass -- filter_bitvec.cc:88-177 over the whole stream).  The records (d_cands, or
 * NULL = the last pm_scan_candidates) must hold every candidate with guard_lo < end <= guard_hi;
 * the call reports the final hits with own_lo < end <= own_hi.  Because a cluster's hit ends between
 * its first and last candidate, the shards' outputs concatenate to exactly the single-scan result
 * as long as no same-pattern chain reaches from a guard edge into the owned range (a tandem repeat
 * longer than the guard band): that case returns PM_E_UNSUPPORTED.  guard_lo <= 0 and guard_hi ==
 * INT64_MAX declare the true start / end of the stream (nothing can be hidden beyond them).  Only
 * for the option sets pm_finalize_device supports; implies PM_FINALIZE_LAST. */
int pm_finalize_device_owned(pm_handle *h, const void *d_cands, size_t n, int64_t own_lo, int64_t own_hi,
                             int64_t guard_lo, int64_t guard_hi, int flags, pm_hit *out, size_t cap, size_t *n_out);

/* pm_finalize_device / pm_finalize_device_owned with out == NULL leave the final hits in HBM (the
 * exchange step of a position-sharded scan gathers them from there: no trip through host memory);
 * this returns their address and count.  Valid until the next scan or finalize call of the handle.
 * PM_FINALIZE_SORTED is not available in this form (PM_E_INVALID). */
int pm_final_hits_device(pm_handle *h, void **d_hits, size_t *n);

/* Copy n 16-byte records from HBM (a pointer obtained from pm_candidates_device /
 * pm_final_hits_device, or a gather buffer) to host memory on the handle's stream, synchronously. */
int pm_copy_records(pm_handle *h, const void *d_src, size_t n, pm_hit *out);

/* The caller's per-hit re-alignment (primer_match.cc:1135-1151, pcr_match.cc:1108-1127):
 * exact_alignment::align (pattern_alignment.cc:29-43) for k == 0, otherwise
 * editdist_alignment(key,key,k,eos,wc,tn,indels,dm,esb,eeb,false)::align with traceback
 * (pattern_alignment.cc:117-705).  start/end are stream indices (pa->start(), pa->end());
 * editdist is pa->editdist(), INT32_MAX for a constraint violation ("Bogus hit"). */
typedef struct { int64_t start, end; int32_t editdist, value; } pm_alignment;
int pm_align_hits(pm_handle *h, const pm_hit *hits, size_t n, pm_alignment *out);

/* Same, plus what the caller's formatter prints per hit (primer_match.cc:1196-1202): the alignment
 * string pa->alignment_string() ('|' equal, '*' substitution, '^' insertion, 'v' deletion, '!'
 * constraint violation; pattern_alignment.h:122-165) and the matching text pa->matching_text(),
 * both NUL-terminated at ops + i*stride and text + i*stride.  stride > longest pattern + k. */
int pm_align_hits_text(pm_handle *h, const pm_hit *hits, size_t n, pm_alignment *out, char *ops, char *text, size_t stride);

/* pm_align_hits / pm_align_hits_text for n 16-byte records that lie in HBM (pm_final_hits_device, a gather buffer, the
 * caller's own) -- the results stay in HBM too: d_out[n] pm_alignment and, when d_ops / d_text are given (both or
 * neither; NULL: stride is ignored), the two strings of record i at i * stride.  On a handle whose whole stream is in HBM
 * (pm_init, pm_init_device, pm_init_packed without windows) one GPU lane re-aligns one record; patterns
 * longer than 32 characters with k >= 1, and k > 3, are beyond that kernel: those records are aligned by the code behind
 * pm_align_hits inside the same call, and so is every record of a pm_init_windowed / pm_init_host handle (their text is
 * not in HBM as a whole) -- the answers are the same, pm_counts' info says how many went which way.  A record that has no
 * alignment at all (editdist INT32_MAX with start 0: the DP gave up at a row, pattern_alignment.cc:425-436) gets two
 * empty strings.  Runs on the handle's stream and returns when the results are complete. */
int pm_align_hits_device(pm_handle *h, const void *d_hits, size_t n, void *d_out, void *d_ops, void *d_text, size_t stride);

/* PatternMatch::find_patterns over (begin, end] plus the caller's tally loop (primer_match.cc:1118-1268, `-c`) with
 * nothing handed out: the range's final hits are re-aligned and tallied where they are, in HBM.  Ranges as for pm_scan
 * (consecutive, increasing; end == n flushes; dense ranges are cut into pieces by the library).  The tally, per pattern
 * (each added pattern is one of its own), over its hits in order of stream end: a hit that comes after the pattern's
 * total has reached max_count is skipped; the others are re-aligned; one that re-aligns to more than k (the caller's
 * "Bogus hit", primer_match.cc:1248-1261) is counted in info.bogus and neither tallied nor counted towards max_count;
 * the rest add one to counts[pattern][editdist].  max_count is primer_match's -M (0: none) and must not change between
 * two pm_reset()s; pm_scan / pm_scan_view and pm_count_scan cannot be mixed between two pm_reset()s (PM_E_INVALID).
 * pm_init_windowed handles give the same tallies with the re-alignment on the host; pm_init_host handles cannot scan. */
int pm_count_scan(pm_handle *h, int64_t begin, int64_t end, uint64_t max_count);

/* The tallies since the last pm_reset: counts[i * (k + 1) + d] for the i-th added pattern (npat = patterns added),
 * capped[i] = 1 when its total reached max_count (capped and info may be NULL).  info: hits tallied, hits skipped behind
 * a cap, records re-aligned on the device / on the host (pm_align_hits_device included), bogus hits and the one with the
 * smallest (end, id) (its k is not recorded: 0), bytes of hit records copied device -> host by these calls. */
typedef struct { uint64_t tallied, skipped, aligned_device, aligned_host, bogus, record_bytes_to_host; pm_hit first_bogus; } pm_count_info;
int pm_counts(pm_handle *h, uint64_t *counts, uint8_t *capped, size_t npat, pm_count_info *info);

/* ---- pcr_match's pairing stage on the device (pcr_match.cc:948-1259).  The final hits of the primers stay in
 * HBM in a list the handle holds; one round joins every held hit with its partner primer's hits inside the amplicon window,
 * re-aligns the hits that take part, filters the pairs and counts the N's of the surviving amplicons.  Only survivors cross
 * PCIe.  Opt-in: nothing else of the library changes.
 *
 * pm_pcr_setup: after pm_init / pm_init_device / pm_init_packed without windows (PM_E_UNSUPPORTED for windowed and
 * host-only handles).  The handle must hold an even number 2n of patterns, n even, added with ids 1..2n in order -- the
 * numbering of pcr_match.cc:806-906: 2j-1 forward, 2j reverse, n+1..2n their reverse complements.  size_lb / size_ub: n/2
 * UniSTS size bounds, one per primer pair, or both NULL; size_slack is -d (-1: none).  entry_starts: the stream position
 * where every FASTA entry starts, increasing (the keys of IndexedFastaFile, fasta_io.t:155-214).  The arrays are copied. */
typedef struct {
  int32_t any_orientation;  /* -a */
  int32_t length_between;   /* -b */
  int64_t amplicon_min;     /* -m, >= 0 */
  int64_t amplicon_max;     /* -M */
  int32_t size_slack;       /* -d, -1: none */
  int32_t reserved;
  const uint64_t *size_lb, *size_ub;
  const int64_t *entry_starts;
  int64_t n_entries;
} pm_pcr_params;
/* One surviving pair: the hit that was processed and its partner, their re-alignments, pe1 - ps (with -b: ps1 - pe), the
 * primer pair (pind, 1-based) and the N / n characters at stream positions al[0].start .. al[0].start + amplicon_len - 1. */
typedef struct {
  pm_hit hit[2];
  pm_alignment al[2];
  int64_t amplicon_len;
  uint32_t pair;
  uint32_t ncount;
} pm_pcr_amplicon;
int pm_pcr_setup(pm_handle *h, const pm_pcr_params *p);
/* Append n final hits from host memory to the held list (tests; callers that already have hits). */
int pm_pcr_feed(pm_handle *h, const pm_hit *hits, size_t n);
/* pm_scan's ranges (consecutive, increasing; end == n flushes; dense ranges are cut by the library) with the final hits
 * appended to the held list instead of handed out; *n_new (may be NULL) = how many.  pm_scan / pm_scan_view, pm_count_scan
 * and pm_pcr_scan cannot be mixed between two pm_reset()s (PM_E_INVALID); pm_reset empties the held list. */
int pm_pcr_scan(pm_handle *h, int64_t begin, int64_t end, size_t *n_new);
/* One round over the held hits (pcr_match.cc:987-1259) with scanned_to = the stream position scanned so far and more = the
 * last find_patterns' result: a hit whose window reaches beyond scanned_to while more != 0 is deferred -- it takes part as
 * a partner and stays held; every other hit is dropped after the round.  *out: *n survivors in a pinned buffer of the
 * handle, valid until the next call, ordered by the processed hit in (end, id) order, its first partner id before its
 * second, partners by end.  with_strings: alignment string and matching text (pm_align_hits_text) of hit[0] / hit[1] of
 * survivor i at *ops / *text + (2i, 2i + 1) * stride.  2^31 candidate pairs or more in one round: PM_E_UNSUPPORTED. */
int pm_pcr_pair(pm_handle *h, int64_t scanned_to, int more, int with_strings, size_t stride, const pm_pcr_amplicon **out, size_t *n,
                const char **ops, const char **text);
/* out[0] hits held before the last round, out[1] its candidate pairs, out[2] its survivors, out[3] / out[4] hits re-aligned
 * on the device / on the host since pm_reset, out[5] bytes copied device -> host by these calls since pm_reset (survivor
 * records and strings, records the host re-aligns).  n <= 6 values are written. */
int pm_pcr_stats(pm_handle *h, uint64_t *out, int n);

/* ---- Multi-GPU exchange (the reference has no counterpart: its scan is one serial
 * pass, primer_match.cc:1118).  One rank = one process = one GPU.  The ranks scan position shards
 * (pm_scan_candidates on local stream indices), exchange their record counts by whatever means the
 * launcher has, then gather the 16-byte records out of HBM into rank 0 over xGMI (RCCL send/recv;
 * librccl.so is loaded on first use).  The unique id (PM_COMM_ID_BYTES) is made on rank 0 and handed
 * to the other ranks by the launcher.  Errors: pm_comm_last_error (NULL = the last failed create). */
#define PM_COMM_ID_BYTES 128
typedef struct pm_comm pm_comm;
int pm_comm_unique_id(void *id_out);
int pm_comm_create(int device, int rank, int world, const void *id, pm_comm **out);
/* counts[0..world): records every rank contributes (the same array on every rank).  Rank r sends
 * d_send[0..n_send) (n_send == counts[r]); rank 0 receives all of them in rank order and copies the
 * list to host_out (sum of counts records).  Collective: every rank of the communicator calls it. */
int pm_comm_gather(pm_comm *c, const void *d_send, size_t n_send, const uint64_t *counts, pm_hit *host_out);
void pm_comm_destroy(pm_comm *c);
const char *pm_comm_last_error(const pm_comm *c);

/* PatternMatch::init for a handle that only runs the HOST stage -- pm_finalize, pm_align_hits[_text]
 * -- over the whole stream: the merge rank of a position-sharded scan, whose own GPU holds one shard
 * only.  `text` (borrowed, n bytes, stays on the host) and `table` as for pm_init; the pattern tables
 * are built as for pm_init (they decide what the shards' records mean), nothing of the stream is
 * uploaded, and every scan entry point returns PM_E_INVALID. */
int pm_init_host(pm_handle *h, const uint8_t *text, int64_t n, const uint8_t *table, int32_t table_len);

/* Bring the HIP runtime up on `device` (no reference counterpart).  A command line calls this on a thread of its own at
 * process start, so that the runtime's start-up (0.06 - 0.15 s) runs beside reading the primers and mapping the database;
 * pm_create / pm_init work without it. */
int pm_prepare_device(int device);

/* PatternMatch::reset (pattern_match.h:134): forget scan state, keep patterns and text. */
int pm_reset(pm_handle *h);
void pm_destroy(pm_handle *h);

/* Introspection */
const char *pm_last_error(const pm_handle *h);        /* NULL handle: error of the last pm_create */
int pm_selected_semantics(const pm_handle *h);        /* resolved pm_semantics after pm_init */
int pm_selected_kernel(const pm_handle *h);
/* name of the dominant scan kernel and its launch geometry, for profiles */
int pm_describe(const pm_handle *h, char *buf, size_t buflen);

/* Timing of the scan kernels of the last pm_scan_candidates[_async], measured with HIP events on
 * the handle's stream: milliseconds and number of launches. */
int pm_last_kernel_time(pm_handle *h, float *ms, int *launches);

/* Counters of the last scan, for measurement (bench.py --stream-style; no reference counterpart): out[0] candidate
 * records; out[1] records handed from the first-stage kernel to the verify kernel (suspects of the pair plan, seed records
 * of the edit / halves plans; the pattern tile with most); out[2] scans the library repeated on its own since pm_init
 * because an internal buffer was too small (pm_last_kernel_time then covers every attempt); with PM_SEED_DEBUG bit 5 set
 * on the pair plan also out[3] blocks of 1024 positions, out[4] rounds of its second pass, out[5] key hits, summed over
 * waves and field pairs; out[6] times pm_scan halved its piece length since pm_init because a range's record lists would have
 * outgrown its bound (hit-dense text); out[7] look-ahead scans pm_scan / pm_scan_view enqueued since pm_init for the range
 * they expected next (see pm_scan_view).  While such a scan is in flight the call waits for it (it stays pm_scan's to
 * collect): out[1] and out[3..5] are then that scan's, out[0] the range's that was handed out.  out[8] suspects between
 * pm_pair_edit_scan and pm_pair_edit_resolve where the edit plan's first stage runs on the pair geometry (the pattern tile
 * with most; 0 elsewhere).  n <= 9 values are written. */
int pm_scan_stats(pm_handle *h, uint64_t *out, int n);

/* Measurement helper (no reference counterpart; DESIGN.md 4.6 "pair geometry for edits"): on a -K 2 handle of the pair plan,
 * time the 14-test pair geometry as the first stage of an edit-distance plan over the whole stream.  mode 1: substitution
 * compare (lower bound), mode 2: five-shift edit test on two patterns per slot.  No hits are produced.  Not on a windowed
 * handle (pm_init_windowed): PM_E_INVALID. */
int pm_measure_pair_edit_floor(pm_handle *h, int mode, float *ms, uint64_t *suspects);

/* Duration of the one-off re-encoding of the stream to 2 bits per base that pm_init[_device] runs
 * for the seed kernel family (0 for the bit-parallel family): not part of a scan, reported so that a
 * reader can add it to a single cold pass.  On a resident pm_init_packed handle: the unpack kernel, which
 * writes the bytes and the 2-bit words in one pass (either kernel family). */
int pm_pack_time(pm_handle *h, float *ms);

/* pick_pattern_index's automatic choice (select.cc:101-141) without a handle. */
int pm_pick_semantics(int32_t alphabet_size, int32_t acgt_normalized, int32_t k, int32_t wildcards,
                      int32_t npat, const int32_t *patlen, const int32_t *esb, const int32_t *eeb);

/* Measurement helper (no reference counterpart; SURVEY.md 8(d) "measured ceiling from the same
 * box"): streams `bytes` of HBM at d_buf (16-byte aligned) through 16-byte loads `reps` times on
 * `stream` and reports the read rate in GB/s. */
int pm_measure_stream_read(const void *d_buf, size_t bytes, int reps, void *stream, float *gbytes_per_s);

#ifdef __cplusplus
}
#endif
#endif
