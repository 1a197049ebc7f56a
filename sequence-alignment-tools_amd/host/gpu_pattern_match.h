// gpu_pattern_match.h -- C++ host side above the C ABI (include/pm_gpu.h).
//
// GpuPatternMatch has the shape of the reference's PatternMatch plugin
// (reference pattern_match.h:84-156): add_pattern / init / find_patterns / reset with the same
// argument meaning, hit triples and error convention (message on stderr, exit(1);
// pattern_match.h:122-123, select.cc:88-89).  Inside the reference tree it would derive from
// PatternMatch and take the reference's CharacterProducer; INTEGRATION.md shows that 30-line
// adapter and the select.cc hunk.  Stand-alone (this repo) it uses the minimal CharacterProducer
// view below, which declares exactly the virtuals of char_io.h:18-71 an engine may call.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/pm_gpu.h"
#include "pm_ranks.h"

namespace pmgpu {

class CharacterProducer {                       // reference char_io.h:18-71 (subset used by engines)
 public:
  virtual ~CharacterProducer() {}
  virtual unsigned char getnch() = 0;           // next stream byte (normalized code), advances
  virtual char ch(unsigned char nch) = 0;       // code -> character
  virtual int nch(char ch) = 0;                 // character -> code, -1 if absent
  virtual unsigned int size() const = 0;        // alphabet size (256 for raw streams)
  virtual int64_t length() const = 0;
  virtual bool eof() const = 0;
  virtual int64_t pos() const = 0;
  virtual void pos(int64_t p) = 0;
  virtual bool has_filename() const { return false; }
  virtual const char *c_str() const { return nullptr; }   // contiguous bytes when has_filename()
};

// What the in-memory streams below share: the alphabet table, the position, and random access to one code (the command
// lines look at single stream positions; a packed stream has no c_str() to index).
class StreamChars : public CharacterProducer {
 public:
  char ch(unsigned char c) override { return table_.empty() ? (char)c : table_[c]; }
  int nch(char c) override { return inv_[(unsigned char)c]; }
  unsigned int size() const override { return table_.empty() ? 256u : (unsigned)table_.size(); }
  int64_t length() const override { return n_; }
  bool eof() const override { return pos_ >= n_; }
  int64_t pos() const override { return pos_; }
  void pos(int64_t p) override { pos_ = p; }
  virtual unsigned char code_at(int64_t p) const = 0;   // the code getnch() returns at position p, 0 <= p < length()
 protected:
  explicit StreamChars(std::string table);              // table empty = raw stream
  int64_t n_ = 0;
  std::string table_;
  int inv_[256];
  int64_t pos_ = 0;
};

// A stream held in memory (what MapFileChars / Normalized<MapFileChars> are to the reference).
class BufferChars : public StreamChars {
 public:
  BufferChars(std::vector<unsigned char> bytes, std::string table);   // table empty = raw stream
  // bytes owned by someone else (a file mapping, seq_io.h) who outlives this object
  BufferChars(const unsigned char *data, size_t n, std::string table);
  unsigned char getnch() override { return data_[pos_++]; }
  unsigned char code_at(int64_t p) const override { return data_[p]; }
  bool has_filename() const override { return true; }
  const char *c_str() const override { return reinterpret_cast<const char *>(data_); }
 private:
  std::vector<unsigned char> bytes_;
  const unsigned char *data_ = nullptr;
};

// A bit-packed stream held in memory (<db>.sqz; what Compressed<> is to the reference, char_io.t:18-214): codes of
// `bits` bits, most significant bit first.  length() counts every whole code the bytes hold, the end-of-sequence codes
// that fill up compress_seq's last buffer included.  No c_str(): GpuPatternMatch::init hands the packed bytes to
// pm_init_packed, which unpacks them on the GPU.
class PackedChars : public StreamChars {
 public:
  PackedChars(std::vector<unsigned char> packed, int bits, std::string table);
  // packed bytes owned by someone else (a file mapping, seq_io.h) who outlives this object
  PackedChars(const unsigned char *packed, size_t packed_bytes, int bits, std::string table);
  unsigned char getnch() override { return code_at(pos_++); }
  unsigned char code_at(int64_t p) const override {      // a code spans at most two bytes
    const int64_t bit = p * bits_, b = bit >> 3;
    const unsigned w = ((unsigned)data_[b] << 8) | (b + 1 < bytes_n_ ? data_[b + 1] : 0u);
    return (unsigned char)((w >> (16 - bits_ - (int)(bit & 7))) & ((1u << bits_) - 1u));
  }
  const unsigned char *packed() const { return data_; }
  int64_t packed_bytes() const { return bytes_n_; }
  int bits() const { return bits_; }
 private:
  std::vector<unsigned char> bytes_;
  const unsigned char *data_ = nullptr;
  int64_t bytes_n_ = 0;
  int bits_ = 8;
};

struct pattern_hit {                            // one element of pattern_hit_vector (pattern_match.h:82)
  int64_t key;                                  // stream index after the last matched char
  unsigned long id;                             // pattern_list_element::id()
  unsigned char value;                          // errors
};
typedef std::vector<pattern_hit> pattern_hit_vector;

class GpuPatternMatch {
 public:
  // kernel: PM_KERNEL_AUTO / PM_KERNEL_BITPAR (-N 16) / PM_KERNEL_SEED (-N 17); the other
  // arguments are pick_pattern_index's (select.cc:19-30).  semantics forces a reference engine.
  // group: the ranks of a position-sharded run (pm_ranks.h), or null / single.  With N ranks every
  // rank scans its own shard of the stream on its own GPU and rank 0's find_patterns hands out the
  // hits of the WHOLE stream; the other ranks' find_patterns returns nothing.
  // Environment: PM_GPU_LONG=1 .. 255 sets pm_config.long_patterns, a bit set (1: -K 1 / -K 2 primers of 33..64 nt on the
  // pair plan; 2: k = 0 primers of 33..64 nt on the seed plan; 4: -k 1 / -k 2 primers of 33..64 nt on the edit plan;
  // 8: exact_halves -k 1 / -k 2 primers of 33..64 nt on the halves plan; 16: with indels, hits of primers of 33..64 nt re-aligned on the device; 32: -w primers of 16..32 nt with more than 16 concrete variants on pm_wild_sub_scan; 64: the -k 1 / -k 2 edit plan's first stage on the pair geometry for every tile, at -k 1 and under exact_bases; 128: together with 32, such -w primers of 33..64 nt on that class as well; sums combine them; default and any other value: 0), read where PM_GPU_PACKED and PM_GPU_WINDOW are: by this class, for every program built on it.
  GpuPatternMatch(int kernel, unsigned int k, char eos = '\n', bool wc = false, bool tn = false,
                  bool indels = true, bool dna_mut = false, int semantics = PM_SEM_AUTO, int device = 0,
                  RankGroup *group = nullptr);
  ~GpuPatternMatch();
  unsigned long add_pattern(std::string const &pat, unsigned long id = 0, int exact_start_bases = 0,
                            int exact_end_bases = 0);                         // pattern_match.h:116
  void init(CharacterProducer &cp);                                           // pattern_match.h:130
  bool find_patterns(CharacterProducer &cp, pattern_hit_vector &hits, unsigned long minka = 1);  // :131
  void reset();                                                               // :134
  // find_patterns over the rest of the stream plus the caller's tally loop (primer_match.cc:1118-1268, -c [-M max_count])
  // with nothing handed out (pm_count_scan / pm_counts): counts[i * (k + 1) + d] and capped[i] for the i-th added
  // pattern, the tally of the whole pass since the last reset().  One rank only: the cap depends on the order of a
  // pattern's hits across the shards.
  void count_patterns(CharacterProducer &cp, uint64_t max_count, std::vector<uint64_t> &counts, std::vector<uint8_t> &capped,
                      pm_count_info *info = nullptr);
  // One round of pcr_match's scan + pairing loop with the pairing stage on the device (pm_pcr_scan / pm_pcr_pair, after a
  // pm_pcr_setup on handle()): the ranges find_patterns would walk are scanned until >= minka hits have joined the held
  // list or the stream ends, then the held hits are paired with scanned_to = cp.pos().  Returns what find_patterns would
  // (hits arrived); the survivors and their strings (at (2i, 2i + 1) * stride) lie in the handle's pinned buffer until the
  // next call.  *new_hits: hits that arrived, *scan_seconds: the share of pm_pcr_scan.
  bool pcr_round(CharacterProducer &cp, unsigned long minka, size_t stride, const pm_pcr_amplicon **out, size_t *n, const char **ops,
                 const char **text, size_t *new_hits, double *scan_seconds);
  bool resident() const;                                                      // the whole stream is in HBM (no windows, one rank)
  bool sharded() const { return group_ != nullptr; }
  int selected_semantics() const;
  int selected_kernel() const;
  void chunk_bytes(int64_t c) { chunk_ = c; }
  void verbose(bool v) { verbose_ = v; }                                      // -v: init names the stream's residency mode
  // for the caller's per-hit re-alignment (pm_align_hits_text): the handle that knows the whole stream
  pm_handle *handle() const { return merge_ ? merge_ : h_; }
 private:
  [[noreturn]] void fatal(const char *what) const;
  bool sharded_scan(CharacterProducer &cp, pattern_hit_vector &hits);
  pm_handle *h_ = nullptr;
  pm_handle *merge_ = nullptr;                  // rank 0 of a sharded run: host-stage handle over the whole stream (pm_init_host)
  pm_comm *comm_ = nullptr;                     // RCCL communicator when every rank has its own GPU
  RankGroup *group_ = nullptr;
  int64_t shard_ = 0, lo_ = 0, hi_ = 0, glo_ = 0, ghi_ = 0;   // this rank's slice of the stream and what it holds around it
  bool sharded_done_ = false;
  std::vector<unsigned char> owned_;            // stream drained from a producer without c_str()
  int64_t n_ = 0;
  int64_t chunk_ = (int64_t)1 << 30;
  unsigned long next_id_ = 0;
  size_t npat_ = 0;
  unsigned int k_ = 0;
  int device_ = 0;
  bool verbose_ = false;
};

}  // namespace pmgpu
