// pm_bits.h -- what the scan kernels of pm_seed.hip, pm_pair.hip and pm_short.hip share below the level of a plan: the
// compile-time loop, bit fields at compile-time offsets of a string of stream words, the load of one stream word, the two
// words a wave carries in from in front of its range, and the mask of a lane's 16 windows that lie inside a range.  (The
// writer of their output lists is pm_slots.h.)
#pragma once
#include <cstdint>
#include <utility>

#include <hip/hip_runtime.h>

namespace pm {

namespace {

// f(integral_constant<int, 0>()), ..., f(integral_constant<int, N - 1>()) in order: the index is a constant inside f
template <int... Is, typename F>
__device__ __forceinline__ void static_each(std::integer_sequence<int, Is...>, F &&f) { (f(std::integral_constant<int, Is>()), ...); }
template <int N, typename F>
__device__ __forceinline__ void static_for(F &&f) { static_each(std::make_integer_sequence<int, N>(), f); }

// 32 bits from bit O (compile time) of the string w0 : w1 : ... of 32-bit words (bit 0 = bit 0 of w0); what lies beyond
// the last word reads as zero
template <int O>
__device__ __forceinline__ uint32_t bits_at(uint32_t w0) {
  static_assert(O >= 0 && O < 32, "offset");
  if constexpr (O == 0) return w0;
  else return w0 >> O;
}
template <int O, typename... W>
__device__ __forceinline__ uint32_t bits_at(uint32_t w0, uint32_t w1, W... more) {
  static_assert(O >= 0, "offset");
  if constexpr (O == 0) return w0;
  else if constexpr (O < 32) return __builtin_amdgcn_alignbit(w1, w0, O);
  else return bits_at<O - 32>(w1, more...);
}

// One dword of the 2-bit packed stream = the 16 bases from `pos` (a multiple of 16) on; zero outside the stream.
// NT: a non-temporal load (a stream that is read once and must not push the tables out of L2).
template <bool NT = false>
__device__ __forceinline__ uint32_t load_packed(const uint32_t *packed, int64_t npacked, int64_t pos) {
  const int64_t i = pos >> 4;
  if (pos < 0 || i >= npacked) return 0u;
  return NT ? __builtin_nontemporal_load(packed + i) : packed[i];
}

// The two dwords in front of a wave's range (ws a multiple of 16): carry2 = the bases ws - 32 .. ws - 17, carry1 = the
// bases ws - 16 .. ws - 1, both wave-uniform -- what lane 0 and lane 1 of the range's first block borrow.
template <bool NT = false>
__device__ __forceinline__ void load_carry(const uint32_t *packed, int64_t npacked, int64_t ws, int lane, uint32_t &carry1, uint32_t &carry2) {
  const uint32_t pk = load_packed<NT>(packed, npacked, ws - 32 + 16 * (lane & 1));
  carry2 = __builtin_amdgcn_readlane(pk, 0);
  carry1 = __builtin_amdgcn_readlane(pk, 1);
}

// A lane's 16 windows end at pbase .. pbase + 15: bit j is set iff lo <= pbase + j < hi
__device__ __forceinline__ uint32_t own_mask16(int64_t pbase, int64_t lo, int64_t hi) {
  const int64_t l = lo - pbase, h = hi - pbase;
  const uint32_t lb = l <= 0 ? 0u : (l >= 16 ? 16u : (uint32_t)l), hb = h <= 0 ? 0u : (h >= 16 ? 16u : (uint32_t)h);
  return ((1u << hb) - 1u) & ~((1u << lb) - 1u);
}

}  // namespace

}  // namespace pm
