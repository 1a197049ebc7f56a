// pm_slots.h -- the one writer of record lists whose slots a wave reserves a block at a time: the seed lists, suspect
// lists and pm_hit record buffers of pm_seed.hip and pm_short.hip.  Device only, like pm_bits.h.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "pm_internal.h"

namespace pm {

namespace {

// how an unused slot is marked: an 8-byte seed record / suspect is ~0 as a whole; of a pm_hit only the pid is stored
__device__ __forceinline__ void mark_hole(uint64_t *slot) { *slot = ~0ull; }
__device__ __forceinline__ void mark_hole(pm_hit *slot) { slot->pid = PM_SEED_HOLE; }

// A wave's slots of an output list: reserved BLOCK at a time with one atomic on the list's counter (one counter serves every
// wave of the grid and same-address atomics serialise: 10^7 of them cost 25 ms); the slots of a block the wave does not
// fill are marked as holes (mark_hole: the reader skips them), and nothing is written at or beyond the list's capacity (the
// counter goes on counting: the caller grows the list and scans again).  All members are wave-uniform.
template <int BLOCK, typename Rec = uint64_t>
struct SlotBlocks {
  static_assert(BLOCK % 64 == 0, "whole waves");
  Rec *list;
  unsigned long long *count;
  unsigned long long cap;
  unsigned long long next = 0;          // next free slot of the reserved block
  int left = 0;

  // (&list[next + u], not list + next + u: the second form cost every scan kernel two VGPRs)
  __device__ __forceinline__ void mark_unused(int lane) const {
#pragma unroll
    for (int u = lane; u < BLOCK; u += 64) if (u < left && next + u < cap) mark_hole(&list[next + u]);
  }
  // the records of the lanes with `pass`, in lane order (called by the whole wave)
  __device__ __forceinline__ void put(int lane, bool pass, Rec rec) {
    const unsigned long long bal = __ballot(pass);
    if (bal == 0) return;
    const int c = __popcll(bal);
    if (c > left) {                                                  // a fresh block; what is left of the old one is marked unused
      mark_unused(lane);
      unsigned long long got = 0;
      if (lane == 0) got = atomicAdd(count, (unsigned long long)BLOCK);
      next = ((unsigned long long)__builtin_amdgcn_readfirstlane((uint32_t)(got >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)got);
      left = BLOCK;
    }
    if (pass) {
      const unsigned long long slot = next + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
      if (slot < cap) list[slot] = rec;
    }
    next += c; left -= c;
  }
};

}  // namespace

}  // namespace pm
