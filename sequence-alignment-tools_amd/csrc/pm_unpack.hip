// pm_unpack.hip -- a bit-packed stream (<db>.sqz: codes of BITS bits, most significant bit first, char_io.t:18-214)
// unpacked in HBM, in one pass, into the two forms the scan kernels read: one byte per base, and the 2-bit words of
// pm_pack_stream (pm_seed.hip: dword i = bases 16i .. 16i+15, base j in bits 2j).
//
// Layout of the work: one lane = 16 consecutive bases = 2*BITS packed bytes in, one 16-byte store of text and one dword
// of 2-bit words out.  Consecutive lanes own consecutive groups, so a wave's text store covers 1 KiB and its word store
// 256 B without a gap.  16 codes are 2*BITS bytes: a lane's input starts on a 2-byte boundary of the packed bytes (on a
// 4-byte boundary when BITS is even); it loads the aligned dwords that cover it (neighbours share them in L1),
// byte-swaps them into MSB-first order and shifts the array by 16 bits where its start is the odd half of a dword.
// From there every code sits at a bit offset known at compile time.  A lane has UNP_GROUPS groups in flight, one block
// of 256 lanes apart, so that the loads of all of them are issued before the first is used.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pm_gpu.h"
#include "pm_internal.h"

namespace {

constexpr int UNP_THREADS = 256;
constexpr int UNP_GROUPS = 4;        // groups of 16 bases per lane

// 4 stream bytes -> 8 bits, 2 bits per base (byte 0 in bits 0-1): pm_seed.hip pack4, restated so that the words made
// here are the words pm_pack_stream makes from the same bytes
__device__ __forceinline__ uint32_t unp_pack4(uint32_t x, int sh) {
  uint32_t y = (x >> sh) & 0x03030303u;
  y |= y >> 6;
  return (y | (y >> 12)) & 0xffu;
}

// dwords that cover 2*BITS bytes starting on a 2-byte boundary (a 4-byte boundary when BITS is even)
template <int BITS> struct UnpackShape {
  static constexpr int ND = (BITS % 2 == 0) ? BITS / 2 : (2 * BITS + 5) / 4;   // loaded
  static constexpr int NW = (2 * BITS + 3) / 4;                                // after the 16-bit shift
};

// byte `i` of the packed input, zero past its end
__device__ __forceinline__ uint32_t unp_byte(const uint8_t *p, int64_t i, int64_t bytes) { return i < bytes ? p[i] : 0u; }

template <int BITS>
__global__ __launch_bounds__(UNP_THREADS) void pm_unpack_stream(const uint32_t *__restrict__ packed, int64_t packed_bytes, int64_t n, int sh,
                                                                uint4 *__restrict__ text, uint32_t *__restrict__ words, int64_t ngroups) {
  constexpr int ND = UnpackShape<BITS>::ND, NW = UnpackShape<BITS>::NW;
  constexpr uint32_t MASK = (1u << BITS) - 1u;
  const int64_t g0 = (int64_t)blockIdx.x * (UNP_THREADS * UNP_GROUPS) + threadIdx.x;
  uint32_t w[UNP_GROUPS][ND + 1];
  bool odd[UNP_GROUPS];
#pragma unroll
  for (int u = 0; u < UNP_GROUPS; ++u) {
    const int64_t g = g0 + (int64_t)u * UNP_THREADS;
    const int64_t off = g * (2 * BITS);                  // first packed byte of the group
    const int64_t a = off & ~(int64_t)3;
    odd[u] = (BITS % 2) && (off & 2);
#pragma unroll
    for (int i = 0; i <= ND; ++i) w[u][i] = 0;
    if (g >= ngroups) continue;
    if (a + 4 * ND <= packed_bytes) {
#pragma unroll
      for (int i = 0; i < ND; ++i) w[u][i] = __builtin_bswap32(packed[(a >> 2) + i]);
    } else {                                             // the tail of the buffer: byte by byte, nothing read past it
      const uint8_t *pb = reinterpret_cast<const uint8_t *>(packed);
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        const int64_t b = a + 4 * i;
        w[u][i] = (unp_byte(pb, b, packed_bytes) << 24) | (unp_byte(pb, b + 1, packed_bytes) << 16) |
                  (unp_byte(pb, b + 2, packed_bytes) << 8) | unp_byte(pb, b + 3, packed_bytes);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < UNP_GROUPS; ++u) {
    const int64_t g = g0 + (int64_t)u * UNP_THREADS;
    if (g >= ngroups) continue;
    uint32_t v[NW + 1];
#pragma unroll
    for (int i = 0; i < NW; ++i) v[i] = odd[u] ? ((w[u][i] << 16) | (w[u][i + 1] >> 16)) : w[u][i];
    v[NW] = 0;
    uint32_t t[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int s = j * BITS, wi = s >> 5, o = s & 31;   // constants after unrolling
      uint32_t c;
      if (o + BITS <= 32) c = (v[wi] >> (32 - o - BITS)) & MASK;
      else c = (uint32_t)(((((uint64_t)v[wi]) << 32) | v[wi + 1]) >> (64 - o - BITS)) & MASK;
      t[j >> 2] |= c << (8 * (j & 3));
    }
    const int64_t left = n - 16 * g;                     // bases of this group inside the stream
    if (left < 16) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t r = left - 4 * q;
        t[q] = r >= 4 ? t[q] : r <= 0 ? 0u : (t[q] & ((1u << (8 * (int)r)) - 1u));
      }
    }
    text[g] = make_uint4(t[0], t[1], t[2], t[3]);
    if (words) words[g] = unp_pack4(t[0], sh) | (unp_pack4(t[1], sh) << 8) | (unp_pack4(t[2], sh) << 16) | (unp_pack4(t[3], sh) << 24);
  }
}

template <int BITS>
hipError_t unpack_launch(const void *d_packed, int64_t packed_bytes, int64_t n, int sh, void *d_text, void *d_words, hipStream_t st) {
  const int64_t ngroups = (n + 15) / 16;
  const int64_t per_block = (int64_t)UNP_THREADS * UNP_GROUPS;
  hipLaunchKernelGGL(pm_unpack_stream<BITS>, dim3((unsigned)((ngroups + per_block - 1) / per_block)), dim3(UNP_THREADS), 0, st,
                     reinterpret_cast<const uint32_t *>(d_packed), packed_bytes, n, sh, reinterpret_cast<uint4 *>(d_text),
                     reinterpret_cast<uint32_t *>(d_words), ngroups);
  return hipGetLastError();
}

}  // namespace

namespace pm {

hipError_t unpack_stream(const void *d_packed, int64_t packed_bytes, int bits, int64_t n, bool ascii, void *d_text, uint32_t *d_words, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const int sh = ascii ? 1 : 0;
  switch (bits) {
    case 1: return unpack_launch<1>(d_packed, packed_bytes, n, sh, d_text, d_words, st);
    case 2: return unpack_launch<2>(d_packed, packed_bytes, n, sh, d_text, d_words, st);
    case 3: return unpack_launch<3>(d_packed, packed_bytes, n, sh, d_text, d_words, st);
    case 4: return unpack_launch<4>(d_packed, packed_bytes, n, sh, d_text, d_words, st);
    case 5: return unpack_launch<5>(d_packed, packed_bytes, n, sh, d_text, d_words, st);
    case 6: return unpack_launch<6>(d_packed, packed_bytes, n, sh, d_text, d_words, st);
    case 7: return unpack_launch<7>(d_packed, packed_bytes, n, sh, d_text, d_words, st);
    case 8: return unpack_launch<8>(d_packed, packed_bytes, n, sh, d_text, d_words, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace pm

extern "C" int pm_unpack_device(const void *d_packed, int64_t packed_bytes, int32_t bits, int64_t n, void *d_text, void *d_words, void *hip_stream) {
  if (bits < 1 || bits > 8 || n < 0 || packed_bytes < 0 || (n > 0 && (!d_packed || !d_text))) return PM_E_INVALID;
  if (packed_bytes > ((int64_t)1 << 59) || n > packed_bytes * 8 / bits) return PM_E_INVALID;
  if (((uintptr_t)d_packed & 7) || ((uintptr_t)d_text & 15) || ((uintptr_t)d_words & 3)) return PM_E_INVALID;
  return pm::unpack_stream(d_packed, packed_bytes, bits, n, false, d_text, (uint32_t *)d_words, (hipStream_t)hip_stream) == hipSuccess ? PM_OK : PM_E_HIP;
}
