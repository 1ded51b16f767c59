// Packed per-row index words of the row-per-lane kernels: the twenty-byte row-slot words (csr_slots_rows) and the 16-bit
// column pairs of the coded fixed-width copy (csr_direct_rows).  Pack and unpack are defined once, as plain C++ for host
// and device, so that a stand-alone program can run them under the sanitizers (tests/host/packed_rows_main.cpp).
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define NSS_HD __host__ __device__ inline
#else
#define NSS_HD inline
#endif

namespace nss {

// A row of the row-slot copy in 20 bytes, five 32-bit words u[0..4]:
//   u[0..2]  one little-endian bit string: staged position k (CSR entry order) in bits 11 k ... 11 k + 10, k = 0 ... 7,
//            the row length (0 ... 8) in bits 88 ... 91, zeros above;
//   u[3]     the codes of slots 0 ... 3, slot k in bits 8 k ... 8 k + 7;  u[4]: those of slots 4 ... 7.
// A slot at or behind the length holds position 0 and code 0.  The kernels read u[0..3] as one aligned 16-byte word and
// u[4] from an array of its own, both unit-stride across the lanes.
constexpr int kPackedSlots = 8;
constexpr int kPackedPosBits = 11;
constexpr uint32_t kPackedPosLimit = 1u << kPackedPosBits;    // positions are below this: the chunk may not exceed it
constexpr int kPackedLenBit = kPackedSlots * kPackedPosBits;  // 88
constexpr int kPackedRowBytes = 20;

struct PackedSlotRow {
  uint32_t u[5];
};

// false -- nothing written -- when the row does not fit: more than eight entries, or a position of 2048 or more
NSS_HD bool pack_slot_row(int len, const uint32_t* pos, const uint32_t* code, PackedSlotRow* out) {
  if (len < 0 || len > kPackedSlots) return false;
  for (int k = 0; k < len; ++k)
    if (pos[k] >= kPackedPosLimit || code[k] > 0xffu) return false;
  uint32_t u[5] = {0u, 0u, 0u, 0u, 0u};
  for (int k = 0; k < len; ++k) {
    const int bit = kPackedPosBits * k, w = bit / 32, s = bit % 32;
    u[w] |= pos[k] << s;
    if (s + kPackedPosBits > 32) u[w + 1] |= pos[k] >> (32 - s);
    u[3 + k / 4] |= code[k] << (8 * (k % 4));
  }
  u[kPackedLenBit / 32] |= uint32_t(len) << (kPackedLenBit % 32);
  for (int i = 0; i < 5; ++i) out->u[i] = u[i];
  return true;
}

NSS_HD uint32_t packed_slot_len(const uint32_t* u) { return (u[kPackedLenBit / 32] >> (kPackedLenBit % 32)) & 0xfu; }

// staged position of slot k (0 for an unused slot)
NSS_HD uint32_t packed_slot_pos(const uint32_t* u, int k) {
  const int bit = kPackedPosBits * k, w = bit / 32, s = bit % 32;
  uint32_t v = u[w] >> s;
  if (s + kPackedPosBits > 32) v |= u[w + 1] << (32 - s);
  return v & (kPackedPosLimit - 1u);
}

NSS_HD uint32_t packed_slot_code(const uint32_t* u, int k) { return (u[3 + k / 4] >> (8 * (k % 4))) & 0xffu; }

// The two columns of a row of the coded fixed-width copy in one 32-bit word: slot 0 in the low half, slot 1 in the high
// half, each the column's offset from the WINDOW BASE of the row's row block -- the smallest column of the block's live
// slots, 0 for a block without one -- or kCol16Pad for a padding slot (column -1 of the 32-bit copy).  A row block fits
// when its largest live column lies at most kCol16MaxWindow above its smallest.
constexpr uint32_t kCol16Pad = 0xffffu;
constexpr int64_t kCol16MaxWindow = 65534;

// (lo, hi: smallest and largest live column of the row block; hi < 0: none)
NSS_HD bool col16_window_fits(int64_t lo, int64_t hi) { return hi < 0 || hi - lo <= kCol16MaxWindow; }
NSS_HD int32_t col16_window_base(int64_t lo, int64_t hi) { return hi < 0 ? 0 : int32_t(lo); }

// c0, c1: columns of the two slots (negative: padding), each live one in [base, base + kCol16MaxWindow]
NSS_HD uint32_t pack_col16_pair(int32_t c0, int32_t c1, int32_t base) {
  const uint32_t lo = c0 < 0 ? kCol16Pad : uint32_t(c0 - base), hi = c1 < 0 ? kCol16Pad : uint32_t(c1 - base);
  return (lo & 0xffffu) | (hi << 16);
}

NSS_HD bool col16_live(uint32_t w, int slot) { return ((w >> (16 * slot)) & 0xffffu) != kCol16Pad; }
// the column the slot gathers from: its own, or the base column for a padding slot (a valid column: its product is
// dropped by a select)
NSS_HD int32_t col16_gather_column(uint32_t w, int slot, int32_t base) {
  const uint32_t off = (w >> (16 * slot)) & 0xffffu;
  return base + int32_t(off != kCol16Pad ? off : 0u);
}

}  // namespace nss
