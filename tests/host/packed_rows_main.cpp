// Stand-alone check of the packed per-row index words (csrc/packed_rows.h), built with -fsanitize=address,undefined by
// tests/test_packed_rows_cpu.py: the twenty-byte row-slot words and the 16-bit column pairs, pack against unpack.
#include "packed_rows.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace nss;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// pack, then every field back: the length, the live slots' positions and codes, zeros in the slots behind the length
static bool round_trip(int len, const uint32_t* pos, const uint32_t* code) {
  PackedSlotRow row;
  for (uint32_t& w : row.u) w = 0xdeadbeefu;
  if (!pack_slot_row(len, pos, code, &row)) return false;
  bool ok = int(packed_slot_len(row.u)) == len;
  for (int k = 0; k < kPackedSlots; ++k) {
    const uint32_t p = packed_slot_pos(row.u, k), c = packed_slot_code(row.u, k);
    ok = ok && (k < len ? (p == pos[k] && c == code[k]) : (p == 0 && c == 0));
  }
  ok = ok && (row.u[2] >> 28) == 0;                         // the bits above the length stay zero
  return ok;
}

static void row_slot_words() {
  static_assert(sizeof(PackedSlotRow) == kPackedRowBytes, "five words");
  static_assert(kPackedLenBit + 4 <= 96, "positions and length fit three words");
  uint32_t pos[kPackedSlots], code[kPackedSlots];
  // every length, each with all-zero and all-ones fields
  for (int len = 0; len <= kPackedSlots; ++len) {
    for (uint32_t fill : {0u, 1u}) {
      for (int k = 0; k < kPackedSlots; ++k) {
        pos[k] = fill ? kPackedPosLimit - 1 : 0u;
        code[k] = fill ? 0xffu : 0u;
      }
      CHECK(round_trip(len, pos, code));
    }
  }
  // positions 0 and 2047 and all 256 codes in every slot, the other slots holding the opposite pattern
  for (int slot = 0; slot < kPackedSlots; ++slot) {
    for (uint32_t p : {0u, kPackedPosLimit - 1}) {
      for (uint32_t c = 0; c < 256; ++c) {
        for (int k = 0; k < kPackedSlots; ++k) {
          pos[k] = p ? 0u : kPackedPosLimit - 1;
          code[k] = ~c & 0xffu;
        }
        pos[slot] = p;
        code[slot] = c;
        CHECK(round_trip(kPackedSlots, pos, code));
        if (slot + 1 < kPackedSlots) CHECK(round_trip(slot + 1, pos, code));   // ... as the row's last entry
      }
    }
  }
  // random rows
  std::mt19937 rng(11);
  for (int trial = 0; trial < 20000; ++trial) {
    const int len = int(rng() % (kPackedSlots + 1));
    for (int k = 0; k < kPackedSlots; ++k) {
      pos[k] = rng() % kPackedPosLimit;
      code[k] = rng() % 256;
    }
    CHECK(round_trip(len, pos, code));
  }
  // refusals: nine entries, a negative length, a position of 2048, a code of 256 -- and nothing is written
  for (int k = 0; k < kPackedSlots; ++k) pos[k] = code[k] = 1;
  PackedSlotRow row;
  for (uint32_t& w : row.u) w = 0x12345678u;
  uint32_t pos9[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1}, code9[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
  CHECK(!pack_slot_row(9, pos9, code9, &row));
  CHECK(!pack_slot_row(-1, pos, code, &row));
  pos[7] = kPackedPosLimit;
  CHECK(!pack_slot_row(8, pos, code, &row) && pack_slot_row(7, pos, code, &row));   // (behind the length: not looked at)
  for (uint32_t& w : row.u) w = 0x12345678u;
  pos[7] = 1;
  code[0] = 256;
  CHECK(!pack_slot_row(8, pos, code, &row));
  for (uint32_t w : row.u) CHECK(w == 0x12345678u);
}

static void column_words() {
  // window offsets 0 and 65534 are accepted, 65535 is refused; no live slot: accepted, base 0
  CHECK(col16_window_fits(7, 7) && col16_window_fits(7, 7 + 65534) && !col16_window_fits(7, 7 + 65535));
  CHECK(col16_window_fits(0, 65534) && !col16_window_fits(0, 65535));
  CHECK(col16_window_fits(2147418113ll, 2147483647ll) && !col16_window_fits(2147418112ll, 2147483647ll));
  CHECK(col16_window_fits(2147483647ll, -1) && col16_window_base(2147483647ll, -1) == 0);
  CHECK(col16_window_base(12, 40) == 12);
  for (int32_t base : {0, 1, 12345, 2147483647 - 65534}) {
    for (int32_t off0 : {0, 1, 255, 256, 65533, 65534}) {
      for (int32_t off1 : {0, 1, 32768, 65534}) {
        const uint32_t both = pack_col16_pair(base + off0, base + off1, base);
        CHECK(col16_live(both, 0) && col16_live(both, 1));
        CHECK(col16_gather_column(both, 0, base) == base + off0 && col16_gather_column(both, 1, base) == base + off1);
        const uint32_t first = pack_col16_pair(base + off0, -1, base);       // one entry: slot 1 is padding
        CHECK(col16_live(first, 0) && !col16_live(first, 1));
        CHECK(col16_gather_column(first, 0, base) == base + off0 && col16_gather_column(first, 1, base) == base);
      }
    }
    const uint32_t none = pack_col16_pair(-1, -1, base);                    // an empty row gathers from the base twice
    CHECK(none == 0xffffffffu && !col16_live(none, 0) && !col16_live(none, 1));
    CHECK(col16_gather_column(none, 0, base) == base && col16_gather_column(none, 1, base) == base);
  }
  // a row block with no live slot: base 0, every slot gathers from column 0
  const int32_t base = col16_window_base(2147483647ll, -1);
  const uint32_t w = pack_col16_pair(-1, -1, base);
  CHECK(col16_gather_column(w, 0, base) == 0 && col16_gather_column(w, 1, base) == 0);
  // random pairs inside random windows
  std::mt19937 rng(13);
  for (int trial = 0; trial < 20000; ++trial) {
    const int32_t b = int32_t(rng() % 2147418113u);
    const int32_t c0 = (rng() & 3) ? b + int32_t(rng() % 65535u) : -1, c1 = (rng() & 3) ? b + int32_t(rng() % 65535u) : -1;
    const uint32_t word = pack_col16_pair(c0, c1, b);
    CHECK(col16_live(word, 0) == (c0 >= 0) && col16_live(word, 1) == (c1 >= 0));
    CHECK(col16_gather_column(word, 0, b) == (c0 >= 0 ? c0 : b) && col16_gather_column(word, 1, b) == (c1 >= 0 ? c1 : b));
  }
}

int main() {
  row_slot_words();
  column_words();
  std::printf(failures ? "%d check(s) failed\n" : "packed_rows ok\n", failures);
  return failures ? 1 : 0;
}
