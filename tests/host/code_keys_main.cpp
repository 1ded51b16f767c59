// Stand-alone check of the host side of the pattern collector (csrc/code_keys.h), built with
// -fsanitize=address,undefined by tests/test_code_keys_cpu.py: tables as the device kernel leaves them.
#include "code_keys.h"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace nss;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// `count` distinct patterns scattered over an otherwise free table
static std::vector<unsigned long long> table_with(int count, std::mt19937_64& rng, std::vector<unsigned long long>& put) {
  std::vector<unsigned long long> t(kCodeSlots, kCodeEmpty);
  put.clear();
  while (int(put.size()) < count) {
    const unsigned long long v = rng();
    if (v == kCodeEmpty || std::find(put.begin(), put.end(), v) != put.end()) continue;
    size_t h = size_t(rng() % kCodeSlots);
    while (t[h] != kCodeEmpty) h = (h + 1) % kCodeSlots;
    t[h] = v;
    put.push_back(v);
  }
  return t;
}

int main() {
  std::mt19937_64 rng(7);
  std::vector<unsigned long long> keys, put;
  for (int count : {1, 2, 7, 255, 256}) {
    auto t = table_with(count, rng, put);
    const int32_t state[4] = {count, 0, 0, 0};
    CHECK(code_keys_from_table(t.data(), kCodeSlots, state, 256, keys));
    std::sort(put.begin(), put.end());
    CHECK(keys == put);
    CHECK(std::is_sorted(keys.begin(), keys.end()) && std::adjacent_find(keys.begin(), keys.end()) == keys.end());
  }
  {   // the pattern that marks a free slot occurs as a value: last key, counted
    auto t = table_with(255, rng, put);
    const int32_t state[4] = {256, 0, 1, 0};
    CHECK(code_keys_from_table(t.data(), kCodeSlots, state, 256, keys));
    CHECK(keys.size() == 256 && keys.back() == kCodeEmpty);
    auto t2 = table_with(256, rng, put);     // ... as the 257th
    CHECK(!code_keys_from_table(t2.data(), kCodeSlots, state, 256, keys) && keys.empty());
  }
  {   // more than the limit, a collector that gave up, nothing seen, a full table
    auto t = table_with(257, rng, put);
    const int32_t ok[4] = {257, 0, 0, 0}, gave_up[4] = {12, 1, 0, 0}, none[4] = {0, 0, 0, 0};
    CHECK(!code_keys_from_table(t.data(), kCodeSlots, ok, 256, keys) && keys.empty());
    auto t7 = table_with(7, rng, put);
    CHECK(!code_keys_from_table(t7.data(), kCodeSlots, gave_up, 256, keys) && keys.empty());
    std::vector<unsigned long long> free_table(kCodeSlots, kCodeEmpty);
    CHECK(!code_keys_from_table(free_table.data(), kCodeSlots, none, 256, keys) && keys.empty());
    auto full = table_with(kCodeSlots, rng, put);
    CHECK(!code_keys_from_table(full.data(), kCodeSlots, ok, 256, keys) && keys.empty());
    CHECK(code_keys_from_table(full.data(), kCodeSlots, ok, kCodeSlots, keys) && keys.size() == size_t(kCodeSlots));
  }
  // the dictionary budget of the block codes: 16 KiB
  CHECK(block_dictionary_fits(7, 6, 16384) && block_dictionary_fits(256, 8, 16384) && !block_dictionary_fits(256, 9, 16384));
  CHECK(block_dictionary_fits(15, 136, 16384) && !block_dictionary_fits(16, 136, 16384) && !block_dictionary_fits(40, 136, 16384));
  CHECK(block_dictionary_fits(8, 256, 16384) && !block_dictionary_fits(9, 256, 16384) && !block_dictionary_fits(0, 6, 16384));
  std::printf(failures ? "%d check(s) failed\n" : "code_keys ok\n", failures);
  return failures ? 1 : 0;
}
