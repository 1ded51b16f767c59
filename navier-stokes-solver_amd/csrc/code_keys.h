// Host side of the distinct-pattern collector (spmv.hip: code_collect_kernel) shared by the value codes of the matrices
// and the block codes of block Jacobi.  Plain C++ without the HIP runtime, so that a stand-alone program can run it
// under the sanitizers (tests/host/code_keys_main.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace nss {

constexpr int kCodeSlots = 1024;                          // open-addressing table (power of two, 4 x the dictionary)
constexpr uint64_t kCodeEmpty = ~uint64_t(0);             // free slot; the value with this very pattern is flagged apart

// The table the collector left (`slots` entries, kCodeEmpty = free) and its state words -- state[1]: gave up, state[2]:
// the pattern kCodeEmpty itself occurs -- as the ascending distinct patterns (ascending: the codes do not depend on the
// race of the insertions).  False, keys empty, when the collector gave up, nothing was seen or more than max_keys were.
inline bool code_keys_from_table(const unsigned long long* table, int slots, const int32_t* state, size_t max_keys,
                                 std::vector<unsigned long long>& keys) {
  keys.clear();
  if (state[1] != 0) return false;
  for (int i = 0; i < slots; ++i)
    if (table[i] != kCodeEmpty) keys.push_back(table[i]);
  if (state[2] != 0) keys.push_back(kCodeEmpty);
  std::sort(keys.begin(), keys.end());
  if (keys.empty() || keys.size() > max_keys) {
    keys.clear();
    return false;
  }
  return true;
}

// whether the dictionary of the block codes -- n_codes blocks of `doubles` entries -- fits `budget` bytes
inline bool block_dictionary_fits(size_t n_codes, int doubles, size_t budget) {
  return n_codes > 0 && doubles > 0 && n_codes * size_t(doubles) * sizeof(double) <= budget;
}

}  // namespace nss
