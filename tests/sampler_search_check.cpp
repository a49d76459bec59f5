// Stand-alone check of csrc/rgcn_sorted_search.h, the only index arithmetic of the constrained sampler that is not a
// clamp: rgcn_lower_bound against std::lower_bound on exactly sized heap arrays (so that AddressSanitizer sees any
// read outside them), for every length around the fan-out's boundaries, offsets, duplicates, values below / above
// the range, a long array, and arrays that are NOT ascending (any answer, but no read outside).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "primekg_rgcn_linkprediction_amd/csrc/rgcn_sorted_search.h"

int main() {
  std::mt19937_64 gen(1);
  long checked = 0;
  for (int n = 0; n <= 600; ++n) {
    for (int rep = 0; rep < 8; ++rep) {
      const int64_t lo = rep % 3;
      std::vector<int64_t> a(lo + n);                        // exactly [0, hi)
      for (auto& x : a) x = (int64_t)(gen() % (uint64_t)(n / 2 + 3));
      std::sort(a.begin() + lo, a.end());
      const int64_t hi = (int64_t)a.size();
      for (int64_t v = -1; v <= n / 2 + 3; ++v) {
        const int64_t want = std::lower_bound(a.begin() + lo, a.end(), v) - a.begin();
        if (rgcn_lower_bound(a.data(), lo, hi, v) != want) {
          std::printf("mismatch: n=%d lo=%ld v=%ld\n", n, (long)lo, (long)v);
          return 1;
        }
        ++checked;
      }
      std::shuffle(a.begin(), a.end(), gen);                 // malformed input: the result is unspecified, the reads are not
      const int64_t at = rgcn_lower_bound(a.data(), lo, hi, n / 4);
      if (at < lo || at > hi) {
        std::printf("out of range on unsorted input: n=%d\n", n);
        return 1;
      }
    }
  }
  std::vector<int64_t> big(200001);
  for (size_t i = 0; i < big.size(); ++i) big[i] = 3 * (int64_t)i;
  for (int64_t v = -2; v < 600010; v += 7) {
    const int64_t want = std::lower_bound(big.begin(), big.end(), v) - big.begin();
    if (rgcn_lower_bound(big.data(), 0, (int64_t)big.size(), v) != want) {
      std::printf("mismatch in the long array at %ld\n", (long)v);
      return 1;
    }
    ++checked;
  }
  std::printf("sampler_search_check ok %ld\n", checked);
  return 0;
}
