// Stand-alone check of what the path enumeration (csrc/paths.hip) shares between host and device:
//   - rgcn_path_before (csrc/rgcn_paths_order.h) is a strict total order on entries without NaN - irreflexive,
//     asymmetric, total on different entries, transitive - and sorting with it gives (score descending, -0.0 == +0.0,
//     then length, then interior nodes) as written here independently with a tuple;
//   - rgcn_path_weight is 1 / (L (1 + 0.2 (L - 1))) rounded once;
//   - the int32 rgcn_lower_bound (csrc/rgcn_sorted_search.h) against std::lower_bound on exactly sized heap arrays (so
//     that AddressSanitizer sees any read outside them), for every length around the fan-out's boundaries, offsets,
//     duplicates, values below / above the range, a long array, and arrays that are NOT ascending.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <tuple>
#include <vector>

#include "primekg_rgcn_linkprediction_amd/csrc/rgcn_paths_order.h"
#include "primekg_rgcn_linkprediction_amd/csrc/rgcn_sorted_search.h"

static std::tuple<float, int, int, int, int> key_of(const rgcn_path_entry& e) {
  return std::make_tuple(-(e.score + 0.f), e.len, e.n1, e.n2, e.n3);      // + 0.f: -0.0 becomes +0.0
}

int main() {
  std::mt19937_64 gen(3);
  long checked = 0;

  // ---- the order
  const float inf = std::numeric_limits<float>::infinity();
  const float scores[] = {-inf, -1.5f, -0.0f, 0.0f, 1e-30f, 0.25f, 0.25f, 1.0f, inf};
  std::vector<rgcn_path_entry> all;
  for (float s : scores)
    for (int len = 1; len <= RGCN_PATHS_MAX_LEN; ++len)
      for (int rep = 0; rep < 6; ++rep) {
        rgcn_path_entry e;
        e.score = s;
        e.len = len;
        e.n1 = len >= 2 ? (int)(gen() % 3) : -1;
        e.n2 = len >= 3 ? (int)(gen() % 3) : -1;
        e.n3 = len >= 4 ? (int)(gen() % 3) + (rep == 0 ? 2147483000 : 0) : -1;
        all.push_back(e);
      }
  for (const auto& a : all) {
    for (const auto& b : all) {
      const bool ab = rgcn_path_before(a, b), ba = rgcn_path_before(b, a);
      const bool same = key_of(a) == key_of(b);
      if ((same && (ab || ba)) || (!same && ab == ba) || ab != (key_of(a) < key_of(b))) {
        std::printf("order: not strict and total, or not the tuple order\n");
        return 1;
      }
      for (const auto& c : all)
        if (ab && rgcn_path_before(b, c) && !rgcn_path_before(a, c)) {
          std::printf("order: not transitive\n");
          return 1;
        }
      ++checked;
    }
  }
  std::vector<rgcn_path_entry> sorted = all;
  std::shuffle(sorted.begin(), sorted.end(), gen);
  std::sort(sorted.begin(), sorted.end(), rgcn_path_before);
  for (size_t i = 1; i < sorted.size(); ++i)
    if (key_of(sorted[i]) < key_of(sorted[i - 1])) {
      std::printf("order: sort disagrees with the tuple order at %zu\n", i);
      return 1;
    }
  const double want_w[] = {1.0, 1.0 / 2.4, 1.0 / 4.2, 1.0 / 6.4};
  for (int len = 1; len <= RGCN_PATHS_MAX_LEN; ++len)
    if (std::fabs((double)rgcn_path_weight(len) - want_w[len - 1]) > 6e-8 * want_w[len - 1]) {
      std::printf("weight of length %d\n", len);
      return 1;
    }
  if (rgcn_path_weight(1) != 1.0f || rgcn_path_weight(4) != 0.15625f) return 1;

  // ---- the int32 search
  for (int n = 0; n <= 600; ++n) {
    for (int rep = 0; rep < 8; ++rep) {
      const int lo = rep % 3;
      std::vector<int32_t> a(lo + n);                        // exactly [0, hi)
      for (auto& x : a) x = (int32_t)(gen() % (uint64_t)(n / 2 + 3));
      std::sort(a.begin() + lo, a.end());
      const int hi = (int)a.size();
      for (int32_t v = -1; v <= n / 2 + 3; ++v) {
        const int want = (int)(std::lower_bound(a.begin() + lo, a.end(), v) - a.begin());
        if (rgcn_lower_bound(a.data(), lo, hi, v) != want) {
          std::printf("search mismatch: n=%d lo=%d v=%d\n", n, lo, (int)v);
          return 1;
        }
        ++checked;
      }
      std::shuffle(a.begin(), a.end(), gen);                 // malformed input: the result is unspecified, the reads are not
      const int at = rgcn_lower_bound(a.data(), lo, hi, (int32_t)(n / 4));
      if (at < lo || at > hi) {
        std::printf("search out of range on unsorted input: n=%d\n", n);
        return 1;
      }
    }
  }
  std::vector<int32_t> big(200001);
  for (size_t i = 0; i < big.size(); ++i) big[i] = 3 * (int32_t)i;
  for (int32_t v = -2; v < 600010; v += 7) {
    const int want = (int)(std::lower_bound(big.begin(), big.end(), v) - big.begin());
    if (rgcn_lower_bound(big.data(), 0, (int)big.size(), v) != want) {
      std::printf("search mismatch in the long array at %d\n", (int)v);
      return 1;
    }
    ++checked;
  }
  const int32_t edge[] = {INT32_MIN, -1, 0, INT32_MAX - 1, INT32_MAX};
  std::vector<int32_t> ends(edge, edge + 5);
  for (int i = 0; i < 5; ++i)
    if (rgcn_lower_bound(ends.data(), 0, 5, edge[i]) != i) return 1;
  std::printf("paths_order_check ok %ld\n", checked);
  return 0;
}
