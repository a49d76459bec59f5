// Position search in an ascending int64 array, shared by the constrained sampler's kernel and its stand-alone host
// check (tests/sampler_search_check.cpp, run under AddressSanitizer / UndefinedBehaviorSanitizer); the int32 overload
// below is the path enumeration's (csrc/paths.hip, tests/paths_order_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RGCN_SEARCH_FN __host__ __device__ inline
#else
#define RGCN_SEARCH_FN inline
#endif

// First position in the ascending a[lo, hi) whose value is >= v (hi if none): what a binary search returns, found
// RGCN_SEARCH_FAN ways at a time.  A round reads RGCN_SEARCH_FAN - 1 evenly spaced pivots - independent loads, one
// latency - and keeps the one interval that can hold the answer, so 2^17 entries take 6 dependent rounds instead of
// 17 dependent loads (the sampler's launch is bound by such chains); the last
// <= RGCN_SEARCH_FAN entries are read together.  Every index read is inside [lo, hi), whatever the values are.
constexpr int RGCN_SEARCH_FAN = 8;
template <typename T, typename I>
RGCN_SEARCH_FN I rgcn_lower_bound_fan(const T* a, I lo, I hi, T v) {
  while (hi - lo > RGCN_SEARCH_FAN) {
    const I step = (hi - lo) / RGCN_SEARCH_FAN;            // >= 1; the last pivot lo + (FAN - 1) * step < hi
    T pivot[RGCN_SEARCH_FAN - 1];
#pragma unroll
    for (int j = 0; j < RGCN_SEARCH_FAN - 1; ++j) pivot[j] = a[lo + step * (j + 1)];
    int below = 0;                                         // ascending: the pivots < v are the first `below` of them
#pragma unroll
    for (int j = 0; j < RGCN_SEARCH_FAN - 1; ++j) below += pivot[j] < v ? 1 : 0;
    const I base = lo;
    if (below > 0) lo = base + step * below + 1;           // that pivot is < v: the answer is after it
    if (below < RGCN_SEARCH_FAN - 1) hi = base + step * (below + 1);   // the next one is >= v: the answer is at most there
  }
  int below = 0;
  if (hi > lo) {
#pragma unroll
    for (int j = 0; j < RGCN_SEARCH_FAN; ++j) {
      const bool in = lo + j < hi;
      const T x = a[in ? lo + j : hi - 1];
      below += in && x < v ? 1 : 0;
    }
  }
  return lo + below;
}
RGCN_SEARCH_FN int64_t rgcn_lower_bound(const int64_t* a, int64_t lo, int64_t hi, int64_t v) {
  return rgcn_lower_bound_fan<int64_t, int64_t>(a, lo, hi, v);
}
// int32 ids with int positions: the neighbour lists of the path enumeration (csrc/paths.hip), in LDS or global memory
RGCN_SEARCH_FN int rgcn_lower_bound(const int32_t* a, int lo, int hi, int32_t v) {
  return rgcn_lower_bound_fan<int32_t, int>(a, lo, hi, v);
}
