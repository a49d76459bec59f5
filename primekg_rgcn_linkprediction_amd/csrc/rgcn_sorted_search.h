// Position search in an ascending int64 array, shared by the constrained sampler's kernel and its stand-alone host
// check (tests/sampler_search_check.cpp, run under AddressSanitizer / UndefinedBehaviorSanitizer).
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
RGCN_SEARCH_FN int64_t rgcn_lower_bound(const int64_t* a, int64_t lo, int64_t hi, int64_t v) {
  while (hi - lo > RGCN_SEARCH_FAN) {
    const int64_t step = (hi - lo) / RGCN_SEARCH_FAN;      // >= 1; the last pivot lo + (FAN - 1) * step < hi
    int64_t pivot[RGCN_SEARCH_FAN - 1];
#pragma unroll
    for (int j = 0; j < RGCN_SEARCH_FAN - 1; ++j) pivot[j] = a[lo + step * (j + 1)];
    int below = 0;                                         // ascending: the pivots < v are the first `below` of them
#pragma unroll
    for (int j = 0; j < RGCN_SEARCH_FAN - 1; ++j) below += pivot[j] < v ? 1 : 0;
    const int64_t base = lo;
    if (below > 0) lo = base + step * below + 1;           // that pivot is < v: the answer is after it
    if (below < RGCN_SEARCH_FAN - 1) hi = base + step * (below + 1);   // the next one is >= v: the answer is at most there
  }
  int below = 0;
  if (hi > lo) {
#pragma unroll
    for (int j = 0; j < RGCN_SEARCH_FAN; ++j) {
      const bool in = lo + j < hi;
      const int64_t x = a[in ? lo + j : hi - 1];
      below += in && x < v ? 1 : 0;
    }
  }
  return lo + below;
}
