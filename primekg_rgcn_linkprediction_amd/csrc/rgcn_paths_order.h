// The total order of the path search (include/rgcn_paths.h), shared by the kernels of csrc/paths.hip and the
// stand-alone host check (tests/paths_order_check.cpp, run under AddressSanitizer / UndefinedBehaviorSanitizer).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RGCN_PATHS_FN __host__ __device__ inline
#else
#define RGCN_PATHS_FN inline
#endif

constexpr int RGCN_PATHS_MAX_LEN = 4;    // edges of the longest path
constexpr int RGCN_PATHS_MAX_K = 64;     // one list entry per lane of the inserting wave
constexpr int RGCN_PATHS_NODES = RGCN_PATHS_MAX_LEN + 1;

// A path s -> n1 -> n2 -> n3 -> t of `len` edges: the interior nodes it does not have are -1 (len = 1: all three).
// len = 0 marks an empty slot.  The score of an entry is never NaN.
struct rgcn_path_entry {
  float score;
  int32_t len, n1, n2, n3;
};

// a stands in front of b: score descending (-0.0 and +0.0 are one score), then fewer edges, then the interior nodes
// lexicographically ascending.  Two different paths of one query never compare equal, so any arrival order sorts alike.
RGCN_PATHS_FN bool rgcn_path_before(const rgcn_path_entry& a, const rgcn_path_entry& b) {
  if (a.score != b.score) return a.score > b.score;
  if (a.len != b.len) return a.len < b.len;
  if (a.n1 != b.n1) return a.n1 < b.n1;
  if (a.n2 != b.n2) return a.n2 < b.n2;
  return a.n3 < b.n3;
}

// w[L] = 1 / (L * (1 + 0.2 * (L - 1))) in double, rounded once to float: the mean over L hops times the length
// penalty 1 / (1 + 0.2 * (nodes - 2)) with nodes = L + 1
RGCN_PATHS_FN float rgcn_path_weight(int len) { return (float)(1.0 / (len * (1 + 0.2 * (len - 1)))); }
