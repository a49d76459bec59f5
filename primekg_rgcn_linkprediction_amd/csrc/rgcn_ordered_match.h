// The ordered scatter's shared pieces (distmult.hip: the DistMult backward and rgcn_segment_sum; transe.hip: the TransE
// step): the wave-uniform iterator over the slots that carry one key, the ordered row sum over what it yields, and the
// segment rule of the two-level relation tree.  Every user adds in slot order, so two runs give the same bits.
#pragma once
#include "rgcn_common.h"

namespace {

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// ordered iteration over the positions p in [lo, hi) with keys[p] == my (keys in LDS or global), wave-uniform
struct MatchIter {
  const int32_t* keys;
  int my, pos, hi;            // pos: next chunk start (multiple of 64)
  unsigned long long mask;    // unvisited matches of the current chunk
  int base;                   // its start
  __device__ inline void start(const int32_t* k, int my_, int lo, int hi_, int lane) {
    keys = k; my = my_; hi = hi_; pos = lo & ~63; mask = 0ull;
    fetch(lane);
    if (lo & 63) mask &= ~((1ull << (lo & 63)) - 1ull);
  }
  __device__ inline void fetch(int lane) {       // load the chunk at pos, advance
    base = pos;
    const int p = pos + lane;
    mask = __ballot(p < hi && keys[p] == my);
    pos += 64;
  }
  __device__ inline int next(int lane) {         // next match or -1
    while (mask == 0ull) {
      if (pos >= hi) return -1;
      fetch(lane);
    }
    const int bit = __ffsll((long long)mask) - 1;
    mask &= mask - 1ull;
    return base + bit;
  }
};

// the rows of the matches the iterator yields, added in order, eight loads in flight
__device__ inline float4 ordered_row_sum(MatchIter& it, const float* __restrict__ rows, int d, int c0, int lane) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  while (true) {
    int p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = it.next(lane);
    if (p[0] < 0) break;
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      v[u] = p[u] >= 0 ? ld4(rows + (size_t)p[u] * d + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
    }
    if (p[7] < 0) break;
  }
  return acc;
}

// samples per segment of the relation-table tree: 64 for the training batch (a wave then adds ~20 rows in order instead
// of ~85 - the launch is one latency chain per wave, 19 us at 256), growing with the batch so that the combine pass
// never walks more than 64 segments
inline int64_t segment_len(int64_t batch) { return std::max<int64_t>(64, (ceil_div64(batch, 64) + 63) / 64 * 64); }

}  // namespace
