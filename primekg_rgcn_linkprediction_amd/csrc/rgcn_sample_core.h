// What the two batch samplers (sampler.hip, sampler_constrained.hip) must agree on to the bit, in one copy: the
// counter-based generator, the lookup of the positive a sample comes from, and the draw of a replacement.  "All groups
// null and one try equals the plain sampler bit for bit" (include/rgcn_sampling.h) rests on both kernels calling these.
#pragma once
#include "rgcn_common.h"

namespace {

__device__ inline void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[1] = (uint32_t)p1; c[3] = (uint32_t)p0; c[0] = n0; c[2] = n2;
}

__device__ inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// Sample i of a batch of B positives and k corruptions of each (i < B: positive i; otherwise corruption (i - B) % k of
// positive p = (i - B) / k): the batch starts at column position `start` = cursor[0] (0 without a cursor), the sample's
// positive is column `colm` = order[start + p] (start + p without an order) and (h, t) are that column's endpoints.
// Position and column are clamped to [0, E): a window past the end never reads outside the columns.
struct rgcn_positive {
  int64_t h, t, colm, start, p;
};
__device__ inline rgcn_positive rgcn_sample_positive(const int64_t* __restrict__ edge_index, int64_t E,
                                                     const int64_t* __restrict__ order,
                                                     const int64_t* __restrict__ cursor, int64_t B, int64_t k, int64_t i) {
  rgcn_positive s;
  s.start = cursor ? cursor[0] : 0;
  s.p = i < B ? i : (i - B) / k;
  int64_t pos = s.start + s.p;
  pos = pos < 0 ? 0 : (pos >= E ? E - 1 : pos);
  s.colm = order ? order[pos] : pos;
  s.colm = s.colm < 0 ? 0 : (s.colm >= E ? E - 1 : s.colm);
  s.h = edge_index[s.colm];
  s.t = edge_index[E + s.colm];
  return s;
}

// the counter of negative i of the batch at `start`: unique per negative of the epoch
__device__ inline uint64_t rgcn_sample_counter(int64_t start, int64_t B, int64_t k, int64_t i) {
  return (uint64_t)start * (uint64_t)k + (uint64_t)(i - B);
}

// a 32-bit word -> uniform on [0, range), range <= 2^32
__device__ inline int64_t rgcn_sample_draw(uint32_t w, int64_t range) {
  return (int64_t)(((uint64_t)w * (uint64_t)range) >> 32);
}

}  // namespace
