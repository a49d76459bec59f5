// The ordered scatter, whole: contribution rows plus int32 keys in, one row per key out, every sum in slot order, so two
// runs give the same bits.  Users: rgcn_decoder_head.h (the backward of the DistMult and ComplEx heads, for distmult.hip
// and complex.hip), distmult.hip (rgcn_segment_sum, the loss reduction), complex.hip (the query launch's lane groups) and
// transe.hip (the TransE step).
//   - rgcn_pick_group / RGCN_DISPATCH_G: the lane group of d/4 lanes per sample of the contribution launches.
//   - rgcn_checked_row: an id outside its table is clamped to row 0 and the library's sticky flag raised.
//   - stage_keys / earlier_slot_has: the prologue of the one-wave-per-slot kernels (k_scatter_rows, k_transe_apply): the
//     keys into LDS, and one step of the ballot scan that retires every occurrence of a key but the first.
//   - MatchIter / ordered_row_sum: the wave-uniform iterator over the slots that carry one key, and the sum of their rows
//     in slot order, eight loads in flight; a policy maps a slot to its row and sign (PlainRows, TranseRows).
//   - k_scatter_rows / rgcn_scatter_rows: the scatter launch of the two heads' backward, decoder-independent.
//   - segment_len / k_segment_partials / k_segment_combine<SUBTRACT>: the fixed two-level tree of a table of few rows.
//   - block1024_sum_tally: the float sum and int tally of the loss reductions (k_bce_reduce, k_transe_loss).
// Everything sits in an anonymous namespace: each translation unit gets its own copies, the kernels included, and no
// symbol crosses objects.
#pragma once
#include "rgcn_common.h"

namespace {

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// lanes per sample: the power of two that covers d/4 float4 columns, at most a wave
inline int rgcn_pick_group(int64_t d) {
  int g = 1;
  while (g < 64 && g * 4 < d) g <<= 1;
  return g;
}

// CALL with `G` a constant expression equal to G_ (a value of rgcn_pick_group)
#define RGCN_DISPATCH_G(G_, CALL)                   \
  switch (G_) {                                     \
    case 1: { constexpr int G = 1; CALL; } break;   \
    case 2: { constexpr int G = 2; CALL; } break;   \
    case 4: { constexpr int G = 4; CALL; } break;   \
    case 8: { constexpr int G = 8; CALL; } break;   \
    case 16: { constexpr int G = 16; CALL; } break; \
    case 32: { constexpr int G = 32; CALL; } break; \
    default: { constexpr int G = 64; CALL; } break; \
  }

// idx[b] (row b itself without an index vector); an id outside its table: clamped to row 0 - nothing is ever dereferenced
// out of bounds - and the library's sticky flag raised (`flag`: distmult.hip's g_index_error, rgcn_index_error_fetch)
__device__ inline int64_t rgcn_checked_row(const int64_t* __restrict__ idx, int64_t b, int64_t rows, int* __restrict__ flag) {
  int64_t v = idx ? idx[b] : b;
  if ((uint64_t)v >= (uint64_t)rows) {
    *flag = 1;
    v = 0;
  }
  return v;
}

// The keys of a one-wave-per-slot kernel, by all THREADS threads of the workgroup: staged in the kernel's own `skeys`
// (IN_LDS; its capacity is the kernel's business) or left where they are.  A template on where the keys are: the scans
// then read LDS with ds_read_b32, not through a flat pointer.
template <bool IN_LDS, int THREADS>
__device__ inline const int32_t* stage_keys(const int32_t* __restrict__ keys, int S, int32_t* skeys) {
  if (IN_LDS) {
    for (int i = threadIdx.x; i < S; i += THREADS) skeys[i] = keys[i];
    __syncthreads();
  }
  return IN_LDS ? skeys : keys;
}

// wave-uniform: one of the 64 slots from c on, and before slot s, carries `my` - an earlier occurrence owns the row.
// One ballot; the kernels walk c = 0, 64, ... < s themselves and return from inside that loop.  (As one function that
// walks all chunks and answers once, the compiler merged the loop's two exits into one and tested the answer again
// behind the loop: a handful of scalar instructions more per step of a scan that bounds both launches.  This form
// compiles to the instructions the kernels had before the prologue was shared; profiles/ordered_scatter_refactor.txt.)
__device__ inline bool earlier_slot_has(const int32_t* k, int my, int s, int c, int lane) {
  const int p = c + lane;
  return __ballot(p < s && k[p] == my) != 0;
}

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

// slot p -> (row of the contribution buffer, sign mask XORed into the row's floats)
struct PlainRows {                               // slot p adds row p
  __device__ static inline int row(int p) { return p; }
  __device__ static inline unsigned flip(int) { return 0u; }
};
// The TransE step's signed rows: slot p belongs to sample p / 4; kinds 0 and 3 (positive head, negative tail) subtract
// their row, kinds 1 and 2 add it; kinds 0, 1 read dpn[2i], kinds 2, 3 read dpn[2i + 1]:
// slot p reads row p >> 1 of dpn (kinds 0, 1 -> 2i, kinds 2, 3 -> 2i + 1).  The sign is a bit flipped for kinds
// 0 and 3, not a select between a row and its negation: written as `neg ? -w : w` inside the `p >= 0` branch,
// the compiler at hand dropped the negation of the first of the eight rows for kind 0 (seen in the ISA)
struct TranseRows {
  __device__ static inline int row(int p) { return p >> 1; }
  __device__ static inline unsigned flip(int p) { return (~((unsigned)p ^ ((unsigned)p >> 1)) & 1u) << 31; }
};

// the (signed) rows of the matches the iterator yields, added in order, eight loads in flight
template <class Rows = PlainRows>
__device__ inline float4 ordered_row_sum(MatchIter& it, const float* __restrict__ rows, int d, int c0, int lane) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  while (true) {
    int p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = it.next(lane);
    if (p[0] < 0) break;
    float4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float4 w = p[u] >= 0 ? ld4(rows + (size_t)Rows::row(p[u]) * d + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
      const unsigned flip = Rows::flip(p[u]);
      v[u] = make_float4(__uint_as_float(__float_as_uint(w.x) ^ flip), __uint_as_float(__float_as_uint(w.y) ^ flip),
                         __uint_as_float(__float_as_uint(w.z) ^ flip), __uint_as_float(__float_as_uint(w.w) ^ flip));
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
    }
    if (p[7] < 0) break;
  }
  return acc;
}

constexpr int kScatterWaves = 16;                // waves (slots) per workgroup: one staging of the keys serves sixteen slots
constexpr int kKeysInLds = 16384;                // key count up to which the keys are staged in LDS

// rows[S, d] (workspace), keys[S] -> out[key] = sum of the rows with that key, in slot order; one wave per slot, sixteen
// slots per workgroup (one staging of the keys serves them all).  A slot that finds an equal key BEFORE itself
// retires; the first occurrence of a row adds the rows of all its occurrences in slot order.  A template on where the
// keys are (stage_keys).
// (Round 3 tried a chunked two-pass form - every 16th occurrence adds its chunk, a second launch adds the chunk sums
// of the rows with more than 16 occurrences - to shorten the chain of a hub with 100+ occurrences: 15 + 18 us against
// this kernel's 27 us.  The launch is bound by the scans over the keys, not by the hub's additions.)
template <bool IN_LDS>
__global__ __launch_bounds__(64 * kScatterWaves) void k_scatter_rows(const int32_t* __restrict__ keys, int S,
                                                                              const float* __restrict__ rows, int d,
                                                                              float* __restrict__ out) {
  __shared__ int32_t skeys[IN_LDS ? kKeysInLds : 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* k = stage_keys<IN_LDS, 64 * kScatterWaves>(keys, S, skeys);
  const int s = blockIdx.x * kScatterWaves + wave;
  if (s >= S) return;
  const int my = k[s];
  for (int c = 0; c < s; c += 64)               // an earlier occurrence owns the row
    if (earlier_slot_has(k, my, s, c, lane)) return;
  for (int c0 = lane * 4; c0 < ((d + 255) & ~255); c0 += 256) {
    MatchIter it;
    it.start(k, my, s, S, lane);
    const int cc = min(c0, d - 4);
    const float4 acc = ordered_row_sum(it, rows, d, cc, lane);
    if (c0 < d) *reinterpret_cast<float4*>(out + (size_t)my * d + c0) = acc;
  }
}

// the scatter launch of a head's backward (rgcn_decoder_head.h): the instance by where the S keys fit
inline void rgcn_scatter_rows(const int32_t* keys, int S, const float* rows, int d, float* out, hipStream_t stream) {
  const unsigned grid = (unsigned)((S + kScatterWaves - 1) / kScatterWaves);
  if (S <= kKeysInLds) k_scatter_rows<true><<<grid, 64 * kScatterWaves, 0, stream>>>(keys, S, rows, d, out);
  else k_scatter_rows<false><<<grid, 64 * kScatterWaves, 0, stream>>>(keys, S, rows, d, out);
}

// samples per segment of the relation-table tree: 64 for the training batch (a wave then adds ~20 rows in order instead
// of ~85 - the launch is one latency chain per wave, 19 us at 256), growing with the batch so that the combine pass
// never walks more than 64 segments
inline int64_t segment_len(int64_t batch) { return std::max<int64_t>(64, (ceil_div64(batch, 64) + 63) / 64 * 64); }

// partial[(seg * R + row), :] = sum of rows[b] over b in segment seg with keys[b] == row, in order
// grid (R, segments), one wave each
__global__ __launch_bounds__(64) void k_segment_partials(const int32_t* __restrict__ keys, int B,
                                                         const float* __restrict__ rows, int d, int R, int seg_len,
                                                         float* __restrict__ partial) {
  const int lane = threadIdx.x, row = blockIdx.x, seg = blockIdx.y;
  const int lo = seg * seg_len, hi = min(B, lo + seg_len);
  for (int c0 = lane * 4; c0 < ((d + 255) & ~255); c0 += 256) {
    MatchIter it;
    it.start(keys, row, lo, hi, lane);
    const int cc = min(c0, d - 4);               // lanes past the row stay for the iterator's ballots
    const float4 acc = ordered_row_sum(it, rows, d, cc, lane);
    if (c0 < d) *reinterpret_cast<float4*>(partial + ((size_t)seg * R + row) * d + c0) = acc;
  }
}

// out[row, :] = sum over segments, in order; SUBTRACT: out[row, :] -= that sum.  One wave per row.
template <bool SUBTRACT>
__global__ __launch_bounds__(64) void k_segment_combine(const float* __restrict__ partial, int nseg, int R, int d,
                                                        float* __restrict__ out) {
  const int lane = threadIdx.x, row = blockIdx.x;
  for (int c0 = lane * 4; c0 < d; c0 += 256) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int s0 = 0; s0 < nseg; s0 += 16) {      // sixteen loads in flight, added in segment order
      float4 v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        v[u] = s0 + u < nseg ? ld4(partial + ((size_t)(s0 + u) * R + row) * d + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
      }
    }
    float* o = out + (size_t)row * d + c0;
    if (SUBTRACT) {
      const float4 w = ld4(o);
      acc = make_float4(w.x - acc.x, w.y - acc.y, w.z - acc.z, w.w - acc.w);
    }
    *reinterpret_cast<float4*>(o) = acc;
  }
}

// By the one 1,024-thread workgroup of a loss reduction: each(b, s, c) adds element b to a float sum and an int tally.
// Fixed order - thread i takes elements i, i + 1024, ..., then a tree halving from 512 - so two runs give the same bits.
// The totals are thread 0's to use.
struct SumTally {
  float sum;
  int tally;
};
template <class Each>
__device__ inline SumTally block1024_sum_tally(int B, Each each) {
  __shared__ float red[1024];
  __shared__ int cnt[1024];
  float s = 0.f;
  int c = 0;
  for (int b = threadIdx.x; b < B; b += 1024) each(b, s, c);
  red[threadIdx.x] = s;
  cnt[threadIdx.x] = c;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[threadIdx.x] += red[threadIdx.x + w];
      cnt[threadIdx.x] += cnt[threadIdx.x + w];
    }
    __syncthreads();
  }
  return {red[0], cnt[0]};
}

}  // namespace
