// Local-neighbourhood statistics of node pairs (include/rgcn_neighborhood.h): what the reference's failure analysis does
// with networkx sets (analyze_failures.analyze_subgraph, analyze_failures.py:368-437; medical_validation.
// find_common_neighbors, medical_validation.py:356-394) - the radius-r balls around both ends of a pair over
// successors + predecessors, their intersection, and the node, edge and node-type counts of the subgraph induced on
// their union - for every pair of a batch, on the device.
//
//   k_pair_neighborhood  one workgroup (4 waves) per query.  Four bitsets over the nodes live in dynamic LDS, N / 8
//                        bytes each: the two balls, the frontier and the next frontier.  Growth is level-synchronous:
//                          - the lanes take the frontier's words, one word per lane and 256 per step, and pop its set
//                            bits (once for the out-rows, once more for the in-rows); a lane walks the row of its
//                            node and ORs every neighbour's bit into the ball with an LDS atomic (after a plain look:
//                            most neighbours of the second round are in the ball already); the lane whose OR set
//                            the bit sets it in the next frontier too.
//                          - a row of kHubDegree entries or more is NOT walked by its lane: the wave collects such
//                            rows by a ballot and walks each with all 64 lanes, 64 entries at a time (PrimeKG's
//                            degrees reach the thousands; one lane would hold the workgroup up for that long).
//                          - after the round the next frontier's popcount is what the ball grew by; the frontiers swap.
//                        From the finished bitsets: popcounts of AND and OR; the union (written over the idle frontier)
//                        is walked once more the same way, out-rows only, every entry a bit test: the induced edges;
//                        the union's classes are counted with LDS integer atomics; the intersection's smallest ids
//                        come from an ordered compaction, a workgroup prefix sum over 256 words' popcounts per step.
//                        Every sum is an integer sum and every bitset operation an OR: the order in which lanes arrive
//                        changes nothing.  All outputs leave through plain vector stores.
#include <algorithm>

#include "rgcn_common.h"
#include "../../include/rgcn_neighborhood.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kHubDegree = RGCN_NEIGHBORHOOD_HUB_DEGREE;
constexpr int kBitsets = 4;
constexpr int kLdsBytes = 160 * 1024;       // LDS of a CU, and the most one workgroup can have
constexpr int kStaticReserve = 4 * 1024;    // the kernel's static LDS (reduction slots, class counters), with room
constexpr int kMaxWords = (kLdsBytes - kStaticReserve) / (kBitsets * 4);
constexpr int64_t kMaxNodes = (int64_t)kMaxWords * 32;
static_assert(kMaxNodes >= 262144, "twice the full PrimeKG node count must fit (include/rgcn_neighborhood.h)");

// The sum of v over the workgroup, in every thread.  `red` may still be read by the previous call's stragglers: the
// first barrier waits for them.  (It is also the barrier that makes the caller's LDS stores before the call visible.)
__device__ inline unsigned long long block_sum(unsigned long long v, unsigned long long* red, int tid) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

// op(v) for every entry v of row u of (ptr, idx), for every set bit u of bits[0 .. W): short rows by the lane that
// holds the bit, rows of kHubDegree entries or more by the whole wave.  Called by all threads of the workgroup; `bits`
// does not change during the call; op ignores a v outside [0, N) (the padding of a short row's last step is -1).  Row bounds are clamped to [0, nnz]: a damaged ptr array reads nothing outside idx.
template <class Op>
__device__ inline void walk_rows(const unsigned* bits, int W, const int64_t* __restrict__ ptr,
                                 const int32_t* __restrict__ idx, int64_t nnz, int tid, Op op) {
  const int lane = tid & 63;
  for (int base = (tid >> 6) * 64; base < W; base += kThreads) {        // wave-uniform
    const int w = base + lane;
    unsigned m = w < W ? bits[w] : 0u;
    while (__ballot(m != 0u)) {                                         // wave-uniform
      int64_t b = 0, e = 0;
      if (m) {
        const int u = w * 32 + __ffs((int)m) - 1;
        m &= m - 1;
        b = clamp64(ptr[u], 0, nnz);
        e = clamp64(ptr[u + 1], b, nnz);
      }
      const bool hub = e - b >= kHubDegree;
      if (!hub) {
        for (int64_t i = b; i < e; i += 4) {                            // four loads in flight; op(-1) does nothing
          const int v0 = idx[i], v1 = i + 1 < e ? idx[i + 1] : -1, v2 = i + 2 < e ? idx[i + 2] : -1,
                    v3 = i + 3 < e ? idx[i + 3] : -1;
          op(v0);
          op(v1);
          op(v2);
          op(v3);
        }
      }
      unsigned long long hubs = __ballot(hub);
      while (hubs) {
        const int src = __ffsll((long long)hubs) - 1;
        hubs &= hubs - 1;
        const int64_t hb = lane_i64(b, src), he = lane_i64(e, src);
        for (int64_t i = hb + lane; i < he; i += 64) op(idx[i]);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_pair_neighborhood(
    const int64_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst, const int64_t* __restrict__ in_ptr,
    const int32_t* __restrict__ in_src, int N, int64_t nnz, const int64_t* __restrict__ sources,
    const int64_t* __restrict__ targets, int radius, const int32_t* __restrict__ node_class, int num_classes,
    int common_cap, int64_t* __restrict__ ball, int32_t* __restrict__ distance, int64_t* __restrict__ common,
    int64_t* __restrict__ union_nodes, int64_t* __restrict__ union_edges, int64_t* __restrict__ class_count,
    int32_t* __restrict__ common_nodes) {
  extern __shared__ unsigned lds[];
  __shared__ unsigned long long red[kWaves];
  __shared__ int cls[RGCN_NEIGHBORHOOD_MAX_CLASSES];
  __shared__ int wave_total[kWaves];
  const int W = (N + 31) >> 5;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q = blockIdx.x;
  unsigned *F = lds + 2 * W, *Fn = lds + 3 * W;                         // the balls: lds and lds + W

  for (int i = tid; i < kBitsets * W; i += kThreads) lds[i] = 0u;
  if (tid < RGCN_NEIGHBORHOOD_MAX_CLASSES) cls[tid] = 0;
  const int64_t ends[2] = {sources[q], targets[q]};
  const bool t_in_range = (uint64_t)ends[1] < (uint64_t)N;
  const int tw = t_in_range ? (int)(ends[1] >> 5) : 0;
  const unsigned tbit = t_in_range ? 1u << (ends[1] & 31) : 0u;
  int dist = -1;
  __syncthreads();

#pragma unroll 1
  for (int side = 0; side < 2; ++side) {
    unsigned* const A = lds + side * W;
    const int64_t x = ends[side];
    bool present = false;                                               // the same in every thread
    if ((uint64_t)x < (uint64_t)N) present = out_ptr[x + 1] > out_ptr[x] || in_ptr[x + 1] > in_ptr[x];
    if (present && tid == 0) {
      A[x >> 5] = 1u << (x & 31);
      F[x >> 5] = 1u << (x & 31);
    }
    int size = present ? 1 : 0, newly = size;
    if (tid == 0) ball[(q * 2 + side) * 5] = size;
    if (side == 0 && present && x == ends[1]) dist = 0;
    __syncthreads();
#pragma unroll 1
    for (int j = 1; j <= RGCN_NEIGHBORHOOD_MAX_RADIUS; ++j) {
      if (j > radius) {
        if (tid == 0) ball[(q * 2 + side) * 5 + j] = 0;
        continue;
      }
      if (newly > 0) {                                                  // workgroup-uniform
        unsigned* const next = Fn;
        auto grow = [A, next, N](int v) {
          if ((unsigned)v >= (unsigned)N) return;
          const unsigned bit = 1u << (v & 31);
          unsigned* const word = A + (v >> 5);
          if (__atomic_load_n(word, __ATOMIC_RELAXED) & bit) return;   // a stale look only costs the atomic below
          if (!(atomicOr(word, bit) & bit)) atomicOr(next + (v >> 5), bit);
        };
        walk_rows(F, W, out_ptr, out_dst, nnz, tid, grow);
        walk_rows(F, W, in_ptr, in_src, nnz, tid, grow);
        __syncthreads();
        // B_j is complete and nobody adds to it before block_sum's barriers below: the one place the target is looked up
        if (side == 0 && dist < 0 && (A[tw] & tbit)) dist = j;
        unsigned grown = 0;
        for (int i = tid; i < W; i += kThreads) {
          grown += __popc(Fn[i]);
          F[i] = 0u;
        }
        newly = (int)block_sum(grown, red, tid);                        // (its barriers: F is clear before it is written again)
        size += newly;
        unsigned* const swap = F;
        F = Fn;
        Fn = swap;
      }
      if (tid == 0) ball[(q * 2 + side) * 5 + j] = size;
    }
    // F's last readers passed a barrier since (or it holds the seed alone); Fn is clear already
    for (int i = tid; i < W; i += kThreads) F[i] = 0u;
    __syncthreads();
  }

  // the union, written over the frontier, and the two popcounts (each below 2^31: one 64-bit sum carries both)
  const unsigned* const A = lds;
  const unsigned* const B = lds + W;
  unsigned long long both = 0;
  for (int i = tid; i < W; i += kThreads) {
    const unsigned a = A[i], b = B[i];
    F[i] = a | b;
    both += ((unsigned long long)__popc(a | b) << 32) + (unsigned long long)__popc(a & b);
  }
  both = block_sum(both, red, tid);
  const int n_union = (int)(both >> 32), n_common = (int)(both & 0xffffffffull);

  const unsigned* const U = F;
  unsigned long long edges = 0;
  walk_rows(U, W, out_ptr, out_dst, nnz, tid, [U, N, &edges](int v) {
    if ((unsigned)v < (unsigned)N) edges += (U[v >> 5] >> (v & 31)) & 1u;
  });
  edges = block_sum(edges, red, tid);
  if (tid == 0) {
    distance[q] = dist;
    common[q] = n_common;
    union_nodes[q] = n_union;
    union_edges[q] = (int64_t)edges;
  }

  if (class_count) {
    for (int i = tid; i < W; i += kThreads) {
      unsigned m = U[i];
      while (m) {
        const int c = node_class[i * 32 + __ffs((int)m) - 1];
        m &= m - 1;
        if ((unsigned)c < (unsigned)num_classes) atomicAdd(&cls[c], 1);
      }
    }
    __syncthreads();
    if (tid < num_classes) class_count[q * num_classes + tid] = cls[tid];
  }

  if (common_nodes) {
    int32_t* const row = common_nodes + q * common_cap;
    int base = 0;                                                       // workgroup-uniform: ids written so far
    for (int start = 0; start < W && base < common_cap; start += kThreads) {
      const int w = start + tid;
      unsigned m = w < W ? (A[w] & B[w]) : 0u;
      const int mine = __popc(m);
      int incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
      }
      __syncthreads();                                                  // the previous step's totals have been read
      if (lane == 63) wave_total[wave] = incl;
      __syncthreads();
      int pos = base + incl - mine, total = 0;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) {
        if (k < wave) pos += wave_total[k];
        total += wave_total[k];
      }
      while (m && pos < common_cap) {
        row[pos++] = w * 32 + __ffs((int)m) - 1;
        m &= m - 1;
      }
      base += total;
    }
    for (int i = std::min(n_common, common_cap) + tid; i < common_cap; i += kThreads) row[i] = -1;
  }
}

}  // namespace

extern "C" {

int64_t rgcn_neighborhood_max_nodes(void) { return kMaxNodes; }

int rgcn_pair_neighborhood(const int64_t* out_ptr, const int32_t* out_dst, const int64_t* in_ptr, const int32_t* in_src,
                           int64_t num_nodes, int64_t nnz, const int64_t* sources, const int64_t* targets,
                           int64_t num_queries, int radius, const int32_t* node_class, int num_classes, int common_cap,
                           int64_t* ball, int32_t* distance, int64_t* common, int64_t* union_nodes, int64_t* union_edges,
                           int64_t* class_count, int32_t* common_nodes, void* stream_) {
  if (num_queries < 0 || num_nodes <= 0 || nnz < 0) return RGCN_ERR_ARG;
  if (radius < 0 || radius > RGCN_NEIGHBORHOOD_MAX_RADIUS || num_classes < 0 || num_classes > RGCN_NEIGHBORHOOD_MAX_CLASSES ||
      common_cap < 0 || common_cap > RGCN_NEIGHBORHOOD_MAX_COMMON)
    return RGCN_ERR_ARG;
  if (num_queries == 0) return RGCN_OK;
  if (num_nodes > kMaxNodes || num_queries > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  if (!out_ptr || !in_ptr || !sources || !targets || !ball || !distance || !common || !union_nodes || !union_edges)
    return RGCN_ERR_ARG;
  if (nnz > 0 && (!out_dst || !in_src)) return RGCN_ERR_ARG;
  const bool classes = node_class && num_classes > 0;
  if ((classes && !class_count) || (common_cap > 0 && !common_nodes)) return RGCN_ERR_ARG;
  // every operand is an index or count vector walked one element at a time: natural alignment
  RGCN_ALIGN_TRY(8, out_ptr, in_ptr, sources, targets, ball, common, union_nodes, union_edges, class_count);
  RGCN_ALIGN_TRY(4, out_dst, in_src, node_class, distance, common_nodes);
  static bool raised[64] = {};
  const int rc = raise_lds(k_pair_neighborhood, kMaxWords * kBitsets * 4, raised);
  if (rc != RGCN_OK) return rc;
  const int words = (int)((num_nodes + 31) / 32);
  k_pair_neighborhood<<<(unsigned)num_queries, kThreads, (size_t)words * kBitsets * 4, (hipStream_t)stream_>>>(
      out_ptr, out_dst, in_ptr, in_src, (int)num_nodes, nnz, sources, targets, radius, classes ? node_class : nullptr,
      num_classes, common_cap, ball, distance, common, union_nodes, union_edges, classes ? class_count : nullptr,
      common_cap > 0 ? common_nodes : nullptr);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
