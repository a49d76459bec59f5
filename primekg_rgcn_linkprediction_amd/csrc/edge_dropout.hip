// Edge dropout and hidden batch edges (include/rgcn_edge_dropout.h).
//
// The bucketed structure of a graph is built once, by a sort that synchronises and allocates; a training step cannot
// rebuild it, least of all inside a captured HIP graph.  What a step CAN change is the per-edge weight the weighted
// body of k_aggregate already multiplies by.  So a draw is three flat launches over arrays that never move:
//   k_ed_mark     one thread per forward position: kept or not (Philox word of the edge's original column, the batch
//                 window), the mark left in w_fwd as 1 / 0, and the kept count of every (destination, relation) segment.
//                 The bucketed order puts a segment in consecutive positions, so a workgroup reduces its runs of equal
//                 segments (wave ballots, then LDS) and issues ONE integer atomic per segment it touches - a hub of
//                 300,000 edges receives 300 adds, not 300,000 (the note above RGCN_AMAX_SLOTS in rgcn_common.h).
//   k_ed_weights  w = kept ? 1 / k[destination, relation] : 0 for every position of both directions (the transposed
//                 half recomputes the mark from the same word: no E-sized mask travels between the directions).
//   k_ed_heads    the copies of the first RGCN_HEAD weights that ride with every level-0 item, both directions.
// The counts are added into counters that are zero between two draws: k_ed_weights copies them out (what
// rgcn_edge_dropout_kept shows) and k_ed_heads, the last launch, clears them - no memset node in a captured step.
// Integer sums are order-free, so two draws with the same (seed, epoch, cursor) leave the same bits.
//
// Twins (RGCN_EDGE_DROPOUT_HIDE_TWINS / RGCN_EDGE_DROPOUT_PAIRED).  Data that stores (h, r, t) and (t, r, h) as two
// columns leaks half of a hidden edge back and drops half of a dropped pair.  create pairs the columns once, on the
// device: two stable radix sorts (direction and the canonical (min, max) node pair, then the relation) put the copies
// of a triple and of its reverse next to each other, forward copies first, each side in column order; k_tw_pair gives
// the j-th forward copy the j-th backward one.  A draw with an option reads twin[e] (and position[twin[e]]) on top of
// what the plain draw reads; the plain draw is the instantiation without either and reads what it always did.
//
// The mask draw (RGCN_EDGE_DROPOUT_MASK).  Nothing is drawn: every edge carries a float of the caller's and a segment's
// weights are m / M with M the segment's sum in the FIXED order the header states - no counter, no atomic on a float.
// A segment has one owner, so the launches of the plain draw are not used (and not touched):
//   k_ed_mask_fwd  a workgroup looks at 256 forward segments.  A thread sums its own if it has at most 64 edges - a
//                  round of eight positions IS the eight strided partial sums, the ids, positions and mask values of a
//                  round loaded in three batches - leaves m in w_fwd, and divides its own stores.  The longer ones are
//                  then taken one at a time by all 256 threads (the strided partial sums, the butterfly, three adds),
//                  as k_edge_long of edge_grad.hip takes them.  M[s] and k[s] are written by the owner.
//   k_ed_mask_t    one thread per transposed position: m of its column again, divided by M of its forward segment.
//   k_ed_heads     as in the plain draw (the counters it clears were never raised).
//
// The attention draw (RGCN_EDGE_DROPOUT_ATTENTION).  The mask draw's frame with the value computed instead of loaded:
// the logit of an edge is a select over one add of two per-(node, relation) scalars, and a segment's weights are its
// softmax.  Its own kernels again - the mask draw's launches are not touched:
//   k_ed_att_fwd   the owners of k_ed_mask_fwd.  A first walk leaves the logit in w_fwd (-inf for a hidden column: it
//                  then drops out of the maximum, and exp gives the 0 the header asks for) and finds the maximum - an
//                  order-free operation; the second walk is the mask draw's: m = exp(l - mx) summed in the FIXED order,
//                  then the owner's own stores divided.  mx[s], M[s] and k[s] are written by the owner.
//   k_ed_att_t     one thread per transposed position: its transposed segment (source, relation) by a search in rowptr
//                  - that index IS the index of a_src - the logit again, exp(l - mx) / M of its forward segment.
//   k_ed_heads     as ever.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "rgcn_common.h"
#include "rgcn_sample_core.h"
#include "../../include/rgcn_edge_dropout.h"
#include "../../include/rgcn_resample.h"

static_assert(RGCN_EDGE_DROPOUT_STREAM != RGCN_RESAMPLE_STREAM, "every generator of the library has its own stream word");

struct rgcn_edge_dropout {
  const rgcn_graph* parent = nullptr;
  rgcn_graph view;              // shares everything but val / head_w with the parent
  float* val[2] = {nullptr, nullptr};
  float* head_w[2] = {nullptr, nullptr};
  int32_t* kept = nullptr;      // [N * R] k of the last draw
  int32_t* count = nullptr;     // [N * R] the counters a draw adds into: all zero between two draws (k_ed_heads clears them)
  int32_t* seg_f = nullptr;     // [E] forward segment of every forward position
  int32_t* seg_t = nullptr;     // [E] forward segment (dst * R + rel) of every transposed position
  int32_t* twin = nullptr;      // [E] by ORIGINAL column: the column holding the reversed triple, -1 without one
  float* msum = nullptr;        // [N * R] M of the last mask draw (the transposed half of that draw divides by it)
  float* mmax = nullptr;        // [N * R] mx of the last attention draw (its transposed half subtracts it)
};

namespace {

constexpr int kMarkThreads = 1024, kMarkWaves = kMarkThreads / 64, kThreads = 256;

inline unsigned grid_for(int64_t n, int threads) { return (unsigned)std::max<int64_t>(1, ceil_div64(n, threads)); }

struct draw_params {
  const int64_t* position;
  const int64_t* cursor;
  const int64_t* rng;
  int64_t batch;                // the window's length: the option bits are template arguments by now
  uint32_t threshold;
  const int32_t* twin;          // read by the instantiations with an option only
};

// (c0, key, epoch) of a draw, read once per thread
struct draw_state {
  int64_t c0;
  uint32_t k0, k1, epoch;
};
__device__ inline draw_state draw_begin(const draw_params& p) {
  draw_state s;
  s.c0 = p.cursor ? p.cursor[0] : 0;
  const uint64_t seed = (uint64_t)p.rng[0];
  s.k0 = (uint32_t)seed;
  s.k1 = (uint32_t)(seed >> 32);
  s.epoch = (uint32_t)(uint64_t)p.rng[1];
  return s;
}
// the mask draw's: rng holds no seed there, only the cursor is read
__device__ inline draw_state draw_begin_cursor(const draw_params& p) {
  draw_state s;
  s.c0 = p.cursor ? p.cursor[0] : 0;
  s.k0 = s.k1 = s.epoch = 0u;
  return s;
}
// twin[e] where an option looks at it (-1: none); the plain draw has no such load
template <bool kHideTwins, bool kPaired>
__device__ inline int64_t edge_twin(const draw_params& p, int64_t e) {
  if constexpr (kHideTwins || kPaired) return p.twin[e];
  return -1;
}
template <bool kHideTwins>
__device__ inline bool edge_hidden(const draw_params& p, const draw_state& s, int64_t e, int64_t t) {
  if (!p.position) return false;
  const int64_t at = p.position[e];
  bool hidden = at >= s.c0 && at < s.c0 + p.batch;
  if constexpr (kHideTwins) {                    // the index clamped and the result selected: no branch around the load
    const int64_t at_t = p.position[t < 0 ? 0 : t];
    hidden |= (t >= 0) & (at_t >= s.c0) & (at_t < s.c0 + p.batch);
  }
  return hidden;
}
template <bool kPaired>
__device__ inline bool edge_dropped(const draw_params& p, const draw_state& s, int64_t e, int64_t t) {
  if constexpr (kPaired) e = t >= 0 && t < e ? t : e;   // a pair shares the word of its lower column
  uint32_t c[4] = {(uint32_t)(uint64_t)e, (uint32_t)(uint64_t)s.c0, s.epoch, RGCN_EDGE_DROPOUT_STREAM};
  philox4x32_10(c, s.k0, s.k1);
  return c[0] < p.threshold;
}

// seg[pos] = the segment whose [rowptr[s], rowptr[s + 1]) holds pos: the last s with rowptr[s] <= pos.  With `col`
// (the transposed structure) the FORWARD segment of that edge instead: col[pos] * R + s % R.
__global__ void k_ed_segments(const int32_t* __restrict__ rowptr, int64_t NR, int64_t E, int64_t R,
                              const int32_t* __restrict__ col, int32_t* __restrict__ seg) {
  const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= E) return;
  int64_t lo = 0, hi = NR;                       // rowptr[lo] <= pos < rowptr[hi] throughout
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)rowptr[mid] <= pos) lo = mid; else hi = mid;
  }
  seg[pos] = col ? (int32_t)((int64_t)col[pos] * R + lo % R) : (int32_t)lo;
}

template <bool kHideTwins, bool kPaired>
__global__ __launch_bounds__(kMarkThreads) void k_ed_mark(const int64_t* __restrict__ perm,
                                                          const int32_t* __restrict__ seg_f, int64_t E, draw_params p,
                                                          float* __restrict__ w_fwd, int32_t* __restrict__ kept,
                                                          unsigned long long* __restrict__ stats) {
  __shared__ int32_t s_seg[kMarkThreads], s_cnt[kMarkThreads], s_rseg[kMarkThreads];
  __shared__ int32_t s_heads[kMarkWaves], s_stat[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t pos = (int64_t)blockIdx.x * kMarkThreads + tid;
  const bool valid = pos < E;
  const draw_state st = draw_begin(p);
  bool keep = false, hide = false;
  int32_t seg = -1;                              // the positions past the end form one run that counts nothing
  if (valid) {
    const int64_t e = perm[pos];
    seg = seg_f[pos];
    const int64_t t = edge_twin<kHideTwins, kPaired>(p, e);
    hide = edge_hidden<kHideTwins>(p, st, e, t);
    keep = !hide && !edge_dropped<kPaired>(p, st, e, t);
    w_fwd[pos] = keep ? 1.f : 0.f;               // the mark; k_ed_weights turns it into the weight
  }
  s_seg[tid] = seg;
  s_cnt[tid] = 0;
  if (tid < 2) s_stat[tid] = 0;
  __syncthreads();
  const bool head = tid == 0 || s_seg[tid - 1] != seg;
  const unsigned long long heads = __ballot(head), keeps = __ballot(keep), hides = __ballot(hide);
  if (lane == 0) s_heads[wave] = __popcll(heads);
  __syncthreads();
  int run = -1, runs = 0;                        // index of this thread's run inside the workgroup
  for (int w = 0; w < kMarkWaves; ++w) {
    if (w == wave) run += runs;
    runs += s_heads[w];
  }
  const unsigned long long upto = lane == 63 ? ~0ull : ((1ull << (lane + 1)) - 1);
  run += __popcll(heads & upto);
  if (head || lane == 0) {                       // first lane of a run's stretch inside this wave
    const unsigned long long above = heads & ~upto;
    const int next = above ? __ffsll((long long)above) - 1 : 64;
    const unsigned long long stretch = (next == 64 ? ~0ull : ((1ull << next) - 1)) & ~(upto >> 1);
    const int n = __popcll(keeps & stretch);
    if (n) atomicAdd(&s_cnt[run], n);
    if (head) s_rseg[run] = seg;
  }
  if (lane == 0) {
    const int nk = __popcll(keeps), nh = __popcll(hides);
    if (nk) atomicAdd(&s_stat[0], nk);
    if (nh) atomicAdd(&s_stat[1], nh);
  }
  __syncthreads();
  if (tid < runs && s_cnt[tid] > 0) atomicAdd(&kept[s_rseg[tid]], s_cnt[tid]);   // a run with a kept edge is no padding
  if (stats && tid < 2 && s_stat[tid] > 0) atomicAdd(&stats[tid], (unsigned long long)s_stat[tid]);
}

template <bool kHideTwins, bool kPaired>
__global__ __launch_bounds__(kThreads) void k_ed_weights(const int64_t* __restrict__ perm_t,
                                                         const int32_t* __restrict__ seg_f,
                                                         const int32_t* __restrict__ seg_t, int64_t E, draw_params p,
                                                         const int32_t* __restrict__ kept, float* __restrict__ w_fwd,
                                                         float* __restrict__ w_t, int64_t NR, int32_t* __restrict__ kept_out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < NR) kept_out[i] = kept[i];             // what rgcn_edge_dropout_kept shows until the next draw
  if (i < E) {
    const bool keep = w_fwd[i] != 0.f;
    w_fwd[i] = keep ? 1.0f / (float)kept[seg_f[i]] : 0.f;
  } else if (i < 2 * E) {
    const int64_t pos = i - E, e = perm_t[pos];
    const draw_state st = draw_begin(p);
    const int64_t t = edge_twin<kHideTwins, kPaired>(p, e);
    const bool keep = !edge_hidden<kHideTwins>(p, st, e, t) && !edge_dropped<kPaired>(p, st, e, t);
    w_t[pos] = keep ? 1.0f / (float)kept[seg_t[pos]] : 0.f;   // a kept edge is counted in its own segment: k >= 1
  }
}

// head_w of both directions, as k_item_heads (rgcn_graph.hip) fills it
__global__ __launch_bounds__(kThreads) void k_ed_heads(const rgcn_item* __restrict__ items0, int64_t n0,
                                                       const float* __restrict__ w0, float* __restrict__ head0,
                                                       const rgcn_item* __restrict__ items1, int64_t n1,
                                                       const float* __restrict__ w1, float* __restrict__ head1,
                                                       int64_t NR, int32_t* __restrict__ count) {
  int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < NR) count[i] = 0;                      // every reader of this draw's counters has finished: ready for the next
  const rgcn_item* items = items0;
  const float* w = w0;
  float* head = head0;
  if (i >= n0 * RGCN_HEAD) {
    i -= n0 * RGCN_HEAD;
    if (i >= n1 * RGCN_HEAD) return;
    items = items1; w = w1; head = head1;
  }
  const rgcn_item it = items[i / RGCN_HEAD];
  const int e = it.begin + (int)(i % RGCN_HEAD);
  head[i] = e < it.end ? w[e] : 0.f;
}

// ----------------------------------------------------------------------------------------------------------- mask draw
// m(e) of the header: the mask value of a column that is not hidden (a select: a hidden NaN is 0)
template <bool kHideTwins>
__device__ inline bool mask_hidden(const draw_params& p, const draw_state& s, int64_t e) {
  int64_t t = -1;
  if constexpr (kHideTwins) t = p.twin[e];
  return edge_hidden<kHideTwins>(p, s, e, t);
}
__device__ inline float mask_weight(float m, float M) { return M > 0.f ? __fdiv_rn(m, M) : 0.f; }   // NaN > 0 is false

template <bool kHideTwins>
__global__ __launch_bounds__(kThreads) void k_ed_mask_fwd(const int32_t* __restrict__ rowptr,
                                                          const int64_t* __restrict__ perm, int64_t NR, int64_t E,
                                                          draw_params p, const float* __restrict__ mask, float* w_fwd,
                                                          float* __restrict__ msum, int32_t* __restrict__ kept,
                                                          unsigned long long* __restrict__ stats) {
  constexpr int kBatch = 8;
  __shared__ int list[kThreads];
  __shared__ int nlist, s_stat[2], s_kept[kThreads / 64];
  __shared__ float wsum[kThreads / 64];
  const int tid = (int)threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kThreads, s_own = base + tid;
  const draw_state st = draw_begin_cursor(p);
  if (tid == 0) nlist = 0;
  if (tid < 2) s_stat[tid] = 0;
  __syncthreads();
  int64_t begin = 0, end = 0;
  if (s_own < NR) { begin = rowptr[s_own]; end = rowptr[s_own + 1]; }
  const bool is_long = end - begin > RGCN_CHUNK;
  if (is_long) list[atomicAdd(&nlist, 1)] = tid;
  int nk = 0, nh = 0;                              // edges with m > 0, hidden edges: this thread's
  if (!is_long) {                                  // (a segment without an edge: M = 0, k = 0)
    float part[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) part[j] = 0.f;
    const int64_t last = end > begin ? end - 1 : 0;
    for (int64_t q = begin; q < end; q += kBatch) {
      int64_t e[kBatch];
      float m[kBatch];
      bool hid[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) e[j] = clamp64(perm[min(q + j, last)], 0, E - 1);   // clamped: never under a branch
#pragma unroll
      for (int j = 0; j < kBatch; ++j) hid[j] = mask_hidden<kHideTwins>(p, st, e[j]);
#pragma unroll
      for (int j = 0; j < kBatch; ++j) m[j] = mask[e[j]];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const bool in = q + j < end;
        const float v = hid[j] ? 0.f : m[j];
        part[j] += in ? v : 0.f;
        nk += in && v > 0.f;
        nh += in && hid[j];
        if (in) w_fwd[q + j] = v;
      }
    }
    const float M = ((part[0] + part[4]) + (part[2] + part[6])) + ((part[1] + part[5]) + (part[3] + part[7]));
    if (s_own < NR) { msum[s_own] = M; kept[s_own] = nk; }
    for (int64_t q = begin; q < end; q += kBatch) {         // this thread's own stores
      float m[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) m[j] = w_fwd[min(q + j, last)];
#pragma unroll
      for (int j = 0; j < kBatch; ++j)
        if (q + j < end) w_fwd[q + j] = mask_weight(m[j], M);
    }
  }
  __syncthreads();
  const int n = nlist;
  for (int i = 0; i < n; ++i) {
    const int64_t s = base + list[i];
    const int64_t b = rowptr[s], en = rowptr[s + 1];
    float sum = 0.f;
    int cnt = 0;
    for (int64_t q = b + tid; q < en; q += (int64_t)kBatch * kThreads) {   // ascending j: thread t adds b + t + 256 j
      int64_t e[kBatch];
      float m[kBatch];
      bool hid[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) e[j] = clamp64(perm[min(q + (int64_t)j * kThreads, en - 1)], 0, E - 1);
#pragma unroll
      for (int j = 0; j < kBatch; ++j) hid[j] = mask_hidden<kHideTwins>(p, st, e[j]);
#pragma unroll
      for (int j = 0; j < kBatch; ++j) m[j] = mask[e[j]];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        const int64_t at = q + (int64_t)j * kThreads;
        const bool in = at < en;
        const float v = hid[j] ? 0.f : m[j];
        sum += in ? v : 0.f;
        cnt += in && v > 0.f;
        nh += in && hid[j];
        if (in) w_fwd[at] = v;
      }
    }
    nk += cnt;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      sum += __shfl_xor(sum, off);
      cnt += __shfl_xor(cnt, off);
    }
    if ((tid & 63) == 0) { wsum[tid >> 6] = sum; s_kept[tid >> 6] = cnt; }
    __syncthreads();
    const float M = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    if (tid == 0) { msum[s] = M; kept[s] = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3]; }
    for (int64_t q = b + tid; q < en; q += (int64_t)kBatch * kThreads) {
      float m[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) m[j] = w_fwd[min(q + (int64_t)j * kThreads, en - 1)];
#pragma unroll
      for (int j = 0; j < kBatch; ++j)
        if (q + (int64_t)j * kThreads < en) w_fwd[q + (int64_t)j * kThreads] = mask_weight(m[j], M);
    }
    __syncthreads();                               // wsum and s_kept are free again
  }
  if (stats) {                                     // integers: order-free
    if (nk) atomicAdd(&s_stat[0], nk);
    if (nh) atomicAdd(&s_stat[1], nh);
    __syncthreads();
    if (tid < 2 && s_stat[tid] > 0) atomicAdd(&stats[tid], (unsigned long long)s_stat[tid]);
  }
}

template <bool kHideTwins>
__global__ __launch_bounds__(kThreads) void k_ed_mask_t(const int64_t* __restrict__ perm_t,
                                                        const int32_t* __restrict__ seg_t, int64_t E, draw_params p,
                                                        const float* __restrict__ mask, const float* __restrict__ msum,
                                                        float* __restrict__ w_t) {
  const int64_t pos = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (pos >= E) return;
  const draw_state st = draw_begin_cursor(p);
  const int64_t e = clamp64(perm_t[pos], 0, E - 1);
  const float M = msum[seg_t[pos]], m = mask[e];
  const bool hid = mask_hidden<kHideTwins>(p, st, e);
  w_t[pos] = mask_weight(hid ? 0.f : m, M);
}

template <bool kHideTwins>
void launch_mask(rgcn_edge_dropout* ed, const draw_params& p, const float* mask, int64_t* stats, hipStream_t stream) {
  const rgcn_graph& v = ed->view;
  const int64_t E = v.E, NR = v.N * v.R;
  k_ed_mask_fwd<kHideTwins><<<grid_for(NR, kThreads), kThreads, 0, stream>>>(
      v.dir[0].rowptr, v.dir[0].perm, NR, E, p, mask, ed->val[0], ed->msum, ed->kept,
      reinterpret_cast<unsigned long long*>(stats));
  k_ed_mask_t<kHideTwins><<<grid_for(E, kThreads), kThreads, 0, stream>>>(v.dir[1].perm, ed->seg_t, E, p, mask, ed->msum,
                                                                          ed->val[1]);
}

int mask_impl(rgcn_edge_dropout* ed, const draw_params& p, const float* mask, bool hide_twins, int64_t* stats,
              hipStream_t stream) {
  const rgcn_graph& v = ed->view;
  const int64_t NR = v.N * v.R;
  if (v.E <= 0) return RGCN_OK;
  if (hide_twins && p.position) launch_mask<true>(ed, p, mask, stats, stream);
  else launch_mask<false>(ed, p, mask, stats, stream);
  const int64_t n0 = v.dir[0].num_items[0], n1 = v.dir[1].num_items[0];
  k_ed_heads<<<grid_for(std::max((n0 + n1) * RGCN_HEAD, NR), kThreads), kThreads, 0, stream>>>(
      v.dir[0].items[0], n0, ed->val[0], ed->head_w[0], v.dir[1].items[0], n1, ed->val[1], ed->head_w[1], NR, ed->count);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

// ------------------------------------------------------------------------------------------------------ attention draw
// l(e) of the header: one fp32 add, then a select (the product rounded by itself).  `s` = i * R + r is the index of
// a_dst, `js` = j * R + r the index of a_src behind the N * R scalars of a_dst.
__device__ inline float att_logit(const float* __restrict__ a, int64_t NR, int64_t s, int64_t js, float slope) {
  const float z = __fadd_rn(a[s], a[NR + js]);
  return z >= 0.f ? z : __fmul_rn(slope, z);     // NaN >= 0 is false: slope * NaN is NaN
}
__device__ inline float att_value(float l, float mx) { return expf(__fsub_rn(l, mx)); }   // hidden: l = -inf
__device__ inline float att_weight(float m, float M, int k) { return k > 0 ? __fdiv_rn(m, M) : 0.f; }

template <bool kHideTwins>
__global__ __launch_bounds__(kThreads) void k_ed_att_fwd(const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col,
                                                         const int64_t* __restrict__ perm, int64_t NR, int64_t E, int64_t R,
                                                         draw_params p, const float* __restrict__ a, float slope,
                                                         float* w_fwd, float* __restrict__ mmax, float* __restrict__ msum,
                                                         int32_t* __restrict__ kept, unsigned long long* __restrict__ stats) {
  constexpr int kBatch = 8;
  constexpr float kNegInf = -__builtin_inff();
  __shared__ int list[kThreads];
  __shared__ int nlist, s_stat[2], s_kept[kThreads / 64];
  __shared__ float wsum[kThreads / 64], wmax[kThreads / 64];
  const int tid = (int)threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kThreads, s_own = base + tid;
  const draw_state st = draw_begin_cursor(p);
  if (tid == 0) nlist = 0;
  if (tid < 2) s_stat[tid] = 0;
  __syncthreads();
  int64_t begin = 0, end = 0;
  if (s_own < NR) { begin = rowptr[s_own]; end = rowptr[s_own + 1]; }
  const bool is_long = end - begin > RGCN_CHUNK;
  if (is_long) list[atomicAdd(&nlist, 1)] = tid;
  int nk = 0, nh = 0;                              // non-hidden edges, hidden edges: this thread's
  if (!is_long) {                                  // (a segment without an edge: mx = -inf, M = 0, k = 0)
    const int64_t last = end > begin ? end - 1 : 0, r_own = s_own % R;
    float mx = kNegInf;
    for (int64_t q = begin; q < end; q += kBatch) {
      int64_t e[kBatch];
      int j[kBatch];
      float l[kBatch];
      bool hid[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) e[u] = clamp64(perm[min(q + u, last)], 0, E - 1);   // clamped: never under a branch
#pragma unroll
      for (int u = 0; u < kBatch; ++u) j[u] = col[min(q + u, last)];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) hid[u] = mask_hidden<kHideTwins>(p, st, e[u]);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) l[u] = att_logit(a, NR, s_own, clamp64((int64_t)j[u] * R + r_own, 0, NR - 1), slope);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const bool in = q + u < end;
        const float v = hid[u] ? kNegInf : l[u];   // a select: a hidden column's scalars change nothing
        mx = in ? fmaxf(mx, v) : mx;               // (fmaxf passes a NaN over: it comes back through exp)
        nk += in && !hid[u];
        nh += in && hid[u];
        if (in) w_fwd[q + u] = v;
      }
    }
    float part[kBatch];
#pragma unroll
    for (int u = 0; u < kBatch; ++u) part[u] = 0.f;
    for (int64_t q = begin; q < end; q += kBatch) {         // this thread's own stores, as the mask draw sums them
      float l[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) l[u] = w_fwd[min(q + u, last)];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const float m = att_value(l[u], mx);
        part[u] += q + u < end ? m : 0.f;
        if (q + u < end) w_fwd[q + u] = m;
      }
    }
    const float M = ((part[0] + part[4]) + (part[2] + part[6])) + ((part[1] + part[5]) + (part[3] + part[7]));
    if (s_own < NR) { mmax[s_own] = mx; msum[s_own] = M; kept[s_own] = nk; }
    for (int64_t q = begin; q < end; q += kBatch) {
      float m[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) m[u] = w_fwd[min(q + u, last)];
#pragma unroll
      for (int u = 0; u < kBatch; ++u)
        if (q + u < end) w_fwd[q + u] = att_weight(m[u], M, nk);
    }
  }
  __syncthreads();
  const int n = nlist;
  for (int i = 0; i < n; ++i) {
    const int64_t s = base + list[i], r_s = s % R;
    const int64_t b = rowptr[s], en = rowptr[s + 1];
    float mx = kNegInf;
    int cnt = 0;
    for (int64_t q = b + tid; q < en; q += (int64_t)kBatch * kThreads) {
      int64_t e[kBatch];
      int j[kBatch];
      float l[kBatch];
      bool hid[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) e[u] = clamp64(perm[min(q + (int64_t)u * kThreads, en - 1)], 0, E - 1);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) j[u] = col[min(q + (int64_t)u * kThreads, en - 1)];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) hid[u] = mask_hidden<kHideTwins>(p, st, e[u]);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) l[u] = att_logit(a, NR, s, clamp64((int64_t)j[u] * R + r_s, 0, NR - 1), slope);
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int64_t at = q + (int64_t)u * kThreads;
        const bool in = at < en;
        const float v = hid[u] ? kNegInf : l[u];
        mx = in ? fmaxf(mx, v) : mx;
        cnt += in && !hid[u];
        nh += in && hid[u];
        if (in) w_fwd[at] = v;
      }
    }
    nk += cnt;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      mx = fmaxf(mx, __shfl_xor(mx, off));
      cnt += __shfl_xor(cnt, off);
    }
    if ((tid & 63) == 0) { wmax[tid >> 6] = mx; s_kept[tid >> 6] = cnt; }
    __syncthreads();
    mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    const int k = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
    float sum = 0.f;
    for (int64_t q = b + tid; q < en; q += (int64_t)kBatch * kThreads) {   // ascending j: thread t adds b + t + 256 j
      float l[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) l[u] = w_fwd[min(q + (int64_t)u * kThreads, en - 1)];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        const int64_t at = q + (int64_t)u * kThreads;
        const float m = att_value(l[u], mx);
        sum += at < en ? m : 0.f;
        if (at < en) w_fwd[at] = m;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;
    __syncthreads();
    const float M = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    if (tid == 0) { mmax[s] = mx; msum[s] = M; kept[s] = k; }
    for (int64_t q = b + tid; q < en; q += (int64_t)kBatch * kThreads) {
      float m[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) m[u] = w_fwd[min(q + (int64_t)u * kThreads, en - 1)];
#pragma unroll
      for (int u = 0; u < kBatch; ++u)
        if (q + (int64_t)u * kThreads < en) w_fwd[q + (int64_t)u * kThreads] = att_weight(m[u], M, k);
    }
    __syncthreads();                               // wmax, wsum and s_kept are free again
  }
  if (stats) {                                     // integers: order-free
    if (nk) atomicAdd(&s_stat[0], nk);
    if (nh) atomicAdd(&s_stat[1], nh);
    __syncthreads();
    if (tid < 2 && s_stat[tid] > 0) atomicAdd(&stats[tid], (unsigned long long)s_stat[tid]);
  }
}

template <bool kHideTwins>
__global__ __launch_bounds__(kThreads) void k_ed_att_t(const int32_t* __restrict__ rowptr_t,
                                                       const int64_t* __restrict__ perm_t,
                                                       const int32_t* __restrict__ seg_t, int64_t NR, int64_t E,
                                                       draw_params p, const float* __restrict__ a, float slope,
                                                       const float* __restrict__ mmax, const float* __restrict__ msum,
                                                       const int32_t* __restrict__ kept, float* __restrict__ w_t) {
  const int64_t pos = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (pos >= E) return;
  const draw_state st = draw_begin_cursor(p);
  const int64_t e = clamp64(perm_t[pos], 0, E - 1);
  const int64_t s = clamp64(seg_t[pos], 0, NR - 1);
  int64_t lo = 0, hi = NR;                         // rowptr_t[lo] <= pos < rowptr_t[hi]: lo = source * R + relation
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)rowptr_t[mid] <= pos) lo = mid; else hi = mid;
  }
  const float mx = mmax[s], M = msum[s], l = att_logit(a, NR, s, lo, slope);
  const int k = kept[s];
  const bool hid = mask_hidden<kHideTwins>(p, st, e);
  w_t[pos] = att_weight(att_value(hid ? -__builtin_inff() : l, mx), M, k);
}

template <bool kHideTwins>
void launch_att(rgcn_edge_dropout* ed, const draw_params& p, const float* a, float slope, int64_t* stats,
                hipStream_t stream) {
  const rgcn_graph& v = ed->view;
  const int64_t E = v.E, NR = v.N * v.R;
  k_ed_att_fwd<kHideTwins><<<grid_for(NR, kThreads), kThreads, 0, stream>>>(
      v.dir[0].rowptr, v.dir[0].col, v.dir[0].perm, NR, E, v.R, p, a, slope, ed->val[0], ed->mmax, ed->msum, ed->kept,
      reinterpret_cast<unsigned long long*>(stats));
  k_ed_att_t<kHideTwins><<<grid_for(E, kThreads), kThreads, 0, stream>>>(v.dir[1].rowptr, v.dir[1].perm, ed->seg_t, NR, E,
                                                                         p, a, slope, ed->mmax, ed->msum, ed->kept,
                                                                         ed->val[1]);
}

int att_impl(rgcn_edge_dropout* ed, const draw_params& p, const float* a, float slope, bool hide_twins, int64_t* stats,
             hipStream_t stream) {
  const rgcn_graph& v = ed->view;
  const int64_t NR = v.N * v.R;
  if (v.E <= 0) return RGCN_OK;
  if (hide_twins && p.position) launch_att<true>(ed, p, a, slope, stats, stream);
  else launch_att<false>(ed, p, a, slope, stats, stream);
  const int64_t n0 = v.dir[0].num_items[0], n1 = v.dir[1].num_items[0];
  k_ed_heads<<<grid_for(std::max((n0 + n1) * RGCN_HEAD, NR), kThreads), kThreads, 0, stream>>>(
      v.dir[0].items[0], n0, ed->val[0], ed->head_w[0], v.dir[1].items[0], n1, ed->val[1], ed->head_w[1], NR, ed->count);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

// the two launches that form the mark, instantiated on the options
template <bool kHideTwins, bool kPaired>
void launch_mark(rgcn_edge_dropout* ed, const draw_params& p, int64_t* stats, hipStream_t stream) {
  const rgcn_graph& v = ed->view;
  const int64_t E = v.E, NR = v.N * v.R;
  k_ed_mark<kHideTwins, kPaired><<<grid_for(E, kMarkThreads), kMarkThreads, 0, stream>>>(
      v.dir[0].perm, ed->seg_f, E, p, ed->val[0], ed->count, reinterpret_cast<unsigned long long*>(stats));
  k_ed_weights<kHideTwins, kPaired><<<grid_for(std::max(2 * E, NR), kThreads), kThreads, 0, stream>>>(
      v.dir[1].perm, ed->seg_f, ed->seg_t, E, p, ed->count, ed->val[0], ed->val[1], NR, ed->kept);
}

int draw_impl(rgcn_edge_dropout* ed, const draw_params& p, bool hide_twins, bool paired, int64_t* stats, hipStream_t stream) {
  const rgcn_graph& v = ed->view;
  const int64_t E = v.E, NR = v.N * v.R;
  if (E <= 0) return RGCN_OK;                    // no edge: kept holds the zeros rgcn_edge_dropout_create left
  hide_twins = hide_twins && p.position;         // (without a position nothing is hidden, a twin's column neither)
  // kernels only, no memset node: the counters are zero on entry (create, then every draw's last launch clears them)
  if (hide_twins && paired) launch_mark<true, true>(ed, p, stats, stream);
  else if (hide_twins) launch_mark<true, false>(ed, p, stats, stream);
  else if (paired) launch_mark<false, true>(ed, p, stats, stream);
  else launch_mark<false, false>(ed, p, stats, stream);
  const int64_t n0 = v.dir[0].num_items[0], n1 = v.dir[1].num_items[0];
  k_ed_heads<<<grid_for(std::max((n0 + n1) * RGCN_HEAD, NR), kThreads), kThreads, 0, stream>>>(
      v.dir[0].items[0], n0, ed->val[0], ed->head_w[0], v.dir[1].items[0], n1, ed->val[1], ed->head_w[1], NR, ed->count);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

// ---------------------------------------------------------------------------------------------------------------- twins
// key of a column: (min, max) of its endpoints above the direction bit (1: source > destination); node ids are < 2^31,
// so bit 63 stays clear and key + 1 cannot wrap.  A self loop is a forward copy without a backward side.
__global__ __launch_bounds__(kThreads) void k_tw_keys(const int64_t* __restrict__ perm, const int32_t* __restrict__ col,
                                                      const int32_t* __restrict__ seg_f, int64_t E, int64_t R,
                                                      unsigned long long* __restrict__ key, int32_t* __restrict__ rel,
                                                      int32_t* __restrict__ ids) {
  const int64_t pos = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (pos >= E) return;
  ids[pos] = (int32_t)pos;                       // the columns in ascending order: what the stable sorts keep inside a run
  const int64_t e = clamp64(perm[pos], 0, E - 1);
  const int64_t seg = seg_f[pos], dst = seg / R, src = col[pos];
  const unsigned long long lo = (unsigned long long)(uint32_t)(src < dst ? src : dst);
  const unsigned long long hi = (unsigned long long)(uint32_t)(src < dst ? dst : src);
  key[e] = (lo << 32) | (hi << 1) | (src > dst ? 1ull : 0ull);
  rel[e] = (int32_t)(seg % R);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void k_tw_gather(const T* __restrict__ by_col, const int32_t* __restrict__ ids,
                                                        int64_t E, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < E) out[i] = by_col[ids[i]];
}

// first i in [0, E) with (rel[i], key[i]) >= (r, k) in the sorted order, E if none
__device__ inline int64_t tw_lower_bound(const int32_t* __restrict__ rel, const unsigned long long* __restrict__ key,
                                         int64_t E, int32_t r, unsigned long long k) {
  int64_t lo = 0, hi = E;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int32_t rm = rel[mid];
    if (rm < r || (rm == r && key[mid] < k)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ids: the columns sorted by (relation, min, max, direction, column), rel / key: their keys in that order.  The copies
// of (a, r, b) and of (b, r, a) form one run, forward copies first; a search finds the run's three borders whatever its
// length (a walk to the borders would be linear in the duplicates of one triple).
__global__ __launch_bounds__(kThreads) void k_tw_pair(const int32_t* __restrict__ ids, const int32_t* __restrict__ rel,
                                                      const unsigned long long* __restrict__ key, int64_t E,
                                                      int32_t* __restrict__ twin) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= E) return;
  const int32_t r = rel[i];
  const unsigned long long k = key[i], fwd = k & ~1ull;
  const int64_t f0 = tw_lower_bound(rel, key, E, r, fwd), b0 = tw_lower_bound(rel, key, E, r, fwd | 1ull),
                b1 = tw_lower_bound(rel, key, E, r, (fwd | 1ull) + 1ull);
  const bool backward = (k & 1ull) != 0;
  const int64_t j = i - (backward ? b0 : f0), others = backward ? b0 - f0 : b1 - b0;
  const int64_t at = clamp64((backward ? f0 : b0) + j, 0, E - 1);
  twin[clamp64(ids[i], 0, E - 1)] = j < others ? ids[at] : -1;   // surplus copies of the longer side stay alone
}

struct twin_scratch {
  unsigned long long *key = nullptr, *skey = nullptr;
  int32_t *rel = nullptr, *srel_in = nullptr, *srel = nullptr, *ids[3] = {nullptr, nullptr, nullptr};
  void* tmp = nullptr;
  ~twin_scratch() {
    for (void* p : {(void*)key, (void*)skey, (void*)rel, (void*)srel_in, (void*)srel, (void*)ids[0], (void*)ids[1], (void*)ids[2], tmp})
      (void)hipFree(p);
  }
};

// twin[] of rgcn_edge_dropout.h from the parent's forward structure (seg_f is built).  Everything allocated here is
// freed before it returns; it synchronises `stream`.
int build_twins(const rgcn_graph* g, const int32_t* seg_f, hipStream_t stream, int32_t* twin) {
  const int64_t E = g->E;
  const size_t n = (size_t)E;
  twin_scratch sc;
  RGCN_HIP_TRY(hipMalloc((void**)&sc.key, n * sizeof(unsigned long long)));
  RGCN_HIP_TRY(hipMalloc((void**)&sc.skey, n * sizeof(unsigned long long)));
  for (int32_t** p : {&sc.rel, &sc.srel_in, &sc.srel, &sc.ids[0], &sc.ids[1], &sc.ids[2]})
    RGCN_HIP_TRY(hipMalloc((void**)p, n * sizeof(int32_t)));
  RGCN_HIP_TRY(hipMemsetAsync(sc.key, 0, n * sizeof(unsigned long long), stream));   // (a perm that skips a column leaves
  RGCN_HIP_TRY(hipMemsetAsync(sc.rel, 0, n * sizeof(int32_t), stream));              //  its keys defined)
  int rel_bits = 1;                              // bits that hold R - 1 (R < 2^31)
  while (rel_bits < 31 && ((g->R - 1) >> rel_bits) != 0) ++rel_bits;
  size_t bytes_key = 0, bytes_rel = 0;
  RGCN_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes_key, sc.key, sc.skey, sc.ids[0], sc.ids[1], (int)E, 0, 63, stream));
  RGCN_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes_rel, sc.srel_in, sc.srel, sc.ids[1], sc.ids[2], (int)E, 0,
                                                   rel_bits, stream));
  size_t bytes = std::max(bytes_key, bytes_rel);
  RGCN_HIP_TRY(hipMalloc(&sc.tmp, bytes + 256));
  const unsigned grid = grid_for(E, kThreads);
  k_tw_keys<<<grid, kThreads, 0, stream>>>(g->dir[0].perm, g->dir[0].col, seg_f, E, g->R, sc.key, sc.rel, sc.ids[0]);
  // least significant first: direction and node pair, then the relation; both passes stable, so a run keeps column order
  size_t b = bytes;
  RGCN_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(sc.tmp, b, sc.key, sc.skey, sc.ids[0], sc.ids[1], (int)E, 0, 63, stream));
  k_tw_gather<int32_t><<<grid, kThreads, 0, stream>>>(sc.rel, sc.ids[1], E, sc.srel_in);
  b = bytes;
  RGCN_HIP_TRY(hipcub::DeviceRadixSort::SortPairs(sc.tmp, b, sc.srel_in, sc.srel, sc.ids[1], sc.ids[2], (int)E, 0, rel_bits, stream));
  k_tw_gather<unsigned long long><<<grid, kThreads, 0, stream>>>(sc.key, sc.ids[2], E, sc.skey);
  k_tw_pair<<<grid, kThreads, 0, stream>>>(sc.ids[2], sc.srel, sc.skey, E, twin);
  RGCN_HIP_TRY(hipGetLastError());
  RGCN_HIP_TRY(hipStreamSynchronize(stream));    // the scratch is freed on return
  return RGCN_OK;
}

int create_impl(const rgcn_graph* g, hipStream_t stream, rgcn_edge_dropout* ed) {
  const int64_t E = g->E, NR = g->N * g->R;
  ed->parent = g;
  ed->view = *g;                                 // every pointer shared ...
  RGCN_HIP_TRY(hipMalloc((void**)&ed->kept, (size_t)std::max<int64_t>(NR, 1) * sizeof(int32_t)));
  RGCN_HIP_TRY(hipMalloc((void**)&ed->count, (size_t)std::max<int64_t>(NR, 1) * sizeof(int32_t)));
  RGCN_HIP_TRY(hipMemsetAsync(ed->kept, 0, (size_t)std::max<int64_t>(NR, 1) * sizeof(int32_t), stream));
  RGCN_HIP_TRY(hipMemsetAsync(ed->count, 0, (size_t)std::max<int64_t>(NR, 1) * sizeof(int32_t), stream));
  RGCN_HIP_TRY(hipMalloc((void**)&ed->msum, (size_t)std::max<int64_t>(NR, 1) * sizeof(float)));
  RGCN_HIP_TRY(hipMemsetAsync(ed->msum, 0, (size_t)std::max<int64_t>(NR, 1) * sizeof(float), stream));
  RGCN_HIP_TRY(hipMalloc((void**)&ed->mmax, (size_t)std::max<int64_t>(NR, 1) * sizeof(float)));
  RGCN_HIP_TRY(hipMemsetAsync(ed->mmax, 0, (size_t)std::max<int64_t>(NR, 1) * sizeof(float), stream));
  for (int d = 0; d < 2; ++d) {                  // ... but the weights and their item-head copies
    rgcn_csr& c = ed->view.dir[d];
    c.weighted = true;
    c.val = nullptr;
    c.head_w = nullptr;
    if (E > 0) RGCN_HIP_TRY(hipMalloc((void**)&ed->val[d], (size_t)E * sizeof(float)));
    if (c.num_items[0] > 0)
      RGCN_HIP_TRY(hipMalloc((void**)&ed->head_w[d], (size_t)c.num_items[0] * RGCN_HEAD * sizeof(float)));
    c.val = ed->val[d];
    c.head_w = ed->head_w[d];
  }
  // bounds that hold for every draw: a forward segment's weights sum to k * fl(1 / k) <= 1 + 2^-23 (the margin
  // plan_structure gives a weighted structure); a transposed weight is <= 1, so a segment's sum is at most its length
  ed->view.dir[0].weight_bound = (float)(1.0 + 1e-6);
  std::vector<int32_t> rp((size_t)NR + 1);
  // ... and for every mask draw with values in [0, inf): M is a sum of non-negative terms through at most h rounded
  // additions on any path of the fixed order (h = ceil(L / 8) + 3 up to 64 edges, ceil(L / 256) + 6 + 3 past that),
  // so M >= sum m * (1 - u)^h, every quotient is <= m / M * (1 + u), and a segment's weights sum to at most
  // (1 + u) / (1 - u)^h, u = 2^-24.  That stays below 1 + 1e-6 up to L = 1,280; a longer forward segment raises the bound.
  RGCN_HIP_TRY(hipMemcpyAsync(rp.data(), g->dir[0].rowptr, (size_t)(NR + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  RGCN_HIP_TRY(hipStreamSynchronize(stream));
  int64_t longest_f = 0;
  for (int64_t s = 0; s < NR; ++s) longest_f = std::max<int64_t>(longest_f, rp[(size_t)s + 1] - rp[(size_t)s]);
  {
    const int64_t h = longest_f <= RGCN_CHUNK ? (longest_f + 7) / 8 + 3 : (longest_f + 255) / 256 + 9;
    const double u = 1.0 / 16777216.0;
    double b = 1.0 + u;
    for (int64_t i = 0; i < h; ++i) b /= 1.0 - u;
    if (b > (double)ed->view.dir[0].weight_bound) {   // (the float that stands there is 1 + 16 u)
      float fb = (float)b;
      if ((double)fb < b) fb = nextafterf(fb, 2.f);   // the conversion may have rounded down
      ed->view.dir[0].weight_bound = fb;
    }
  }
  RGCN_HIP_TRY(hipMemcpyAsync(rp.data(), g->dir[1].rowptr, (size_t)(NR + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  RGCN_HIP_TRY(hipStreamSynchronize(stream));
  int32_t longest = 1;
  for (int64_t s = 0; s < NR; ++s) longest = std::max(longest, rp[(size_t)s + 1] - rp[(size_t)s]);
  ed->view.dir[1].weight_bound = (float)longest;
  if (E > 0) {
    RGCN_HIP_TRY(hipMalloc((void**)&ed->seg_f, (size_t)E * sizeof(int32_t)));
    RGCN_HIP_TRY(hipMalloc((void**)&ed->seg_t, (size_t)E * sizeof(int32_t)));
    k_ed_segments<<<grid_for(E, kThreads), kThreads, 0, stream>>>(g->dir[0].rowptr, NR, E, g->R, nullptr, ed->seg_f);
    k_ed_segments<<<grid_for(E, kThreads), kThreads, 0, stream>>>(g->dir[1].rowptr, NR, E, g->R, g->dir[1].col, ed->seg_t);
    RGCN_HIP_TRY(hipGetLastError());
    RGCN_HIP_TRY(hipMalloc((void**)&ed->twin, (size_t)E * sizeof(int32_t)));
    const int rc = build_twins(g, ed->seg_f, stream, ed->twin);
    if (rc != RGCN_OK) return rc;
  }
  // the draw p = 0 without a window: usable at once (threshold 0 drops nothing, whatever the key)
  int64_t* rng = nullptr;
  RGCN_HIP_TRY(hipMalloc((void**)&rng, 2 * sizeof(int64_t)));
  int rc = hipMemsetAsync(rng, 0, 2 * sizeof(int64_t), stream) == hipSuccess ? RGCN_OK : RGCN_ERR_HIP;
  if (rc == RGCN_OK) rc = draw_impl(ed, draw_params{nullptr, nullptr, rng, 0, 0u, ed->twin}, false, false, nullptr, stream);
  if (rc == RGCN_OK && hipStreamSynchronize(stream) != hipSuccess) rc = RGCN_ERR_HIP;
  (void)hipFree(rng);
  return rc;
}

}  // namespace

extern "C" {

int rgcn_edge_dropout_create(const rgcn_graph* g, void* stream, rgcn_edge_dropout** out) {
  if (!out) return RGCN_ERR_ARG;
  *out = nullptr;
  if (!g) return RGCN_ERR_ARG;
  const rgcn_csr &f = g->dir[0], &t = g->dir[1];
  if (!f.rowptr || !t.rowptr || f.weighted || !t.weighted || f.n_key != g->N || f.n_other != g->N || t.n_key != g->N ||
      t.n_other != g->N)
    return RGCN_ERR_UNSUPPORTED;
  rgcn_edge_dropout* ed = new (std::nothrow) rgcn_edge_dropout();
  if (!ed) return RGCN_ERR_HIP;
  const int rc = create_impl(g, (hipStream_t)stream, ed);
  if (rc != RGCN_OK) {
    rgcn_edge_dropout_destroy(ed);
    return rc;
  }
  *out = ed;
  return RGCN_OK;
}

void rgcn_edge_dropout_destroy(rgcn_edge_dropout* ed) {
  if (!ed) return;
  for (int d = 0; d < 2; ++d) {
    (void)hipFree(ed->val[d]);
    (void)hipFree(ed->head_w[d]);
  }
  (void)hipFree(ed->kept);
  (void)hipFree(ed->count);
  (void)hipFree(ed->seg_f);
  (void)hipFree(ed->seg_t);
  (void)hipFree(ed->twin);
  (void)hipFree(ed->msum);
  (void)hipFree(ed->mmax);
  delete ed;                                     // the shared arrays stay the parent's
}

const rgcn_graph* rgcn_edge_dropout_graph(const rgcn_edge_dropout* ed) { return ed ? &ed->view : nullptr; }

const int32_t* rgcn_edge_dropout_kept(const rgcn_edge_dropout* ed) { return ed ? ed->kept : nullptr; }

int rgcn_edge_dropout_kept_export(const rgcn_edge_dropout* ed, int32_t* out, void* stream) {
  if (!ed) return RGCN_ERR_ARG;
  const size_t nr = (size_t)(ed->view.N * ed->view.R);
  if (nr && !out) return RGCN_ERR_ARG;           // (a graph without nodes has nothing to copy)
  RGCN_ALIGN_TRY(4, out);
  if (nr) RGCN_HIP_TRY(hipMemcpyAsync(out, ed->kept, nr * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return RGCN_OK;
}

int rgcn_edge_dropout_draw(rgcn_edge_dropout* ed, double p, const int64_t* rng, const int64_t* cursor, int64_t batch,
                           const int64_t* position, int64_t* stats, void* stream) {
  if (!ed || !rng || batch < 0) return RGCN_ERR_ARG;            // (bit 63 is no option: a negative batch)
  const bool hide_twins = (batch & RGCN_EDGE_DROPOUT_HIDE_TWINS) != 0, paired = (batch & RGCN_EDGE_DROPOUT_PAIRED) != 0;
  const bool masked = (batch & RGCN_EDGE_DROPOUT_MASK) != 0, attention = (batch & RGCN_EDGE_DROPOUT_ATTENTION) != 0;
  batch &= ~(RGCN_EDGE_DROPOUT_HIDE_TWINS | RGCN_EDGE_DROPOUT_PAIRED | RGCN_EDGE_DROPOUT_MASK |
             RGCN_EDGE_DROPOUT_ATTENTION);           // what is left is the window's length
  if (attention) {                                   // p is the slope there: its own range, nothing drawn, no shared word
    if (!(p >= 0.0 && p <= 1.0) || masked || paired) return RGCN_ERR_ARG;
    RGCN_ALIGN_TRY(8, rng, cursor, position, stats);
    return att_impl(ed, draw_params{position, cursor, nullptr, batch, 0u, ed->twin}, reinterpret_cast<const float*>(rng),
                    (float)p, hide_twins, stats, (hipStream_t)stream);
  }
  if (!(p >= 0.0 && p < 1.0)) return RGCN_ERR_ARG;            // NaN fails both compares
  if (masked && (p != 0.0 || paired)) return RGCN_ERR_ARG;    // a mask draw draws nothing: no p, no shared word
  RGCN_ALIGN_TRY(8, rng, cursor, position, stats);
  if (masked)
    return mask_impl(ed, draw_params{position, cursor, nullptr, batch, 0u, ed->twin}, reinterpret_cast<const float*>(rng),
                     hide_twins, stats, (hipStream_t)stream);
  const uint32_t threshold = (uint32_t)(uint64_t)(p * 4294967296.0);   // floor(p * 2^32) <= 2^32 - 1 for p < 1
  return draw_impl(ed, draw_params{position, cursor, rng, batch, threshold, ed->twin}, hide_twins, paired, stats,
                   (hipStream_t)stream);
}

}  // extern "C"
