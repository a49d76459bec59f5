// Gather + per-(node, relation) aggregation: the HBM-bound half of the layer.
//
// Replaces PyG RGCNConv.forward's per-relation `x.index_select(0, src)` ->
// `scatter_add_` (sum) -> `scatter_add_` (count) -> clamp(min=1) -> divide
// (SURVEY.md section 8a rows A3 + A4; reference call sites src/models/rgcn.py:123,128) and,
// with the transposed structure, the scatter that autograd runs for them in backward (A7).
//
// Layout: a feature row is d contiguous floats.  A lane group of G = d/4 lanes owns one
// work item (a run of <= 64 source rows of one (node, rel) segment); each lane holds a
// float4 column slice, so every neighbour row is read as one coalesced 16 B x G access and
// the neighbour sum needs no cross-lane reduction.  A wave64 carries 64/G items.  Eight
// row loads are kept in flight per group, the column ids of the next eight are fetched
// behind them, and the adds retire in edge order, which keeps the sum of an unsplit segment
// identical to a sequential scatter.
//
// A segment longer than 64 edges is walked as runs of 64; four consecutive runs (a pack) sit in one
// workgroup and are combined through LDS, so a segment of up to 256 edges is finished here and a
// longer one leaves one partial row per pack; k_reduce_partials sums the (contiguous) partial rows
// of a segment with a whole workgroup per item (up to 512 rows: 256/G row slots in parallel, LDS
// combine in slot order), so even a 100k-edge hub costs one extra short launch and the result is
// run-to-run deterministic.
//
// The grid of the level-0 launch has three parts, in dispatch order:
//   1. the gather proper: the workgroups that walk the live item slots;
//   2. zero-fill workgroups: a (node, relation) segment without an edge (half of C2's 92,778) is an item too, and the
//      plan's order makes these items the suffix of level 0.  Their rows are +0.0f and depend on nothing the walk
//      computes, so they are not walked (item, flags, id window, cnt and four divides for one zero row, in workgroups
//      dispatched after the walk has drained): a workgroup reads the `dst` of RGCN_ZERO_ROWS of them and stores.  A
//      SPARSE aggregate (RGCN_MODE_SPARSE_ROWS: one that stays inside a training pass, read only by the split transforms,
//      which never load those rows) has no part 2 at all, and its walk ends at the last live slot;
//   3. riders: the workgroups of a pending parameter-gradient slab reduction (rgcn_slab_reduce.h).  They are the last
//      to start, so what each of them takes is the tail of the launch: one batch of loads (all the slabs of its group
//      at C2), the adds in slab order, one barrier.
// The parts share nothing: no counter, no ticket, no workgroup waits for another.  Behind the walk is where the zero
// rows measured fastest (in front of it, behind the riders, interleaved with the walk: profiles/gather_empty_rows.txt),
// and behind the zero rows the riders: between the walk and the zero rows is 0.3 us slower at d = 128, in front of the
// walk 0.4 us faster at d = 128 and 0.75 us slower on the merged d = 64 gather (profiles/slab_riders.txt).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include <hip/hip_fp16.h>

#include "rgcn_common.h"
#include "rgcn_slab_reduce.h"
#include "rgcn_hub_finish.h"

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = RGCN_HEAD;   // rows in flight per lane group = ids that travel with an item
#ifndef RGCN_REDUCE_UNROLL
#define RGCN_REDUCE_UNROLL 16
#endif
#ifndef RGCN_ZERO_ROWS
#define RGCN_ZERO_ROWS 64            // rows of a zero-fill workgroup (32, 128 and 256 measured no better)
#endif

__device__ inline float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ inline float f4amax(const float4& a) { return fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w))); }

__device__ inline void f4add(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
__device__ inline void f4fma(float4& a, const float4& b, float s) {   // explicit fma: one rounding, in every build
  a.x = fmaf(b.x, s, a.x); a.y = fmaf(b.y, s, a.y); a.z = fmaf(b.z, s, a.z); a.w = fmaf(b.w, s, a.w);
}


// Column ids (and weights) of a work item, fetched by the lane group as a team.  A vector-memory
// instruction occupies the CU's address unit for the same 16 cycles whether it returns 1 KB of
// rows or one broadcast dword, and the per-lane form (every lane loading the same 8 ids, then the
// same 8 weights) made the id traffic HALF of the kernel's memory instructions - the gather ran
// with that unit 71 % busy (PMC: TA_TA_BUSY).  Here lane j of the group loads edge base + j of a
// window of G edges with ONE instruction, and the ids are handed round with ds_bpermute (__shfl,
// LDS crossbar, no memory).  The first RGCN_HEAD ids come with the item (head_col / head_w).
template <int G, bool WEIGHTED>
struct IdWindow {
  int cur, nxt, pos, len, nbase, end;
  float curw, nxtw;
  __device__ inline void fetch_next(int gl, const int32_t* __restrict__ col, const float* __restrict__ w) {
    const int e = nbase + gl;
    const bool ok = e < end;
    nxt = ok ? col[e] : -1;
    nxtw = (WEIGHTED && ok) ? w[e] : 0.f;
  }
  __device__ inline void init(int64_t item_id, int gl, const rgcn_item& it, const int32_t* __restrict__ col,
                              const float* __restrict__ w, const int32_t* __restrict__ head_col,
                              const float* __restrict__ head_w) {
    const bool h = gl < RGCN_HEAD;
    cur = h ? head_col[item_id * RGCN_HEAD + gl] : -1;
    curw = (WEIGHTED && h) ? head_w[item_id * RGCN_HEAD + gl] : 0.f;
    pos = 0;
    len = RGCN_HEAD;
    nbase = it.begin + RGCN_HEAD;
    end = it.end;
    fetch_next(gl, col, w);
  }
  __device__ inline void get(int (&idx)[RGCN_HEAD], float (&wt)[RGCN_HEAD]) const {
#pragma unroll
    for (int u = 0; u < RGCN_HEAD; ++u) {
      idx[u] = __shfl(cur, pos + u, G);
      wt[u] = WEIGHTED ? __shfl(curw, pos + u, G) : 0.f;
    }
  }
  __device__ inline void advance(int gl, const int32_t* __restrict__ col, const float* __restrict__ w) {
    pos += RGCN_HEAD;
    if (pos == len) {                     // the same iteration for every group of the wave
      cur = nxt;
      curw = nxtw;
      pos = 0;
      len = G;
      nbase += G;
      fetch_next(gl, col, w);             // in flight behind the rows of this round
    }
  }
};

// workgroup `bx` of the gather proper (the kernels below put riders before / behind it in their grids)
template <int G, bool WEIGHTED>
__device__ inline void aggregate_block(
    const int bx, float4* red, const float* __restrict__ src, const rgcn_item* __restrict__ items, int64_t nitems,
    const int32_t* __restrict__ col, const float* __restrict__ w, const float* __restrict__ cnt,
    float* __restrict__ agg, float* __restrict__ partial, int d, const int32_t* __restrict__ head_col,
    const float* __restrict__ head_w, unsigned* __restrict__ amax_out) {
  const int64_t item_id = ((int64_t)bx * kThreads + threadIdx.x) / G;
  const int c4 = ((int)threadIdx.x % G + (int)blockIdx.y * G) * 4;
  if (item_id >= nitems) return;                 // whole lane groups only
  const unsigned seen = rgcn_amax_peek(amax_out);
  const bool live = c4 < d;                      // lanes past the row end still carry ids for their group
  const rgcn_item it = items[item_id];
  // packs come first in the item order: the workgroup's first slot says whether any is in here
  const bool has_packs = (items[(int64_t)bx * (kThreads / G)].flags & RGCN_ITEM_PACK) != 0;

  float4 acc = f4zero();
  if constexpr (G >= RGCN_HEAD) {
    const int gl = (int)threadIdx.x % G;
    IdWindow<G, WEIGHTED> win;
    win.init(item_id, gl, it, col, w, head_col, head_w);
    for (int e = it.begin; e < it.end; e += kUnroll) {
      int idx[kUnroll];
      float wt[kUnroll];
      float4 v[kUnroll];
      win.get(idx, wt);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        v[u] = f4zero();
        if (live && idx[u] >= 0) v[u] = *reinterpret_cast<const float4*>(src + (size_t)idx[u] * d + c4);
      }
      win.advance(gl, col, w);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (WEIGHTED) f4fma(acc, v[u], wt[u]);
        else f4add(acc, v[u]);
      }
    }
  } else if (live) {                            // fewer than 8 lanes per row (d < 32): every lane loads the ids
    int idx_n[kUnroll];
    float wt_n[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      idx_n[u] = head_col[item_id * kUnroll + u];
      wt_n[u] = WEIGHTED ? head_w[item_id * kUnroll + u] : 0.f;
    }
    for (int e = it.begin; e < it.end; e += kUnroll) {
      int idx[kUnroll];
      float wt[kUnroll];
      float4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        idx[u] = idx_n[u];
        wt[u] = wt_n[u];
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        v[u] = f4zero();
        if (idx[u] >= 0) v[u] = *reinterpret_cast<const float4*>(src + (size_t)idx[u] * d + c4);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {   // ids of the next round, in flight behind the rows
        const int en = e + kUnroll + u;
        const bool ok = en < it.end;
        idx_n[u] = ok ? col[en] : -1;
        wt_n[u] = (WEIGHTED && ok) ? w[en] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        if (WEIGHTED) f4fma(acc, v[u], wt[u]);
        else f4add(acc, v[u]);
      }
    }
  }
  // Lanes that write nothing (members and padding of a pack, lanes past the row end) stay to the end with a maximum
  // of 0: rgcn_amax_publish wants the wave's lanes from 0 up to the last one with an item, not a subset with holes.
  bool writes = live;
  if (has_packs) {                               // the runs of a pack meet in LDS; its leader adds them in slot order
    red[threadIdx.x] = acc;
    __syncthreads();
    if (it.flags & (RGCN_ITEM_MEMBER | RGCN_ITEM_SKIP)) {
      writes = false;
    } else {
      const int followers = (it.flags >> RGCN_ITEM_FOLLOW_SHIFT) & (RGCN_PACK - 1);
      for (int f = 1; f <= followers; ++f) f4add(acc, red[threadIdx.x + f * G]);
    }
  }
  float lmax = 0.f;
  if (writes && (it.flags & RGCN_ITEM_FINAL)) {
    if (cnt) {  // mean: true division by max(1, segment size), as `sum / count` does
      const float c = cnt[it.dst];
      acc.x /= c; acc.y /= c; acc.z /= c; acc.w /= c;
    }
    *reinterpret_cast<float4*>(agg + (size_t)it.dst * d + c4) = acc;
    lmax = f4amax(acc);
  } else if (writes) {
    *reinterpret_cast<float4*>(partial + (size_t)it.dst * d + c4) = acc;
  }
  if (amax_out) rgcn_amax_publish(amax_out, lmax, seen);
}

// Rows of one zero-fill workgroup: whole passes of its 256 / G row slots.
template <int G>
constexpr int zero_rows() { return RGCN_ZERO_ROWS > kThreads / G ? RGCN_ZERO_ROWS : kThreads / G; }

// Zero-fill workgroup `zb`: the items [first + zb * zero_rows, ...) are segments without an edge (rgcn_csr::
// empty_items0), whose rows of `agg` are +0.0f whatever the table holds (0 / cnt, or a sum of nothing).  It reads their
// `dst` and stores the rows: no id window, no cnt, no amax (a zero never raises a maximum), nothing shared with any
// other workgroup.  1-D grids only (d <= 4 * G).
template <int G>
__device__ inline void zero_rows_block(const int64_t zb, const rgcn_item* __restrict__ items, int64_t first,
                                       int64_t nitems, float* __restrict__ agg, int d) {
  constexpr int kSlots = kThreads / G, kPasses = zero_rows<G>() / kSlots;
  const int c4 = ((int)threadIdx.x % G) * 4;
  const int64_t base = first + zb * zero_rows<G>() + (int)threadIdx.x / G;
  int32_t dst[kPasses];
#pragma unroll
  for (int p = 0; p < kPasses; ++p) {            // all the item loads first: one round trip, then stores only
    const int64_t i = base + (int64_t)p * kSlots;
    dst[p] = i < nitems ? items[i].dst : -1;
  }
  if (c4 >= d) return;
#pragma unroll
  for (int p = 0; p < kPasses; ++p)
    if (dst[p] >= 0) *reinterpret_cast<float4*>(agg + (size_t)dst[p] * d + c4) = f4zero();
}

// Grid of the level-0 launch, in dispatch order: `gather_blocks` workgroups of the gather proper, `zero_blocks`
// zero-fill workgroups, then the riders of a pending slab reduction (see the file header).
// (The weighted body takes 68 registers, one granule over the 64 that let eight waves share a SIMD; holding it to 64
// with amdgpu_waves_per_eu(8) costs three spilled registers and measured ~1 us on the d = 128 transposed gather, inside
// the box-to-box spread: left alone.)
template <int G, bool WEIGHTED>
__global__ __launch_bounds__(kThreads) void k_aggregate(
    const float* __restrict__ src, const rgcn_item* __restrict__ items, int64_t nitems,
    const int32_t* __restrict__ col, const float* __restrict__ w, const float* __restrict__ cnt,
    float* __restrict__ agg, float* __restrict__ partial, int d, const int32_t* __restrict__ head_col,
    const float* __restrict__ head_w, const rgcn_slab_job job, int gather_blocks, int zero_blocks,
    unsigned* __restrict__ amax_out) {
  __shared__ float4 red[kThreads];               // pack combine (see rgcn_common.h)
  const int bx = (int)blockIdx.x, zb = bx - gather_blocks, rb = zb - zero_blocks;
  if (rb >= 0) {                                // workgroups past both: a pending slab reduction rides along
    rgcn_slab_reduce_block<RGCN_SLAB_OUTS, RGCN_SLAB_GROUPS>(job, (int64_t)rb, red);
    return;
  }
  if (zb >= 0) {
    zero_rows_block<G>(zb, items, (int64_t)gather_blocks * (kThreads / G), nitems, agg, d);
    return;
  }
  aggregate_block<G, WEIGHTED>(bx, red, src, items, nitems, col, w, cnt, agg, partial, d, head_col, head_w, amax_out);
}

// fp16 feature table, fp32 accumulate (BASELINE.json configs[4]): the same walk with 8 halves
// (16 B) per lane, so a row costs half the bytes (132 / 260 B per edge at d = 64 / 128) and a
// wave64 carries 64 / (d/8) items.  Sums, partial rows and the output stay fp32.
template <int G, bool WEIGHTED>
__global__ __launch_bounds__(kThreads) void k_aggregate_h(
    const __half* __restrict__ src, const rgcn_item* __restrict__ items, int64_t nitems,
    const int32_t* __restrict__ col, const float* __restrict__ w, const float* __restrict__ cnt,
    float* __restrict__ agg, float* __restrict__ partial, int d, const int32_t* __restrict__ head_col,
    const float* __restrict__ head_w) {
  const int64_t item_id = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / G;
  __shared__ float4 red[2 * kThreads];           // pack combine: two float4 per lane
  const int c8 = ((int)threadIdx.x % G + (int)blockIdx.y * G) * 8;
  if (item_id >= nitems) return;
  const bool live = c8 < d;
  const rgcn_item it = items[item_id];
  const bool has_packs = (items[(int64_t)blockIdx.x * (kThreads / G)].flags & RGCN_ITEM_PACK) != 0;

  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  auto accumulate = [&](const uint4 (&v)[kUnroll], const float (&wt)[kUnroll]) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const __half2* h2 = reinterpret_cast<const __half2*>(&v[u]);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float2 f = __half22float2(h2[k]);
        if (WEIGHTED) {
          acc[2 * k] = fmaf(f.x, wt[u], acc[2 * k]);
          acc[2 * k + 1] = fmaf(f.y, wt[u], acc[2 * k + 1]);
        } else {                                  // rows of absent edges were loaded as zeros
          acc[2 * k] += f.x;
          acc[2 * k + 1] += f.y;
        }
      }
    }
  };
  if constexpr (G >= RGCN_HEAD) {                 // ids fetched by the group as a team (see IdWindow)
    const int gl = (int)threadIdx.x % G;
    IdWindow<G, WEIGHTED> win;
    win.init(item_id, gl, it, col, w, head_col, head_w);
    for (int e = it.begin; e < it.end; e += kUnroll) {
      int idx[kUnroll];
      float wt[kUnroll];
      uint4 v[kUnroll];
      win.get(idx, wt);
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (live && idx[u] >= 0) v[u] = *reinterpret_cast<const uint4*>(src + (size_t)idx[u] * d + c8);
      }
      win.advance(gl, col, w);
      accumulate(v, wt);
    }
  } else if (live) {
    int idx_n[kUnroll];
    float wt_n[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      idx_n[u] = head_col[item_id * kUnroll + u];
      wt_n[u] = WEIGHTED ? head_w[item_id * kUnroll + u] : 0.f;
    }
    for (int e = it.begin; e < it.end; e += kUnroll) {
      int idx[kUnroll];
      float wt[kUnroll];
      uint4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        idx[u] = idx_n[u];
        wt[u] = wt_n[u];
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        v[u] = make_uint4(0u, 0u, 0u, 0u);
        if (idx[u] >= 0) v[u] = *reinterpret_cast<const uint4*>(src + (size_t)idx[u] * d + c8);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int en = e + kUnroll + u;
        const bool ok = en < it.end;
        idx_n[u] = ok ? col[en] : -1;
        wt_n[u] = (WEIGHTED && ok) ? w[en] : 0.f;
      }
      accumulate(v, wt);
    }
  }
  if (has_packs) {
    red[2 * threadIdx.x] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    red[2 * threadIdx.x + 1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
    __syncthreads();
    if (it.flags & (RGCN_ITEM_MEMBER | RGCN_ITEM_SKIP)) return;
    const int followers = (it.flags >> RGCN_ITEM_FOLLOW_SHIFT) & (RGCN_PACK - 1);
    for (int f = 1; f <= followers; ++f) {
      const float4 a = red[2 * (threadIdx.x + f * G)], b = red[2 * (threadIdx.x + f * G) + 1];
      acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
      acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
    }
  }
  if (!live) return;
  float* out = (it.flags & RGCN_ITEM_FINAL) ? agg : partial;
  if ((it.flags & RGCN_ITEM_FINAL) && cnt) {
    const float c = cnt[it.dst];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] /= c;
  }
  float4* o4 = reinterpret_cast<float4*>(out + (size_t)it.dst * d + c8);
  o4[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  o4[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// One workgroup per item: rows [begin, end) of `partial` (contiguous) -> one row.
// Slot s of SLOTS = 256/G sums rows begin+s, begin+s+SLOTS, ... in order; the slots are then
// added in slot order through LDS.  Reads and writes of `partial` never alias inside one
// launch: a level reads rows written by the level below and writes rows of its own range.
template <int G>
__global__ __launch_bounds__(kThreads) void k_reduce_partials(const rgcn_item* __restrict__ items,
                                                              const float* __restrict__ cnt,
                                                              float* __restrict__ agg, float* partial, int d,
                                                              unsigned* __restrict__ amax_out) {
  __shared__ float4 red[kThreads];
  const float lmax = rgcn_reduce_item<G>(items[blockIdx.x], cnt, agg, partial, d, (int)blockIdx.y * G, red);
  if (amax_out && (int)threadIdx.x < G && (((int)threadIdx.x + (int)blockIdx.y * G) * 4 < d) &&
      (items[blockIdx.x].flags & RGCN_ITEM_FINAL))
    rgcn_amax_publish(amax_out, lmax);
}

template <int G>
void launch_level(const rgcn_csr* c, int level, bool weighted, const float* x, const float* cnt, float* agg,
                  float* partial, int d, hipStream_t stream, const rgcn_slab_job* tail = nullptr,
                  unsigned* amax_out = nullptr, bool sparse = false) {
  int64_t nitems = c->num_items[level];
  if (nitems == 0) return;
  const unsigned gy = (unsigned)ceil_div64(d, 4 * G);
  if (level == 0) {
    // Segments without an edge (the suffix of the item order, rgcn_csr::empty_items0) only need their zero rows: the
    // gather proper covers the live slots rounded up to whole workgroups - the few empty items inside the last of them
    // go the walk's way - and zero-fill workgroups store the rest.  Where the slab rider is allowed (can_ride below):
    // the fp32 gather on a 1-D grid, d <= 256.  A 2-D grid (d > 256) and k_aggregate_h walk every item as before.
    const int64_t slots = kThreads / G;
    const int64_t walked = gy == 1 ? std::min(nitems, ceil_div64(nitems - c->empty_items0, slots) * slots) : nitems;
    const unsigned gather_blocks = (unsigned)ceil_div64(walked, slots);
    // A sparse aggregate (RGCN_MODE_SPARSE_ROWS; gy == 1 is the caller's check) gets no zero-fill workgroups, and the
    // walk's last workgroup ends at the last live slot: no row of a segment without an edge is written at all.
    if (sparse) nitems -= c->empty_items0;
    const unsigned zero_blocks = sparse ? 0u : (unsigned)ceil_div64(nitems - walked, zero_rows<G>());
    const rgcn_slab_job job = tail ? *tail : rgcn_slab_job{};
    dim3 grid(gather_blocks + zero_blocks + (tail ? (unsigned)rgcn_slab_reduce_blocks(job) : 0u), gy);   // tail only with gy == 1
    if (grid.x == 0) return;                     // (a sparse aggregate of a structure without any edge)
    if (weighted)
      k_aggregate<G, true><<<grid, kThreads, 0, stream>>>(x, c->items[0], nitems, c->col, c->val, cnt, agg, partial, d,
                                                          c->head_col, c->head_w, job, (int)gather_blocks,
                                                          (int)zero_blocks, amax_out);
    else
      k_aggregate<G, false><<<grid, kThreads, 0, stream>>>(x, c->items[0], nitems, c->col, nullptr, cnt, agg, partial, d,
                                                           c->head_col, nullptr, job, (int)gather_blocks,
                                                           (int)zero_blocks, amax_out);
  } else {
    dim3 grid((unsigned)nitems, gy);
    k_reduce_partials<G><<<grid, kThreads, 0, stream>>>(c->items[level], cnt, agg, partial, d, amax_out);
  }
}

template <int G>
void launch_level0_h(const rgcn_csr* c, bool weighted, const __half* x, const float* cnt, float* agg, float* partial,
                     int d, hipStream_t stream) {
  const int64_t nitems = c->num_items[0];
  if (nitems == 0) return;
  dim3 grid((unsigned)ceil_div64(nitems, kThreads / G), (unsigned)ceil_div64(d, 8 * G));
  if (weighted)
    k_aggregate_h<G, true><<<grid, kThreads, 0, stream>>>(x, c->items[0], nitems, c->col, c->val, cnt, agg, partial, d,
                                                            c->head_col, c->head_w);
  else
    k_aggregate_h<G, false><<<grid, kThreads, 0, stream>>>(x, c->items[0], nitems, c->col, nullptr, cnt, agg, partial, d,
                                                             c->head_col, nullptr);
}

int aggregate_levels(const rgcn_graph* g, int transposed, int first, int last, const float* x, int64_t d,
                     float* agg, void* workspace, size_t workspace_bytes, void* stream_, bool half_in,
                     const rgcn_slab_job* tail, float* amax, bool sparse) {
  if (!g) return RGCN_ERR_ARG;
  const rgcn_csr* c = &g->dir[transposed ? 1 : 0];
  hipStream_t stream = (hipStream_t)stream_;
  if (!tail || !tail->slab) tail = nullptr;     // nothing pending
  if (tail && (!tail->grad_weight || tail->splits <= 0 || tail->Kc <= 0 || tail->N <= 0 || (tail->N & 3)))
    return RGCN_ERR_ARG;
  if (tail && c->rowptr && c->n_key == 0) {     // nothing to gather: the reduction still has to run
    RGCN_ALIGN_TRY(16, tail->slab, tail->bias_part, tail->grad_weight, tail->grad_root, tail->grad_bias);
    k_slab_reduce<<<(unsigned)rgcn_slab_reduce_blocks(*tail), 256, 0, stream>>>(*tail);
    RGCN_HIP_TRY(hipGetLastError());
    return RGCN_OK;
  }
  if (d <= 0 || (d & 3) || (half_in && (d & 7))) return RGCN_ERR_ARG;
  if (!c->rowptr) return RGCN_ERR_ARG;   // direction not built
  if (c->n_key == 0) return RGCN_OK;     // no row to write: an empty result has no address
  if (!agg || !x) return RGCN_ERR_ARG;
  if (d > (1 << 20)) return RGCN_ERR_UNSUPPORTED;
  if (first < 0 || last > c->num_levels || first > last) return RGCN_ERR_ARG;
  if (c->num_partials > 0 &&
      (!workspace || workspace_bytes < (size_t)c->num_partials * (size_t)d * sizeof(float)))
    return RGCN_ERR_WORKSPACE;
  float* partial = (float*)workspace;
  unsigned* amax_out = reinterpret_cast<unsigned*>(amax);
  if (amax && half_in) return RGCN_ERR_UNSUPPORTED;            // the fp16-table gather feeds the fp16 transform: no scale needed
  // no zero rows: only where the zero-fill workgroups exist (fp32 table, 1-D grid) and the consumers can tell the rows
  if (sparse && (half_in || d > 256 || !c->tile_mask)) return RGCN_ERR_UNSUPPORTED;
  // a lane reads 16 bytes of a table row (four floats, eight halves) and writes float4; amax heads are single words
  RGCN_ALIGN_TRY(16, x, agg, workspace);
  RGCN_ALIGN_TRY(4, amax);
  if (tail) RGCN_ALIGN_TRY(16, tail->slab, tail->bias_part, tail->grad_weight, tail->grad_root, tail->grad_bias);
  const float* cnt = c->weighted ? nullptr : c->val;
  const bool weighted = c->weighted;
  const int q = (int)(d / 4);
  // a pending slab reduction rides in the level-0 launch when that launch is a plain 1-D grid of the
  // fp32 gather with work of its own; otherwise it is launched by itself, first
  const bool can_ride = !half_in && first == 0 && last > 0 && d <= 256 && c->num_items[0] > 0;
  if (tail && !can_ride) {
    k_slab_reduce<<<(unsigned)rgcn_slab_reduce_blocks(*tail), 256, 0, stream>>>(*tail);
    tail = nullptr;
  }
  for (int l = first; l < last; ++l) {
    const rgcn_slab_job* t0 = l == 0 ? tail : nullptr;
    if (l == 0 && half_in) {                    // fp16 table: 8 columns per lane
      const __half* xh = reinterpret_cast<const __half*>(x);
      const int q8 = (int)(d / 8);
      if (q8 <= 1) launch_level0_h<1>(c, weighted, xh, cnt, agg, partial, (int)d, stream);
      else if (q8 <= 2) launch_level0_h<2>(c, weighted, xh, cnt, agg, partial, (int)d, stream);
      else if (q8 <= 4) launch_level0_h<4>(c, weighted, xh, cnt, agg, partial, (int)d, stream);
      else if (q8 <= 8) launch_level0_h<8>(c, weighted, xh, cnt, agg, partial, (int)d, stream);
      else if (q8 <= 16) launch_level0_h<16>(c, weighted, xh, cnt, agg, partial, (int)d, stream);
      else if (q8 <= 32) launch_level0_h<32>(c, weighted, xh, cnt, agg, partial, (int)d, stream);
      else launch_level0_h<64>(c, weighted, xh, cnt, agg, partial, (int)d, stream);
      continue;
    }
    if (q <= 1) launch_level<1>(c, l, weighted, x, cnt, agg, partial, (int)d, stream, t0, amax_out, sparse);
    else if (q <= 2) launch_level<2>(c, l, weighted, x, cnt, agg, partial, (int)d, stream, t0, amax_out, sparse);
    else if (q <= 4) launch_level<4>(c, l, weighted, x, cnt, agg, partial, (int)d, stream, t0, amax_out, sparse);
    else if (q <= 8) launch_level<8>(c, l, weighted, x, cnt, agg, partial, (int)d, stream, t0, amax_out, sparse);
    else if (q <= 16) launch_level<16>(c, l, weighted, x, cnt, agg, partial, (int)d, stream, t0, amax_out, sparse);
    else if (q <= 32) launch_level<32>(c, l, weighted, x, cnt, agg, partial, (int)d, stream, t0, amax_out, sparse);
    else launch_level<64>(c, l, weighted, x, cnt, agg, partial, (int)d, stream, t0, amax_out, sparse);
  }
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // namespace

extern "C" {

size_t rgcn_aggregate_workspace_bytes(const rgcn_graph* g, int transposed, int64_t d) {
  if (!g || d <= 0) return 0;
  return (size_t)g->dir[transposed ? 1 : 0].num_partials * (size_t)d * sizeof(float);
}

int rgcn_aggregate_ex(const rgcn_graph* g, int transposed, const void* x, int x_f16, int64_t d, float* agg,
                      void* workspace, size_t workspace_bytes, int first_level, int last_level, const rgcn_slab_job* job,
                      float* amax, void* stream) {
  if (!g) return RGCN_ERR_ARG;
  if (x_f16 & RGCN_MODE_EDGE_SUM)               // not a gather: per-edge values summed per segment (edge_grad.hip)
    return rgcn_edge_sum(g, transposed, x, x_f16, d, agg, first_level, last_level, job, amax, stream);
  if ((x_f16 & RGCN_MODE_MEAN_GRAD) && !(x_f16 & RGCN_MODE_WEIGHT_GRAD)) return RGCN_ERR_ARG;
  if ((x_f16 & RGCN_MODE_LOG_WEIGHT_GRAD) && !(x_f16 & RGCN_MODE_WEIGHT_GRAD)) return RGCN_ERR_ARG;
  if ((x_f16 & RGCN_MODE_LOG_WEIGHT_GRAD) && (x_f16 & RGCN_MODE_MEAN_GRAD)) return RGCN_ERR_ARG;   // one or the other
  if (x_f16 & RGCN_MODE_WEIGHT_GRAD)            // not a gather: the adjoint in the edge weights (edge_grad.hip)
    return rgcn_edge_grad(g, transposed, x, x_f16, d, agg, workspace, workspace_bytes, first_level, last_level, job, amax,
                          stream);
  return aggregate_levels(g, transposed, first_level, last_level < 0 ? g->dir[transposed ? 1 : 0].num_levels : last_level,
                          reinterpret_cast<const float*>(x), d, agg, workspace, workspace_bytes, stream, (x_f16 & 1) != 0, job,
                          amax, (x_f16 & RGCN_MODE_SPARSE_ROWS) != 0);
}

int rgcn_aggregate(const rgcn_graph* g, int transposed, const float* x, int64_t d, float* agg,
                   void* workspace, size_t workspace_bytes, void* stream) {
  return rgcn_aggregate_ex(g, transposed, x, 0, d, agg, workspace, workspace_bytes, 0, -1, nullptr, nullptr, stream);
}

int rgcn_aggregate_deferrable(const rgcn_graph* g, int transposed, int64_t d) {
  if (!g) return 0;
  const rgcn_csr& c = g->dir[transposed ? 1 : 0];
  return (c.num_levels == 2 && c.fin_ptr && (d == 64 || d == 128 || d == 256)) ? 1 : 0;
}

}  // extern "C"
