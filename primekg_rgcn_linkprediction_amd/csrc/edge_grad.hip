// The gather's adjoint in its edge weights (include/rgcn_hip.h, RGCN_MODE_WEIGHT_GRAD of rgcn_aggregate_ex):
//
//   out[p] = < gagg[s(p), :], x[col[p], :] >            one fp32 dot product per edge of a direction's CSR
//
// for agg[s] = sum_p w[p] * x[col[p]] this is dL/dw[p] given gagg = dL/dagg.  It reads the rows the gather reads and
// walks the gather's own level-0 work items (rgcn_plan.h: level 0 covers every edge, hub segments included, as runs of
// <= 64 edges of ONE segment), so a lane group of G = d / 4 lanes (rounded up to a power of two) owns an item, keeps
// its float4 slice of the segment's gagg row in registers for the whole run, and has eight source rows in flight.
// The eight partial dots of a round are reduced over the group TOGETHER: a reduce-scatter over the top three lane
// bits (4 + 2 + 1 exchanges) leaves one edge per lane, log2(G) - 3 butterfly steps finish it, and the eight lanes
// whose low bits are zero store eight consecutive floats.  Every exchange is a fixed __shfl_xor, so a dot has one
// summation tree whatever the launch looks like: run-to-run identical bits, no atomics.
//
// RGCN_MODE_MEAN_GRAD, out[p] = (dot[p] - S * w) * w with S the segment's sum of dots in the order the header states:
// a segment of <= 64 edges is ONE item, so its lane group has every dot pass through its registers - it keeps eight
// partial sums (edge slot j of every round), combines them over the same three lane bits, and the lanes that stored
// the dots rewrite their own positions (the first round's from registers, later rounds re-read: a lane's own stores).
// Longer segments - packs of the plan, a handful per graph - are finished by a second short launch: a workgroup looks
// at 256 segments, and all of its threads take the long ones among them one by one, in place.
//
// RGCN_MODE_LOG_WEIGHT_GRAD, out[p] = w[p] * (dot[p] - S) with S the segment's sum of fl(w[q] * dot[q]) in the SAME
// fixed order, on a weighted structure whose weights are normalised per segment (the forward direction of an edge
// dropout's view): the same frame with one more operand per edge.  The weight of the position a lane stores is loaded
// from a clamped index before the round's row loads - independent of them, never under a branch - and the rewrite of
// the later rounds re-reads the weights beside the dots in one batch.
//
// RGCN_MODE_EDGE_SUM, the inverse shape: one float per ORIGINAL column in, out[s] = the sum over the segment's positions
// of x[perm[pos]] in the same fixed order.  A segment has one owner, as in k_edge_long: a workgroup looks at 256
// segments, a thread sums its own if it has at most 64 edges (a round of eight positions IS the eight strided partial
// sums), the longer ones are taken one at a time by all 256 threads.  Every segment is written, an empty one with +0.0f.
#include "rgcn_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRound = RGCN_HEAD;     // edges per round = rows in flight per lane group

__device__ inline float dot4(const float4& g, const float4& v) {   // four fmaf from +0: a dot is never -0
  float p = fmaf(v.x, g.x, 0.f);
  p = fmaf(v.y, g.y, p);
  p = fmaf(v.z, g.z, p);
  return fmaf(v.w, g.w, p);
}

// The segment of a level-0 item.  A single item and the runs of a one-pack segment name it in `dst`; the runs of a
// longer segment name a partial row there, so the segment is found from the run's first edge: the last s with
// rowptr[s] <= begin < rowptr[s + 1] (segments without an edge share their neighbour's offset and are passed over).
__device__ inline int item_segment(const rgcn_item& it, const int32_t* __restrict__ rowptr, int64_t NR) {
  if (!(it.flags & RGCN_ITEM_PACK) || it.begin >= it.end) return it.dst;
  int64_t lo = 0, hi = NR + 1;                    // rowptr[0] = 0 <= begin < E = rowptr[NR]: 1 <= lo <= NR at the end
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (rowptr[mid] <= it.begin) lo = mid + 1;
    else hi = mid;
  }
  return (int)(lo - 1);
}

// The mean mode's arithmetic, each operation rounded by itself (no contraction into an fma, whatever the build says).
__device__ inline float mean_weight(float cnt) { return __fdiv_rn(1.0f, cnt); }
__device__ inline float mean_scaled_sum(float sum, float w) {
#pragma clang fp contract(off)
  return sum * w;
}
__device__ inline float mean_value(float dot, float sw, float w) {
#pragma clang fp contract(off)
  return (dot - sw) * w;
}

// The log-weight mode's arithmetic: the product inside S, and the value (+0.0f at a zero weight, whatever the rest is).
__device__ inline float logw_term(float w, float dot) {
#pragma clang fp contract(off)
  return w * dot;
}
__device__ inline float logw_value(float dot, float sum, float w) {
#pragma clang fp contract(off)
  const float v = w * (dot - sum);
  return w == 0.f ? 0.f : v;
}

enum : int { kPlain = 0, kMean = 1, kLogW = 2 };   // what a launch does with the dots
// what is subtracted from every dot of a segment, and the value of a position, by mode (w: w[s], or the position's own)
template <int MODE>
__device__ inline float seg_total(float sum, float w) { return MODE == kLogW ? sum : mean_scaled_sum(sum, w); }
template <int MODE>
__device__ inline float seg_value(float dot, float total, float w) {
  return MODE == kLogW ? logw_value(dot, total, w) : mean_value(dot, total, w);
}

template <int G, int MODE>
__global__ __launch_bounds__(kThreads) void k_edge_dot(
    const float* __restrict__ x, const float* __restrict__ gagg, const rgcn_item* __restrict__ items, int64_t nitems,
    const int32_t* __restrict__ rowptr, int64_t NR, const int32_t* __restrict__ col,
    const int32_t* __restrict__ head_col, const float* __restrict__ cnt, float* out, int d) {
  constexpr bool MEAN = MODE == kMean, LOGW = MODE == kLogW, SUMS = MODE != kPlain;   // cnt: cnt[s] (mean), w[p] (log weight)
  const int64_t item_id = ((int64_t)blockIdx.x * kThreads + threadIdx.x) / G;
  if (item_id >= nitems) return;                  // whole lane groups only
  const int gl = (int)threadIdx.x % G;
  const bool live = gl * 4 < d;                   // lanes past the row end carry +0 into the exchanges
  const int c4 = live ? gl * 4 : 0;
  const rgcn_item it = items[item_id];
  if (it.begin >= it.end) return;                 // padding slot of a pack; a segment without an edge
  const int seg = item_segment(it, rowptr, NR);
  float4 g = *reinterpret_cast<const float4*>(gagg + (size_t)seg * d + c4);
  if (!live) g = make_float4(0.f, 0.f, 0.f, 0.f);
  const int last = it.end - 1;
  // mean mode: an item that is no pack is a whole segment (<= 64 edges) and is finished here
  const bool finish = SUMS && !(it.flags & RGCN_ITEM_PACK);
  float w = 0.f;
  if constexpr (MEAN) {
    if (finish) w = mean_weight(cnt[seg]);
  }

  if constexpr (G >= kRound) {
    // ids: lane u < 8 of the group holds the id of edge e + u; the first round's come with the item (padded with -1),
    // a later round's are loaded one round ahead from a clamped position - never under a branch
    int cur = head_col[item_id * kRound + (gl & (kRound - 1))];
    const int slot = gl / (G / kRound);           // the top three lane bits, read as a number: the edge of a round
    const bool stores = gl % (G / kRound) == 0;
    float part = 0.f, first = 0.f;                // mean: this slot's partial sum; the first round's dot
    float wp = 0.f, first_w = 0.f;                // log weight: the weight of this round's / the first round's position
    for (int64_t e = it.begin; e < it.end; e += kRound) {       // int64: a run may end within a round of 2^31
      const int nxt = col[min(e + kRound + (gl & (kRound - 1)), (int64_t)last)];
      if constexpr (LOGW) wp = cnt[min(e + slot, (int64_t)last)];
      float p[kRound];
      float4 v[kRound];
#pragma unroll
      for (int u = 0; u < kRound; ++u) {
        const int idx = max(__shfl(cur, u, G), 0);          // past the item's end: some valid row, never stored
        v[u] = *reinterpret_cast<const float4*>(x + (size_t)idx * d + c4);
      }
#pragma unroll
      for (int u = 0; u < kRound; ++u) p[u] = dot4(g, v[u]);
      cur = nxt;
      // reduce-scatter over the three top lane bits: a lane whose bit is set keeps the upper half of the edges
#pragma unroll
      for (int half = kRound / 2, off = G / 2; half >= 1; half >>= 1, off >>= 1) {
        const bool up = (gl & off) != 0;
#pragma unroll
        for (int j = 0; j < half; ++j) {
          const float keep = up ? p[j + half] : p[j], send = up ? p[j] : p[j + half];
          p[j] = keep + __shfl_xor(send, off, G);
        }
      }
#pragma unroll
      for (int off = G / 16; off >= 1; off >>= 1) p[0] += __shfl_xor(p[0], off, G);
      const int64_t mine = e + slot;
      if (stores && mine < it.end) out[mine] = p[0];
      if (SUMS) {
        float term = p[0];
        if constexpr (LOGW) term = logw_term(wp, p[0]);
        part += mine < it.end ? term : 0.f;
        if (e == it.begin) first = p[0];
        if constexpr (LOGW) {
          if (e == it.begin) first_w = wp;
        }
      }
    }
    if (finish) {
      // ((P0 + P4) + (P2 + P6)) + ((P1 + P5) + (P3 + P7)): the slots differ in the top three lane bits
      float sum = part;
#pragma unroll
      for (int off = G / 2; off >= G / kRound; off >>= 1) sum += __shfl_xor(sum, off, G);
      const float sw = seg_total<MODE>(sum, w);
      const int64_t mine = (int64_t)it.begin + slot;
      if (stores && mine < it.end) out[mine] = seg_value<MODE>(first, sw, LOGW ? first_w : w);
      if (stores && it.end - it.begin > kRound) {             // later rounds: this lane's own stores, re-read in one batch
        float later[kRound - 1], later_w[kRound - 1];         // (log weight: their weights beside them)
#pragma unroll
        for (int r = 1; r < kRound; ++r) {
          later[r - 1] = out[min(mine + r * kRound, (int64_t)last)];
          later_w[r - 1] = LOGW ? cnt[min(mine + r * kRound, (int64_t)last)] : w;
        }
#pragma unroll
        for (int r = 1; r < kRound; ++r)
          if (mine + r * kRound < it.end) out[mine + r * kRound] = seg_value<MODE>(later[r - 1], sw, later_w[r - 1]);
      }
    }
  } else {
    int idx_n[kRound];                                      // fewer than 8 lanes per row: every lane loads the ids
    float part[kRound], first[kRound], wp[kRound], first_w[kRound];   // wp, first_w: the log weight mode's operands
#pragma unroll
    for (int u = 0; u < kRound; ++u) {
      idx_n[u] = col[min((int64_t)it.begin + u, (int64_t)last)];
      part[u] = first[u] = 0.f;
      wp[u] = first_w[u] = w;
    }
    for (int64_t e = it.begin; e < it.end; e += kRound) {
      float p[kRound];
      float4 v[kRound];
#pragma unroll
      for (int u = 0; u < kRound; ++u) v[u] = *reinterpret_cast<const float4*>(x + (size_t)idx_n[u] * d + c4);
      if constexpr (LOGW) {
#pragma unroll
        for (int u = 0; u < kRound; ++u) wp[u] = cnt[min(e + u, (int64_t)last)];
      }
#pragma unroll
      for (int u = 0; u < kRound; ++u) idx_n[u] = col[min(e + kRound + u, (int64_t)last)];
#pragma unroll
      for (int u = 0; u < kRound; ++u) {
        p[u] = dot4(g, v[u]);
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) p[u] += __shfl_xor(p[u], off, G);
      }
      if (gl == 0) {
#pragma unroll
        for (int u = 0; u < kRound; ++u)
          if (e + u < it.end) out[e + u] = p[u];
      }
      if (SUMS) {
#pragma unroll
        for (int u = 0; u < kRound; ++u) {
          part[u] += e + u < it.end ? (LOGW ? logw_term(wp[u], p[u]) : p[u]) : 0.f;
          if (e == it.begin) first[u] = p[u];
          if (LOGW && e == it.begin) first_w[u] = wp[u];
        }
      }
    }
    if (finish && gl == 0) {                                // every lane holds every dot: lane 0 stored them all
      const float sum = ((part[0] + part[4]) + (part[2] + part[6])) + ((part[1] + part[5]) + (part[3] + part[7]));
      const float sw = seg_total<MODE>(sum, w);
#pragma unroll
      for (int u = 0; u < kRound; ++u)
        if ((int64_t)it.begin + u < it.end) out[it.begin + u] = seg_value<MODE>(first[u], sw, first_w[u]);
      for (int64_t e = (int64_t)it.begin + kRound; e < it.end; e += kRound) {
        float later[kRound], later_w[kRound];
#pragma unroll
        for (int u = 0; u < kRound; ++u) {
          later[u] = out[min(e + u, (int64_t)last)];
          later_w[u] = LOGW ? cnt[min(e + u, (int64_t)last)] : w;
        }
#pragma unroll
        for (int u = 0; u < kRound; ++u)
          if (e + u < it.end) out[e + u] = seg_value<MODE>(later[u], sw, later_w[u]);
      }
    }
  }
}

// The segments of more than 64 edges of a mean structure (kMean, cnt = cnt[N * R]) or of a weighted one (kLogW, cnt =
// w[E]), in place over the dots k_edge_dot stored in that mode (it has finished the shorter ones).  A workgroup looks at
// 256 segments, one per thread, and then takes the long ones among them one at a time with all its threads: thread t
// adds dot[begin + t + 256 j] (kLogW: fl(w * dot) of that position) for j = 0, 1, ... in ascending j onto +0.0f; the 64 sums of a wavefront meet in an xor butterfly (32, 16, 8, 4, 2, 1); S = ((W0 + W1) + W2) + W3 over the
// four wavefronts.  Each position is then re-read and rewritten by the thread that summed it.
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_edge_long(const int32_t* __restrict__ rowptr,
                                                        const float* __restrict__ cnt, int64_t NR, float* out) {
  constexpr bool LOGW = MODE == kLogW;
  constexpr int kBatch = 8;                       // loads in flight per thread
  __shared__ int list[kThreads];
  __shared__ int nlist;
  __shared__ float wsum[kThreads / 64];
  const int tid = (int)threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kThreads;
  if (tid == 0) nlist = 0;
  __syncthreads();
  if (base + tid < NR && rowptr[base + tid + 1] - rowptr[base + tid] > RGCN_CHUNK) list[atomicAdd(&nlist, 1)] = tid;
  __syncthreads();
  const int n = nlist;                            // (the order of the list changes no value: a segment is summed alone)
  for (int i = 0; i < n; ++i) {
    const int64_t s = base + list[i];
    const int64_t begin = rowptr[s], end = rowptr[s + 1];
    float w = 0.f;
    if constexpr (!LOGW) w = mean_weight(cnt[s]);
    float sum = 0.f;
    int64_t p = begin + tid;
    for (; p + (kBatch - 1) * kThreads < end; p += kBatch * kThreads) {
      float v[kBatch], wv[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        v[j] = out[p + j * kThreads];
        if constexpr (LOGW) wv[j] = cnt[p + j * kThreads];
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) sum += LOGW ? logw_term(wv[j], v[j]) : v[j];
    }
    for (; p < end; p += kThreads) sum += LOGW ? logw_term(cnt[p], out[p]) : out[p];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;
    __syncthreads();
    const float sw = seg_total<MODE>(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3], w);
    p = begin + tid;
    for (; p + (kBatch - 1) * kThreads < end; p += kBatch * kThreads) {
      float v[kBatch], wv[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) {
        v[j] = out[p + j * kThreads];
        wv[j] = LOGW ? cnt[p + j * kThreads] : w;
      }
#pragma unroll
      for (int j = 0; j < kBatch; ++j) out[p + j * kThreads] = seg_value<MODE>(v[j], sw, wv[j]);
    }
    for (; p < end; p += kThreads) out[p] = seg_value<MODE>(out[p], sw, LOGW ? cnt[p] : w);
    __syncthreads();                              // wsum is free again
  }
}

// out[s] for every s < NR (the header's RGCN_MODE_EDGE_SUM): nothing but perm, rowptr and the values is read
__global__ __launch_bounds__(kThreads) void k_edge_sum(const int32_t* __restrict__ rowptr, const int64_t* __restrict__ perm,
                                                       int64_t NR, int64_t E, const float* __restrict__ x,
                                                       float* __restrict__ out) {
  constexpr int kBatch = 8;
  __shared__ int list[kThreads];
  __shared__ int nlist;
  __shared__ float wsum[kThreads / 64];
  const int tid = (int)threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * kThreads, s_own = base + tid;
  if (tid == 0) nlist = 0;
  __syncthreads();
  int64_t begin = 0, end = 0;
  if (s_own < NR) { begin = rowptr[s_own]; end = rowptr[s_own + 1]; }
  const bool is_long = end - begin > RGCN_CHUNK;
  if (is_long) list[atomicAdd(&nlist, 1)] = tid;
  if (!is_long && s_own < NR) {
    float part[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; ++j) part[j] = 0.f;
    const int64_t last = end > begin ? end - 1 : 0;
    for (int64_t q = begin; q < end; q += kBatch) {
      int64_t e[kBatch];
      float v[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) e[j] = clamp64(perm[min(q + j, last)], 0, E - 1);   // clamped: never under a branch
#pragma unroll
      for (int j = 0; j < kBatch; ++j) v[j] = x[e[j]];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) part[j] += q + j < end ? v[j] : 0.f;
    }
    out[s_own] = ((part[0] + part[4]) + (part[2] + part[6])) + ((part[1] + part[5]) + (part[3] + part[7]));
  }
  __syncthreads();
  const int n = nlist;                            // (the order of the list changes no value: a segment is summed alone)
  for (int i = 0; i < n; ++i) {
    const int64_t s = base + list[i];
    const int64_t b = rowptr[s], en = rowptr[s + 1];
    float sum = 0.f;
    for (int64_t q = b + tid; q < en; q += (int64_t)kBatch * kThreads) {   // ascending j: thread t adds b + t + 256 j
      int64_t e[kBatch];
      float v[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) e[j] = clamp64(perm[min(q + (int64_t)j * kThreads, en - 1)], 0, E - 1);
#pragma unroll
      for (int j = 0; j < kBatch; ++j) v[j] = x[e[j]];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) sum += q + (int64_t)j * kThreads < en ? v[j] : 0.f;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) out[s] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    __syncthreads();                              // wsum is free again
  }
}

template <int G>
void launch_dot(const rgcn_csr* c, int64_t NR, int what, const float* x, const float* gagg, float* out, int d,
                hipStream_t stream) {
  const int64_t nitems = c->num_items[0] - c->empty_items0;       // the segments without an edge are the suffix
  if (nitems <= 0) return;
  const unsigned grid = (unsigned)ceil_div64(nitems, kThreads / G);
  if (what == kMean)
    k_edge_dot<G, kMean><<<grid, kThreads, 0, stream>>>(x, gagg, c->items[0], nitems, c->rowptr, NR, c->col, c->head_col,
                                                        c->val, out, d);
  else if (what == kLogW)
    k_edge_dot<G, kLogW><<<grid, kThreads, 0, stream>>>(x, gagg, c->items[0], nitems, c->rowptr, NR, c->col, c->head_col,
                                                        c->val, out, d);
  else
    k_edge_dot<G, kPlain><<<grid, kThreads, 0, stream>>>(x, gagg, c->items[0], nitems, c->rowptr, NR, c->col, c->head_col,
                                                         nullptr, out, d);
}

}  // namespace

int rgcn_edge_grad(const rgcn_graph* g, int transposed, const void* x, int mode, int64_t d, const float* gagg,
                   void* out, size_t out_bytes, int first_level, int last_level, const rgcn_slab_job* job,
                   const float* amax, void* stream_) {
  const rgcn_csr* c = &g->dir[transposed ? 1 : 0];
  if ((mode & 1) || (mode & RGCN_MODE_SPARSE_ROWS)) return RGCN_ERR_UNSUPPORTED;
  if (d <= 0 || (d & 3)) return RGCN_ERR_ARG;
  if (d > 256) return RGCN_ERR_UNSUPPORTED;       // the dot would span column blocks
  if (amax) return RGCN_ERR_UNSUPPORTED;
  if (job && job->slab) return RGCN_ERR_UNSUPPORTED;   // a pending reduction must not be lost silently
  if (!c->rowptr) return RGCN_ERR_ARG;            // direction not built
  if (first_level != 0 || (last_level >= 0 && last_level != c->num_levels)) return RGCN_ERR_ARG;
  const bool mean = (mode & RGCN_MODE_MEAN_GRAD) != 0, logw = (mode & RGCN_MODE_LOG_WEIGHT_GRAD) != 0;
  if (mean && c->weighted) return RGCN_ERR_UNSUPPORTED;
  if (logw && !c->weighted) return RGCN_ERR_UNSUPPORTED;   // a mean structure has no per-edge weights: the mean mode
  const int what = mean ? kMean : logw ? kLogW : kPlain;
  if (g->E == 0 || c->n_key == 0) return RGCN_OK; // nothing to write
  if (!x || !gagg) return RGCN_ERR_ARG;
  if (!out || out_bytes < (size_t)g->E * sizeof(float)) return RGCN_ERR_WORKSPACE;
  RGCN_ALIGN_TRY(16, x, gagg, out);
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t NR = c->n_key * g->R;
  const float* xf = reinterpret_cast<const float*>(x);
  float* o = reinterpret_cast<float*>(out);
  const int q = (int)(d / 4);
  if (q <= 1) launch_dot<1>(c, NR, what, xf, gagg, o, (int)d, stream);
  else if (q <= 2) launch_dot<2>(c, NR, what, xf, gagg, o, (int)d, stream);
  else if (q <= 4) launch_dot<4>(c, NR, what, xf, gagg, o, (int)d, stream);
  else if (q <= 8) launch_dot<8>(c, NR, what, xf, gagg, o, (int)d, stream);
  else if (q <= 16) launch_dot<16>(c, NR, what, xf, gagg, o, (int)d, stream);
  else if (q <= 32) launch_dot<32>(c, NR, what, xf, gagg, o, (int)d, stream);
  else launch_dot<64>(c, NR, what, xf, gagg, o, (int)d, stream);
  if (mean)                                       // the segments of more than 64 edges, if there are any
    k_edge_long<kMean><<<(unsigned)ceil_div64(NR, kThreads), kThreads, 0, stream>>>(c->rowptr, c->val, NR, o);
  else if (logw)
    k_edge_long<kLogW><<<(unsigned)ceil_div64(NR, kThreads), kThreads, 0, stream>>>(c->rowptr, c->val, NR, o);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

int rgcn_edge_sum(const rgcn_graph* g, int transposed, const void* x, int mode, int64_t d, float* out, int first_level,
                  int last_level, const rgcn_slab_job* job, const float* amax, void* stream_) {
  const rgcn_csr* c = &g->dir[transposed ? 1 : 0];
  if (mode != RGCN_MODE_EDGE_SUM) return RGCN_ERR_ARG;   // the call is no gather and no dot: no other bit has a meaning
  if (d != 1) return RGCN_ERR_ARG;
  if (amax) return RGCN_ERR_UNSUPPORTED;
  if (job && job->slab) return RGCN_ERR_UNSUPPORTED;   // a pending reduction must not be lost silently
  if (!c->rowptr || !c->perm) return RGCN_ERR_ARG;     // direction not built
  if (first_level != 0 || (last_level >= 0 && last_level != c->num_levels)) return RGCN_ERR_ARG;
  const int64_t NR = c->n_key * g->R;
  if (NR == 0) return RGCN_OK;                    // nothing to write
  if (!out || (g->E > 0 && !x)) return RGCN_ERR_ARG;   // (without an edge x is never read: zeros)
  RGCN_ALIGN_TRY(4, x, out);
  k_edge_sum<<<(unsigned)ceil_div64(NR, kThreads), kThreads, 0, (hipStream_t)stream_>>>(
      c->rowptr, c->perm, NR, g->E, reinterpret_cast<const float*>(x), out);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}
