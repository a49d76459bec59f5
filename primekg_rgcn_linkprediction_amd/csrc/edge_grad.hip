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

template <int G, bool MEAN>
__global__ __launch_bounds__(kThreads) void k_edge_dot(
    const float* __restrict__ x, const float* __restrict__ gagg, const rgcn_item* __restrict__ items, int64_t nitems,
    const int32_t* __restrict__ rowptr, int64_t NR, const int32_t* __restrict__ col,
    const int32_t* __restrict__ head_col, const float* __restrict__ cnt, float* out, int d) {
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
  const bool finish = MEAN && !(it.flags & RGCN_ITEM_PACK);
  float w = 0.f;
  if (finish) w = mean_weight(cnt[seg]);

  if constexpr (G >= kRound) {
    // ids: lane u < 8 of the group holds the id of edge e + u; the first round's come with the item (padded with -1),
    // a later round's are loaded one round ahead from a clamped position - never under a branch
    int cur = head_col[item_id * kRound + (gl & (kRound - 1))];
    const int slot = gl / (G / kRound);           // the top three lane bits, read as a number: the edge of a round
    const bool stores = gl % (G / kRound) == 0;
    float part = 0.f, first = 0.f;                // mean: this slot's partial sum; the first round's dot
    for (int64_t e = it.begin; e < it.end; e += kRound) {       // int64: a run may end within a round of 2^31
      const int nxt = col[min(e + kRound + (gl & (kRound - 1)), (int64_t)last)];
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
      if (MEAN) {
        part += mine < it.end ? p[0] : 0.f;
        if (e == it.begin) first = p[0];
      }
    }
    if (finish) {
      // ((P0 + P4) + (P2 + P6)) + ((P1 + P5) + (P3 + P7)): the slots differ in the top three lane bits
      float sum = part;
#pragma unroll
      for (int off = G / 2; off >= G / kRound; off >>= 1) sum += __shfl_xor(sum, off, G);
      const float sw = mean_scaled_sum(sum, w);
      const int64_t mine = (int64_t)it.begin + slot;
      if (stores && mine < it.end) out[mine] = mean_value(first, sw, w);
      if (stores && it.end - it.begin > kRound) {             // later rounds: this lane's own stores, re-read in one batch
        float later[kRound - 1];
#pragma unroll
        for (int r = 1; r < kRound; ++r) later[r - 1] = out[min(mine + r * kRound, (int64_t)last)];
#pragma unroll
        for (int r = 1; r < kRound; ++r)
          if (mine + r * kRound < it.end) out[mine + r * kRound] = mean_value(later[r - 1], sw, w);
      }
    }
  } else {
    int idx_n[kRound];                                      // fewer than 8 lanes per row: every lane loads the ids
    float part[kRound], first[kRound];
#pragma unroll
    for (int u = 0; u < kRound; ++u) {
      idx_n[u] = col[min((int64_t)it.begin + u, (int64_t)last)];
      part[u] = first[u] = 0.f;
    }
    for (int64_t e = it.begin; e < it.end; e += kRound) {
      float p[kRound];
      float4 v[kRound];
#pragma unroll
      for (int u = 0; u < kRound; ++u) v[u] = *reinterpret_cast<const float4*>(x + (size_t)idx_n[u] * d + c4);
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
      if (MEAN) {
#pragma unroll
        for (int u = 0; u < kRound; ++u) {
          part[u] += e + u < it.end ? p[u] : 0.f;
          if (e == it.begin) first[u] = p[u];
        }
      }
    }
    if (finish && gl == 0) {                                // every lane holds every dot: lane 0 stored them all
      const float sum = ((part[0] + part[4]) + (part[2] + part[6])) + ((part[1] + part[5]) + (part[3] + part[7]));
      const float sw = mean_scaled_sum(sum, w);
#pragma unroll
      for (int u = 0; u < kRound; ++u)
        if ((int64_t)it.begin + u < it.end) out[it.begin + u] = mean_value(first[u], sw, w);
      for (int64_t e = (int64_t)it.begin + kRound; e < it.end; e += kRound) {
        float later[kRound];
#pragma unroll
        for (int u = 0; u < kRound; ++u) later[u] = out[min(e + u, (int64_t)last)];
#pragma unroll
        for (int u = 0; u < kRound; ++u)
          if (e + u < it.end) out[e + u] = mean_value(later[u], sw, w);
      }
    }
  }
}

// The segments of more than 64 edges of a mean structure, in place over the dots k_edge_dot<., true> stored (it has
// finished the shorter ones).  A workgroup looks at 256 segments, one per thread, and then takes the long ones among
// them one at a time with all its threads: thread t adds dot[begin + t + 256 j] for j = 0, 1, ... in ascending j onto
// +0.0f; the 64 sums of a wavefront meet in an xor butterfly (32, 16, 8, 4, 2, 1); S = ((W0 + W1) + W2) + W3 over the
// four wavefronts.  Each position is then re-read and rewritten by the thread that summed it.
__global__ __launch_bounds__(kThreads) void k_edge_mean_long(const int32_t* __restrict__ rowptr,
                                                             const float* __restrict__ cnt, int64_t NR, float* out) {
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
    const float w = mean_weight(cnt[s]);
    float sum = 0.f;
    int64_t p = begin + tid;
    for (; p + (kBatch - 1) * kThreads < end; p += kBatch * kThreads) {
      float v[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) v[j] = out[p + j * kThreads];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) sum += v[j];
    }
    for (; p < end; p += kThreads) sum += out[p];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = sum;
    __syncthreads();
    const float sw = mean_scaled_sum(((wsum[0] + wsum[1]) + wsum[2]) + wsum[3], w);
    p = begin + tid;
    for (; p + (kBatch - 1) * kThreads < end; p += kBatch * kThreads) {
      float v[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) v[j] = out[p + j * kThreads];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) out[p + j * kThreads] = mean_value(v[j], sw, w);
    }
    for (; p < end; p += kThreads) out[p] = mean_value(out[p], sw, w);
    __syncthreads();                              // wsum is free again
  }
}

template <int G>
void launch_dot(const rgcn_csr* c, int64_t NR, bool mean, const float* x, const float* gagg, float* out, int d,
                hipStream_t stream) {
  const int64_t nitems = c->num_items[0] - c->empty_items0;       // the segments without an edge are the suffix
  if (nitems <= 0) return;
  const unsigned grid = (unsigned)ceil_div64(nitems, kThreads / G);
  if (mean)
    k_edge_dot<G, true><<<grid, kThreads, 0, stream>>>(x, gagg, c->items[0], nitems, c->rowptr, NR, c->col, c->head_col,
                                                       c->val, out, d);
  else
    k_edge_dot<G, false><<<grid, kThreads, 0, stream>>>(x, gagg, c->items[0], nitems, c->rowptr, NR, c->col, c->head_col,
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
  const bool mean = (mode & RGCN_MODE_MEAN_GRAD) != 0;
  if (mean && c->weighted) return RGCN_ERR_UNSUPPORTED;
  if (g->E == 0 || c->n_key == 0) return RGCN_OK; // nothing to write
  if (!x || !gagg) return RGCN_ERR_ARG;
  if (!out || out_bytes < (size_t)g->E * sizeof(float)) return RGCN_ERR_WORKSPACE;
  RGCN_ALIGN_TRY(16, x, gagg, out);
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t NR = c->n_key * g->R;
  const float* xf = reinterpret_cast<const float*>(x);
  float* o = reinterpret_cast<float*>(out);
  const int q = (int)(d / 4);
  if (q <= 1) launch_dot<1>(c, NR, mean, xf, gagg, o, (int)d, stream);
  else if (q <= 2) launch_dot<2>(c, NR, mean, xf, gagg, o, (int)d, stream);
  else if (q <= 4) launch_dot<4>(c, NR, mean, xf, gagg, o, (int)d, stream);
  else if (q <= 8) launch_dot<8>(c, NR, mean, xf, gagg, o, (int)d, stream);
  else if (q <= 16) launch_dot<16>(c, NR, mean, xf, gagg, o, (int)d, stream);
  else if (q <= 32) launch_dot<32>(c, NR, mean, xf, gagg, o, (int)d, stream);
  else launch_dot<64>(c, NR, mean, xf, gagg, o, (int)d, stream);
  if (mean)                                       // the segments of more than 64 edges, if there are any
    k_edge_mean_long<<<(unsigned)ceil_div64(NR, kThreads), kThreads, 0, stream>>>(c->rowptr, c->val, NR, o);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}
