// Score-ranked connecting paths between node pairs (include/rgcn_paths.h): what the reference's analysis scripts do
// with networkx.all_simple_paths(cutoff=4) + score_path + rank_paths (explain_predictions.py:255-352,
// case_studies.py:319-351, analyze_failures.py:345-366), exhaustively and on the device.
//
//   k_edge_cosine   8 lanes per unique edge (u, v): cos(x_u, x_v) in fp32; the source u of out-entry e is found by
//                   the fan-out search in out_ptr.
//   k_paths_select  grid (Q, S), 4 waves per workgroup: the G = 4 S waves of a query divide its work into units
//                     L = 1  one search for t in out(s)                                    wave 0
//                     L = 2  64-entry chunk c of out(s)                                    wave c mod G
//                     L = 3  first hop a = out(s)[i]: the walk of out(a)                   wave i mod G
//                     L = 4  prefix (a = out(s)[i], b = out(a)[j]): the walk of out(b)     wave (i + j) mod G
//                   so a hub first hop is spread over ALL waves of the query (no prefix sum needed: the unit's owner
//                   follows from its two positions).  A walk takes 64 entries at a time, one per lane: the lane's
//                   node must differ from the path's earlier nodes and from t (4 compares) and be in in(t) - a
//                   fan-out search of in(t)'s ids, staged in LDS with their edge scores when in(t) has at most
//                   kLdsIds entries, read from global memory otherwise.  When a staged in(t) is much the shorter
//                   list the lanes walk IT and search out(.) instead.  Hits are counted by a ballot (a 64-bit
//                   per-wave sum, one atomic per wave and length at the end: integer, so order-free) and the ones that
//                   beat the wave's current k-th entry are inserted, one after the other, into the wave's sorted
//                   list, which lives in REGISTERS: lane i holds entry i (k <= 64), an insertion is a ballot for the
//                   position and one lane shift.  The comparison is the full total order (rgcn_paths_order.h): paths
//                   arrive in no particular order here, so "earlier stays in front" would not be a rule.
//   k_paths_merge   one wave per query: the 4 S lists of the query through the same insertion -> the output rows.
#include <math.h>

#include <algorithm>

#include "rgcn_common.h"
#include "../../include/rgcn_paths.h"
#include "rgcn_paths_order.h"
#include "rgcn_sorted_search.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kLdsIds = 2048;      // entries of in(t) a workgroup stages (ids + scores: 16 KB of LDS)
constexpr int kMaxSlices = 256;
constexpr int kFill = 64 * 256;    // workgroups the automatic slice rule aims for.  Far more than are resident at once: a
                                   // query's work is as skewed as its source's degree (one hub source of 100 queries took
                                   // 5.3 of the batch's 5.5 ms at 11 slices), and many short workgroups even that out
constexpr int kEdgeLanes = 8;      // lanes that share one edge of k_edge_cosine

static_assert(sizeof(rgcn_path_entry) == 20, "workspace layout");

__global__ __launch_bounds__(kThreads) void k_edge_cosine(const float* __restrict__ emb, int N, int d,
                                                          const int64_t* __restrict__ out_ptr,
                                                          const int32_t* __restrict__ out_dst, int64_t nnz,
                                                          float* __restrict__ edge_score) {
  const int tid = threadIdx.x, sub = tid & (kEdgeLanes - 1);
  const int64_t e = ((int64_t)blockIdx.x * kThreads + tid) / kEdgeLanes;
  const bool live = e < nnz;
  const int64_t ee = live ? e : nnz - 1;                       // idle groups of the last block redo the last edge
  // the source: the last u with out_ptr[u] <= e (its row is not empty: out_ptr[u + 1] > e)
  int64_t u = rgcn_lower_bound(out_ptr, 0, (int64_t)N + 1, ee + 1) - 1;
  u = u < 0 ? 0 : (u > N - 1 ? N - 1 : u);
  int v = out_dst[ee];
  const bool ok = (unsigned)v < (unsigned)N;
  if (!ok) v = 0;
  const float4* xu = reinterpret_cast<const float4*>(emb + (size_t)u * d);
  const float4* xv = reinterpret_cast<const float4*>(emb + (size_t)v * d);
  float dot = 0.f, nu = 0.f, nv = 0.f;
  for (int i = sub; i < d / 4; i += kEdgeLanes) {
    const float4 a = xu[i], b = xv[i];
    dot = fmaf(a.x, b.x, dot); dot = fmaf(a.y, b.y, dot); dot = fmaf(a.z, b.z, dot); dot = fmaf(a.w, b.w, dot);
    nu = fmaf(a.x, a.x, nu); nu = fmaf(a.y, a.y, nu); nu = fmaf(a.z, a.z, nu); nu = fmaf(a.w, a.w, nu);
    nv = fmaf(b.x, b.x, nv); nv = fmaf(b.y, b.y, nv); nv = fmaf(b.z, b.z, nv); nv = fmaf(b.w, b.w, nv);
  }
#pragma unroll
  for (int o = kEdgeLanes / 2; o > 0; o >>= 1) {
    dot += __shfl_xor(dot, o);
    nu += __shfl_xor(nu, o);
    nv += __shfl_xor(nv, o);
  }
  if (live && sub == 0) {
    const float den = sqrtf(nu) * sqrtf(nv);
    edge_score[e] = (!ok || den == 0.f) ? 0.f : dot / den;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// a wave's sorted list, in registers
struct WaveList {
  rgcn_path_entry mine;   // lane i: entry i, meaningful for i < cnt
  rgcn_path_entry thr;    // wave-uniform: entry k - 1 once the list is full
  int cnt;                // wave-uniform
};

__device__ inline rgcn_path_entry empty_entry() {
  rgcn_path_entry e;
  e.score = -INFINITY;
  e.len = 0;
  e.n1 = e.n2 = e.n3 = -1;
  return e;
}

__device__ inline rgcn_path_entry entry_of_lane(const rgcn_path_entry& e, int src) {
  rgcn_path_entry r;
  r.score = __shfl(e.score, src);
  r.len = __shfl(e.len, src);
  r.n1 = __shfl(e.n1, src);
  r.n2 = __shfl(e.n2, src);
  r.n3 = __shfl(e.n3, src);
  return r;
}

// c is the same in every lane and its score is not NaN
__device__ inline void list_insert(WaveList& l, int k, int lane, const rgcn_path_entry& c) {
  if (l.cnt == k && !rgcn_path_before(c, l.thr)) return;
  const bool front = lane < l.cnt && rgcn_path_before(l.mine, c);
  const int p = __popcll(__ballot(front));                     // the list is sorted: the entries in front of c are the first p; p < k
  rgcn_path_entry up;
  up.score = __shfl_up(l.mine.score, 1);
  up.len = __shfl_up(l.mine.len, 1);
  up.n1 = __shfl_up(l.mine.n1, 1);
  up.n2 = __shfl_up(l.mine.n2, 1);
  up.n3 = __shfl_up(l.mine.n3, 1);
  if (lane > p) l.mine = up;
  else if (lane == p) l.mine = c;
  if (l.cnt < k) ++l.cnt;
  if (l.cnt == k) l.thr = entry_of_lane(l.mine, k - 1);
}

// every lane with `has` offers its own entry; the ones that cannot enter the list are dropped by one ballot
__device__ inline void list_offer(WaveList& l, int k, int lane, bool has, const rgcn_path_entry& c) {
  unsigned long long m = __ballot(has && c.score == c.score && (l.cnt < k || rgcn_path_before(c, l.thr)));
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    list_insert(l, k, lane, entry_of_lane(c, src));
  }
}

struct PathWeights {
  float w[RGCN_PATHS_MAX_LEN + 1];
};

__global__ __launch_bounds__(kThreads) void k_paths_select(
    const int64_t* __restrict__ out_ptr, const int32_t* __restrict__ out_dst, const float* __restrict__ edge_score,
    const int64_t* __restrict__ in_ptr, const int32_t* __restrict__ in_src, const int64_t* __restrict__ in_pos, int N,
    int64_t nnz, const int64_t* __restrict__ sources, const int64_t* __restrict__ targets, int max_len, int k,
    PathWeights pw, rgcn_path_entry* __restrict__ ws, unsigned long long* __restrict__ count) {
  __shared__ int32_t s_ids[kLdsIds];
  __shared__ float s_sc[kLdsIds];
  const int q = blockIdx.x, S = gridDim.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = blockIdx.y * kWaves + wave, G = S * kWaves;

  WaveList l;
  l.mine = l.thr = empty_entry();
  l.cnt = 0;
  unsigned long long found1 = 0, found2 = 0, found3 = 0, found4 = 0;   // wave-uniform

  const int64_t s64 = sources[q], t64 = targets[q];
  int ds = 0, m = 0;
  int64_t ps = 0, ib = 0;
  if (s64 >= 0 && s64 < N && t64 >= 0 && t64 < N && s64 != t64) {      // the same in every thread of the workgroup
    ps = clamp64(out_ptr[s64], 0, nnz);
    ds = (int)(clamp64(out_ptr[s64 + 1], ps, nnz) - ps);
    ib = clamp64(in_ptr[t64], 0, nnz);
    m = (int)(clamp64(in_ptr[t64 + 1], ib, nnz) - ib);
  }
  if (ds > 0 && m > 0) {                                               // workgroup-uniform
    const int s = (int)s64, t = (int)t64;
    const bool staged = m <= kLdsIds;
    if (staged) {
      for (int i = tid; i < m; i += kThreads) {
        s_ids[i] = in_src[ib + i];
        s_sc[i] = edge_score[clamp64(in_pos[ib + i], 0, nnz - 1)];
      }
      __syncthreads();
    }
    const int32_t* g_ids = in_src + ib;
    // is c -> t an edge?  its score
    auto closes = [&](int c, float& sc) -> bool {
      if (staged) {
        const int j = rgcn_lower_bound(s_ids, 0, m, c);
        const int jj = j < m ? j : m - 1;
        sc = s_sc[jj];
        return j < m && s_ids[jj] == c;
      }
      const int j = rgcn_lower_bound(g_ids, 0, m, c);
      const int jj = j < m ? j : m - 1;
      if (g_ids[jj] != c || j >= m) return false;
      sc = edge_score[clamp64(in_pos[ib + jj], 0, nnz - 1)];
      return true;
    };
    // One path candidate per lane -> the wave's counts and list.  c: the lane's last interior node of a path of L edges
    // whose earlier interior nodes are n1, n2 (-1: none); its hops: `pre` (the sum so far, L > 2), cw, then cc into t.
    auto offer = [&](bool hit, int c, int L, float pre, float cw, float cc, int n1, int n2, unsigned long long& found) {
      rgcn_path_entry cand;
      cand.score = __fmul_rn(__fadd_rn(L > 2 ? __fadd_rn(pre, cw) : cw, cc), pw.w[L]);
      cand.len = L;
      cand.n1 = L == 2 ? c : n1;
      cand.n2 = L == 3 ? c : (L == 4 ? n2 : -1);
      cand.n3 = L == 4 ? c : -1;
      found += (unsigned long long)__popcll(__ballot(hit));
      list_offer(l, k, lane, hit, cand);
    };
    // The intersection of out-entries [b, e) with in(t), by the wave.  The lanes walk one list, 64 entries a step,
    // and search the other: out(.) against in(t) as a rule; a staged in(t) against a long out(.) in global memory when
    // that takes fewer steps, a step of the second kind costing about four dependent rounds (8-way search of <= 2^12
    // entries and the score) against one.
    auto walk = [&](int64_t b, int64_t e, int L, float pre, int n1, int n2, unsigned long long& found) {
      const int64_t len = e - b;
      if (staged && len <= INT32_MAX && 4 * ((m + 63) / 64) < (len + 63) / 64) {
        const int32_t* outs = out_dst + b;
        for (int base = 0; base < m; base += 64) {
          const int j = base + lane;
          const bool in = j < m;
          const int c = in ? s_ids[j] : -1;
          const float cc = in ? s_sc[j] : 0.f;
          bool hit = in && c != s && c != t && c != n1 && c != n2;
          float cw = 0.f;
          if (hit) {
            const int at = rgcn_lower_bound(outs, 0, (int)len, c);
            const int aa = at < (int)len ? at : (int)len - 1;
            hit = at < (int)len && outs[aa] == c;
            cw = edge_score[b + aa];
          }
          offer(hit, c, L, pre, cw, cc, n1, n2, found);
        }
        return;
      }
      for (int64_t base = b; base < e; base += 64) {
        const int64_t i = base + lane;
        const bool in = i < e;
        int c = -1;
        float cw = 0.f, cc = 0.f;
        if (in) {
          c = out_dst[i];
          cw = edge_score[i];
        }
        bool hit = in && (unsigned)c < (unsigned)N && c != s && c != t && c != n1 && c != n2;
        if (hit) hit = closes(c, cc);
        offer(hit, c, L, pre, cw, cc, n1, n2, found);
      }
    };

    // L = 1
    if (g == 0) {
      const int j = rgcn_lower_bound(out_dst + ps, 0, ds, t);
      if (j < ds && out_dst[ps + j] == t) {
        rgcn_path_entry cand = empty_entry();
        cand.score = __fmul_rn(edge_score[ps + j], pw.w[1]);
        cand.len = 1;
        found1 = 1;
        if (cand.score == cand.score) list_insert(l, k, lane, cand);
      }
    }
    // L = 2: out(s) against in(t)
    if (max_len >= 2) {
      for (int64_t ch = g; ch * 64 < ds; ch += G)
        walk(ps + ch * 64, ps + (ch * 64 + 64 < ds ? ch * 64 + 64 : ds), 2, 0.f, -1, -1, found2);
    }
    // L = 3: this wave's first hops, 64 at a time in the lanes, then one walk each
    if (max_len >= 3) {
      for (int64_t base = 0; g + base * G < ds; base += 64) {
        const int64_t ia = g + (base + lane) * G;
        int a = -1;
        float c1 = 0.f;
        int64_t pa = 0, pe = 0;
        if (ia < ds) {
          a = out_dst[ps + ia];
          c1 = edge_score[ps + ia];
          if ((unsigned)a < (unsigned)N && a != s && a != t) {
            pa = clamp64(out_ptr[a], 0, nnz);
            pe = clamp64(out_ptr[a + 1], pa, nnz);
          }
        }
        unsigned long long todo = __ballot(pe > pa);
        while (todo) {
          const int src = __ffsll((long long)todo) - 1;
          todo &= todo - 1;
          walk(lane_i64(pa, src), lane_i64(pe, src), 3, lane_float(c1, src), lane_int(a, src), -1, found3);
        }
      }
    }
    // L = 4: every first hop in the lanes, 64 at a time; lane's prefixes (a, out(a)[j]) are the j with
    // (i + j) mod G == g
    if (max_len >= 4) {
      for (int64_t base = 0; base < ds; base += 64) {
        const int64_t ia = base + lane;
        int a = -1;
        float c1 = 0.f;
        int64_t pa = 0, da = 0, j = 0;
        if (ia < ds) {
          a = out_dst[ps + ia];
          c1 = edge_score[ps + ia];
          if ((unsigned)a < (unsigned)N && a != s && a != t) {
            pa = clamp64(out_ptr[a], 0, nnz);
            da = clamp64(out_ptr[a + 1], pa, nnz) - pa;
            j = (int64_t)((g - (int)(ia % G) + G) % G);
          }
        }
        while (__ballot(j < da)) {
          int b = -1;
          float c2 = 0.f;
          int64_t pb = 0, pe = 0;
          if (j < da) {
            b = out_dst[pa + j];
            c2 = edge_score[pa + j];
            if ((unsigned)b < (unsigned)N && b != s && b != t && b != a) {
              pb = clamp64(out_ptr[b], 0, nnz);
              pe = clamp64(out_ptr[b + 1], pb, nnz);
            }
          }
          unsigned long long todo = __ballot(pe > pb);
          while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const float pre = __fadd_rn(lane_float(c1, src), lane_float(c2, src));
            walk(lane_i64(pb, src), lane_i64(pe, src), 4, pre, lane_int(a, src), lane_int(b, src), found4);
          }
          j += G;
        }
      }
    }
  }

  // this wave's list -> workspace [Q][S][waves][k]
  if (lane < k) ws[(((size_t)q * S + blockIdx.y) * kWaves + wave) * k + lane] = lane < l.cnt ? l.mine : empty_entry();
  if (lane == 0) {
    unsigned long long* cq = count + (size_t)q * RGCN_PATHS_MAX_LEN;
    if (found1) atomicAdd(cq + 0, found1);
    if (found2) atomicAdd(cq + 1, found2);
    if (found3) atomicAdd(cq + 2, found3);
    if (found4) atomicAdd(cq + 3, found4);
  }
}

// One wave per query: all entries of the query's lists through the same insertion.  The lists are sorted, so once the
// output is full almost every 64-entry load is dropped by the one ballot of list_offer.
__global__ __launch_bounds__(64) void k_paths_merge(const rgcn_path_entry* __restrict__ ws, int per_query, int k,
                                                    const int64_t* __restrict__ sources,
                                                    const int64_t* __restrict__ targets, int32_t* __restrict__ nodes,
                                                    int32_t* __restrict__ length, float* __restrict__ score) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const rgcn_path_entry* mine = ws + (size_t)q * per_query;
  WaveList l;
  l.mine = l.thr = empty_entry();
  l.cnt = 0;
  for (int base = 0; base < per_query; base += 64) {
    const int i = base + lane;
    rgcn_path_entry e = empty_entry();
    if (i < per_query) e = mine[i];
    list_offer(l, k, lane, e.len > 0, e);
  }
  if (lane < k) {
    const bool has = lane < l.cnt;
    const rgcn_path_entry e = has ? l.mine : empty_entry();
    const int s = (int)sources[q], t = (int)targets[q], L = e.len;
    int32_t* row = nodes + ((size_t)q * k + lane) * RGCN_PATHS_NODES;
    row[0] = has ? s : -1;
    row[1] = !has ? -1 : (L == 1 ? t : e.n1);
    row[2] = !has ? -1 : (L == 2 ? t : (L > 2 ? e.n2 : -1));
    row[3] = !has ? -1 : (L == 3 ? t : (L > 3 ? e.n3 : -1));
    row[4] = !has ? -1 : (L == 4 ? t : -1);
    length[(size_t)q * k + lane] = L;
    score[(size_t)q * k + lane] = e.score;
  }
}

// workgroups per query: as asked, or enough to fill the device when the batch is small; at most kMaxSlices
inline int plan_slices(int64_t num_queries, int slices) {
  int64_t want = slices > 0 ? slices : ceil_div64(kFill, num_queries);
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, kMaxSlices));
}

}  // namespace

extern "C" {

int rgcn_edge_cosine(const float* emb, int64_t num_nodes, int d, const int64_t* out_ptr, const int32_t* out_dst,
                     int64_t nnz, float* edge_score, void* stream_) {
  if (d <= 0 || num_nodes <= 0 || nnz < 0) return RGCN_ERR_ARG;
  if (d % 32) return RGCN_ERR_UNSUPPORTED;
  if (num_nodes > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  if (nnz == 0) return RGCN_OK;
  if (!emb || !out_ptr || !out_dst || !edge_score) return RGCN_ERR_ARG;
  const int64_t blocks = ceil_div64(nnz * kEdgeLanes, kThreads);
  if (blocks > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  RGCN_ALIGN_TRY(16, emb);                       // rows as float4
  RGCN_ALIGN_TRY(8, out_ptr);
  RGCN_ALIGN_TRY(4, out_dst, edge_score);
  k_edge_cosine<<<(unsigned)blocks, kThreads, 0, (hipStream_t)stream_>>>(emb, (int)num_nodes, d, out_ptr, out_dst, nnz,
                                                                         edge_score);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

size_t rgcn_paths_workspace_bytes(int64_t num_queries, int k, int slices) {
  if (num_queries <= 0 || k <= 0 || k > RGCN_PATHS_MAX_K || slices < 0) return 0;
  return (size_t)num_queries * plan_slices(num_queries, slices) * kWaves * k * sizeof(rgcn_path_entry);
}

int rgcn_paths_topk(const int64_t* out_ptr, const int32_t* out_dst, const float* edge_score, const int64_t* in_ptr,
                    const int32_t* in_src, const int64_t* in_pos, int64_t num_nodes, int64_t nnz, const int64_t* sources,
                    const int64_t* targets, int64_t num_queries, int max_len, int k, int slices, int32_t* nodes,
                    int32_t* length, float* score, int64_t* count, void* ws, size_t ws_bytes, void* stream_) {
  if (num_queries < 0 || num_nodes <= 0 || nnz < 0) return RGCN_ERR_ARG;
  if (max_len < 1 || max_len > RGCN_PATHS_MAX_LEN || k <= 0 || slices < 0) return RGCN_ERR_ARG;
  if (num_queries == 0) return RGCN_OK;
  if (k > RGCN_PATHS_MAX_K || num_nodes > INT32_MAX || num_queries > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  if (!out_ptr || !in_ptr || !sources || !targets || !nodes || !length || !score || !count) return RGCN_ERR_ARG;
  if (nnz > 0 && (!out_dst || !edge_score || !in_src || !in_pos)) return RGCN_ERR_ARG;
  if (!ws || ws_bytes < rgcn_paths_workspace_bytes(num_queries, k, slices)) return RGCN_ERR_ARG;
  hipStream_t stream = (hipStream_t)stream_;
  const int S = plan_slices(num_queries, slices);
  if ((int64_t)S * kWaves * k > INT32_MAX) return RGCN_ERR_UNSUPPORTED;
  RGCN_ALIGN_TRY(16, ws);
  RGCN_ALIGN_TRY(8, out_ptr, in_ptr, in_pos, sources, targets, count);
  RGCN_ALIGN_TRY(4, out_dst, edge_score, in_src, nodes, length, score);
  PathWeights pw;
  pw.w[0] = 0.f;
  for (int L = 1; L <= RGCN_PATHS_MAX_LEN; ++L) pw.w[L] = rgcn_path_weight(L);
  RGCN_HIP_TRY(hipMemsetAsync(count, 0, (size_t)num_queries * RGCN_PATHS_MAX_LEN * sizeof(int64_t), stream));
  k_paths_select<<<dim3((unsigned)num_queries, (unsigned)S), kThreads, 0, stream>>>(
      out_ptr, out_dst, edge_score, in_ptr, in_src, in_pos, (int)num_nodes, nnz, sources, targets, max_len, k, pw,
      (rgcn_path_entry*)ws, (unsigned long long*)count);
  RGCN_HIP_TRY(hipGetLastError());
  k_paths_merge<<<(unsigned)num_queries, 64, 0, stream>>>((const rgcn_path_entry*)ws, S * kWaves * k, k, sources, targets,
                                                         nodes, length, score);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
