// K-means (Lloyd) and silhouette samples of embedding rows (include/rgcn_cluster.h; the reference's
// visualize_embeddings.cluster_analysis: KMeans(n_init = 10) + silhouette_score per node type).
//
// Both matrix products go through the k-tile of k_gemm_nt_dma<2, B_BLK> and the walk of k_topk_select over its entity
// range, both shared (rgcn_mma_f32_dma.h): a workgroup owns 64 rows and takes the (column tile, k-tile) pairs as ONE
// stream through the three-buffer ring (mma_f32_dma::walk_tiles).  What differs is what happens to the 64 x 128
// accumulators after the last k-tile of a column tile:
//   assignment  X . C^T   the centroids of all R restarts are the columns, every restart padded to a multiple of 32,
//                         so a 32-column accumulator block belongs to one restart: key = |c|^2 - 2 acc, arg-min over
//                         the block's 32 lanes, one (key, id) pair per (row, block) to the workspace; a finish kernel
//                         takes the minimum over a restart's blocks in block order.
//   silhouette  X . Xs^T  Xs = the rows grouped by label, every label padded to a multiple of 32, so a block is one
//                         label: dist = sqrt(max(0, |x_i|^2 + |x_j|^2 - 2 acc)) is added into 16 registers per lane;
//                         at a label boundary the 32 lanes are summed and the wave writes S[row][label] - once per
//                         (wave column, slice, label), because a label's blocks are consecutive in a wave's stream.
// Neither epilogue touches LDS (the cross-lane steps are ds_bpermute, which is no memory access), so nothing makes the
// compiler drain the LDS-DMA ring.
// The centroid update is a segmented sum, not a product: partial sums per fixed row chunk, the chunks added in order.
#include <math.h>

#include <algorithm>

#include "../../include/rgcn_cluster.h"
#include "rgcn_common.h"
#include "rgcn_mma_f32_dma.h"

namespace {

using namespace mma_f32_dma;    // kThreads (256: 4 waves, 2 (m) x 2 (n)), BK, BM, NBUF, walk_tiles, acc_row, the vector types

typedef KTile<2, B_BLK> Tile;   // 64 x 128 outputs per workgroup
constexpr int BN = Tile::BN;
constexpr int STAGE_BYTES = NBUF * Tile::BUF_FLOATS * 4;         // 73,728: the ring is the kernels' only LDS object
constexpr int kMaxK = RGCN_CLUSTER_MAX_K;
constexpr int kMaxSlices = 256;
constexpr int kNanBias = 1 << 20;   // id offset of a NaN key: behind every real id, in front of the pad columns
constexpr int kPadId = 0x7fffffff;
constexpr int kUpdCols = 128;   // columns (= threads) of an update workgroup
constexpr int kUpdRows = 256;   // rows whose labels an update workgroup stages at a time
constexpr int kInertiaRows = 256;

// |row|^2 of `rows` rows, one thread per row: an fmaf chain in the order in which the tile above takes the k of a
// product (per 8 floats: 0, 4, 1, 5, 2, 6, 3, 7), so that |x_i|^2 and <x_i, x_j> of two equal rows agree as closely as
// the matrix core allows.  `zero` (may be NULL): int32[zero_n], entry i cleared unless flag[i] is set - the
// assignment's per-restart counters ride on this launch.
__global__ __launch_bounds__(256) void k_row_norms(const float* __restrict__ x, int64_t rows, int d, float* __restrict__ out,
                                                   int32_t* __restrict__ zero, int zero_n, const int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (zero && i < zero_n && !(flag && flag[i])) zero[i] = 0;
  if (i >= rows) return;
  const f32x4* p = reinterpret_cast<const f32x4*>(x + (size_t)i * d);
  float acc = 0.f;
  for (int j = 0; j < d / 8; ++j) {
    const f32x4 u = p[2 * j], v = p[2 * j + 1];
    acc = __builtin_fmaf(u.x, u.x, acc); acc = __builtin_fmaf(v.x, v.x, acc);
    acc = __builtin_fmaf(u.y, u.y, acc); acc = __builtin_fmaf(v.y, v.y, acc);
    acc = __builtin_fmaf(u.z, u.z, acc); acc = __builtin_fmaf(v.z, v.z, acc);
    acc = __builtin_fmaf(u.w, u.w, acc); acc = __builtin_fmaf(v.w, v.w, acc);
  }
  out[i] = acc;
}

// (key, id) order of the arg-min: key ascending, then id ascending
__device__ __forceinline__ void take_min(float& key, int& id, float okey, int oid) {
  const bool better = okey < key || (okey == key && oid < id);
  key = better ? okey : key;
  id = better ? oid : id;
}

// ------------------------------------------------------------------------------------------ assignment
// grid ceil(M / 64): the workgroup walks all R * kb blocks of 32 columns (kb = ceil(k / 32) blocks per restart).
// pkey / pid [M][nblk]: the best (key, id) of every (row, block); id is the cluster id, + kNanBias for a NaN key.
__global__ __launch_bounds__(kThreads) void k_assign(const float* __restrict__ x, const float* __restrict__ cent,
                                                     const float* __restrict__ cnorm, int M, int d, int R, int k, int kb,
                                                     int num_tiles, float* __restrict__ pkey, int* __restrict__ pid) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int m0 = blockIdx.x * BM;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  const int nblk = R * kb, kp = kb * 32;
  Tile tile(wm, wn, li, lh);

  float cn[2] = {0.f, 0.f};                                    // |c|^2 of this lane's column in either block; +inf: pad
  int cid[2] = {kPadId, kPadId};
  auto pre = [&](int ct) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int blk = ct * 4 + wn * 2 + b;
      const int r = blk / kb, c = (blk - r * kb) * 32 + li;
      const bool real = r < R && c < k;
      cn[b] = cnorm[real ? r * k + c : 0];
      cid[b] = real ? c : kPadId;
    }
  };
  auto epi = [&](int ct, floatx16 (&acc)[2]) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int blk = ct * 4 + wn * 2 + b;
      if (blk >= nblk) continue;                               // wave-uniform
      float mkey = INFINITY;
      int mid = kPadId;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float key = __builtin_fmaf(-2.f, acc[b][r], cn[b]);
        int id = cid[b];
        if (id == kPadId) key = INFINITY;
        else if (key != key) { key = INFINITY; id += kNanBias; }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) take_min(key, id, __shfl_xor(key, o), __shfl_xor(id, o));
        if (li == r) { mkey = key; mid = id; }
      }
      const int m = m0 + wm * 32 + acc_row(li & 15, lh);
      if (li < 16 && m < M) {
        pkey[(size_t)m * nblk + blk] = mkey;
        pid[(size_t)m * nblk + blk] = mid;
      }
    }
  };
  walk_tiles(lds, x, cent, M, d, m0, 0, num_tiles, wave, lane, tile,
             [&](int n) { const int r = min(n / kp, R - 1); return r * k + min(n - (n / kp) * kp, k - 1); }, pre, epi);
}

// one thread per (restart, row): the minimum over the restart's blocks in block order, the label, the change count
__global__ __launch_bounds__(256) void k_assign_finish(const float* __restrict__ pkey, const int* __restrict__ pid, int M,
                                                       int R, int kb, const int32_t* labels_prev, int32_t* labels,
                                                       int32_t* __restrict__ num_changed, const int32_t* __restrict__ done) {
  const int r = blockIdx.y;
  if (done && done[r]) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool changed = false;
  if (i < M) {
    const size_t base = (size_t)i * (R * kb) + (size_t)r * kb;
    float key = pkey[base];
    int id = pid[base];
    for (int b = 1; b < kb; ++b) take_min(key, id, pkey[base + b], pid[base + b]);
    const int label = id >= kNanBias ? id - kNanBias : id;
    const size_t o = (size_t)r * M + i;
    changed = !labels_prev || labels_prev[o] != label;
    labels[o] = label;
  }
  const int n = __popcll(__ballot(changed));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&num_changed[r], n);   // an integer: the order of arrival does not show
}

// ------------------------------------------------------------------------------------------ update
// grid (chunks, R, ceil(d / 128)): thread = one column; the rows of the chunk in order, each added into the LDS slot of
// its label - a thread touches only its own column, so there is no race and the order is the row order.
__global__ __launch_bounds__(kUpdCols) void k_update_partial(const float* __restrict__ x, const int32_t* __restrict__ labels,
                                                             int M, int d, int k, int rows_per_chunk,
                                                             const int32_t* __restrict__ done, float* __restrict__ part,
                                                             int32_t* __restrict__ pcnt) {
  __shared__ float s_sum[kMaxK * kUpdCols];
  __shared__ int s_lab[kUpdRows];
  const int chunk = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  if (done && done[r]) return;
  const int j = blockIdx.z * kUpdCols + tid;
  const bool jok = j < d;
  for (int c = 0; c < k; ++c) s_sum[c * kUpdCols + tid] = 0.f;
  const int i0 = chunk * rows_per_chunk, i1 = min(M, i0 + rows_per_chunk);
  int cnt = 0;                                                 // rows of label `tid` (threads below k)
  for (int base = i0; base < i1; base += kUpdRows) {
    __syncthreads();
    for (int t = tid; t < kUpdRows; t += kUpdCols) s_lab[t] = base + t < i1 ? labels[(size_t)r * M + base + t] : 0;
    __syncthreads();
    const int n = min(kUpdRows, i1 - base);
    const float* xr = x + (size_t)base * d + (jok ? j : 0);
#pragma unroll 4
    for (int ii = 0; ii < n; ++ii) {
      const int c = min(max(s_lab[ii], 0), k - 1);
      const float v = xr[(size_t)ii * d];
      if (jok) s_sum[c * kUpdCols + tid] += v;
      cnt += c == tid;
    }
  }
  const size_t slot = (size_t)r * gridDim.x + chunk;
  if (jok)
    for (int c = 0; c < k; ++c) part[(slot * k + c) * d + j] = s_sum[c * kUpdCols + tid];
  if (blockIdx.z == 0 && tid < k) pcnt[slot * k + tid] = cnt;
}

// sum of the 128 values of a workgroup in a fixed tree
__device__ __forceinline__ float block_sum_128(float v, float* s, int tid) {
  s[tid] = v;
  __syncthreads();
  for (int o = 64; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  return s[0];
}

// grid (k, R): the chunks in order -> count, mean (or the old centroid), |new - old|^2 of this cluster
__global__ __launch_bounds__(kUpdCols) void k_update_finish(const float* __restrict__ part, const int32_t* __restrict__ pcnt,
                                                            int chunks, int d, int k, const int32_t* __restrict__ done,
                                                            float* __restrict__ cent, int32_t* __restrict__ counts,
                                                            float* __restrict__ shift_part) {
  __shared__ float s_red[kUpdCols];
  const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  if (done && done[r]) return;
  int count = 0;
  for (int ch = 0; ch < chunks; ++ch) count += pcnt[((size_t)r * chunks + ch) * k + c];
  float local = 0.f;
  for (int j = tid; j < d; j += kUpdCols) {
    float s = 0.f;
    for (int ch = 0; ch < chunks; ++ch) s += part[(((size_t)r * chunks + ch) * k + c) * d + j];
    float* at = cent + ((size_t)r * k + c) * d + j;
    const float old = *at;
    const float nw = count > 0 ? s / (float)count : old;
    const float diff = nw - old;
    local = __builtin_fmaf(diff, diff, local);
    *at = nw;
  }
  const float total = block_sum_128(local, s_red, tid);
  if (tid == 0) {
    shift_part[r * k + c] = total;
    counts[r * k + c] = count;
  }
}

// one thread per restart: shift^2, the iteration count, the done flag
__global__ void k_converge(const float* __restrict__ shift_part, const int32_t* __restrict__ num_changed, int R, int k,
                           float tol_abs, float* __restrict__ shift2, int32_t* __restrict__ num_iter, int32_t* done) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R || (done && done[r])) return;
  float s = 0.f;
  for (int c = 0; c < k; ++c) s += shift_part[r * k + c];
  shift2[r] = s;
  num_iter[r] += 1;
  if (done && (num_changed[r] == 0 || s <= tol_abs)) done[r] = 1;
}

// ------------------------------------------------------------------------------------------ inertia
// grid (ceil(M / 256), R): wave w takes rows w, w + 4, ... of the chunk; a row's squared distance is an fp32 sum (lane
// = column mod 64, then a butterfly), the rows are added in double
__global__ __launch_bounds__(256) void k_inertia_partial(const float* __restrict__ x, const float* __restrict__ cent,
                                                         const int32_t* __restrict__ labels, int M, int d, int k,
                                                         double* __restrict__ ipart) {
  __shared__ double s_w[4];
  const int r = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.x * kInertiaRows, i1 = min(M, i0 + kInertiaRows);
  double acc = 0.0;
  for (int i = i0 + wave; i < i1; i += 4) {
    int c = labels[(size_t)r * M + i];
    c = min(max(c, 0), k - 1);
    const float* xr = x + (size_t)i * d;
    const float* cr = cent + ((size_t)r * k + c) * d;
    float s = 0.f;
    for (int j = lane; j < d; j += 64) {
      const float diff = xr[j] - cr[j];
      s = __builtin_fmaf(diff, diff, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    acc += (double)s;
  }
  if (lane == 0) s_w[wave] = acc;
  __syncthreads();
  if (tid == 0) ipart[(size_t)r * gridDim.x + blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ void k_inertia_finish(const double* __restrict__ ipart, int R, int chunks, double* __restrict__ inertia) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  double s = 0.0;
  for (int ch = 0; ch < chunks; ++ch) s += ipart[(size_t)r * chunks + ch];
  inertia[r] = s;
}

// ------------------------------------------------------------------------------------------ silhouette
// grid (ceil(M / 64), S): slice s walks column tiles [s * tiles_per_slice, ...) of xs.  ws_s [S][2][M][k], zeroed by
// the host: S[row][label] as wave column 0 / 1 of slice s saw it (a label a wave never meets stays 0).
__global__ __launch_bounds__(kThreads) void k_silhouette(const float* __restrict__ x, const float* __restrict__ xs,
                                                         const float* __restrict__ xnorm, const float* __restrict__ cnorm,
                                                         const int32_t* __restrict__ col_row,
                                                         const int32_t* __restrict__ blk_cluster, int M, int Mp, int d, int k,
                                                         int tiles_per_slice, int num_tiles, float* __restrict__ ws_s) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int m0 = blockIdx.x * BM;
  const int ct_begin = blockIdx.y * tiles_per_slice, ct_end = min(num_tiles, ct_begin + tiles_per_slice);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int li = lane & 31, lh = lane >> 5;
  Tile tile(wm, wn, li, lh);

  float xn[16], part[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    xn[r] = xnorm[min(m0 + wm * 32 + acc_row(r, lh), M - 1)];
    part[r] = 0.f;
  }
  float* out = ws_s + ((size_t)blockIdx.y * 2 + wn) * M * k;
  int cur_cl = -1;                                             // the label the registers are collecting; wave-uniform

  // the 32 lanes of a half hold 32 columns of the same 16 rows: sum them, lane li < 16 writes row acc_row(li, lh)
  auto flush = [&]() {
    if (cur_cl >= 0) {
      float mine = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = part[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (li == r) mine = v;
      }
      const int m = m0 + wm * 32 + acc_row(li & 15, lh);
      if (li < 16 && m < M) out[(size_t)m * k + cur_cl] = mine;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) part[r] = 0.f;
  };

  int cj[2] = {-1, -1}, cl[2] = {-1, -1};
  float cn[2] = {0.f, 0.f};
  auto pre = [&](int ct) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int blk = ct * 4 + wn * 2 + b;                     // (Mp % 128 == 0: every block of a tile exists)
      cj[b] = col_row[blk * 32 + li];
      cn[b] = cnorm[blk * 32 + li];
      cl[b] = blk_cluster[blk];
    }
  };
  auto epi = [&](int ct, floatx16 (&acc)[2]) {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int c = __builtin_amdgcn_readfirstlane(cl[b]);
      if (c != cur_cl) {
        flush();
        cur_cl = (c >= 0 && c < k) ? c : -1;
      }
      if (cur_cl < 0) continue;
      const int j = cj[b];
      const float nj = cn[b];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + acc_row(r, lh);
        const float d2 = __builtin_fmaf(-2.f, acc[b][r], xn[r] + nj);
        const float dist = __builtin_amdgcn_sqrtf(fmaxf(d2, 0.f));
        part[r] += (j < 0 || j == m) ? 0.f : dist;
      }
    }
  };
  walk_tiles(lds, x, xs, M, d, m0, ct_begin, ct_end, wave, lane, tile, [&](int n) { return min(n, Mp - 1); }, pre, epi);
  flush();
}

// one thread per row: the slices in order (wave column 0, then 1), a, b, s
__global__ __launch_bounds__(256) void k_silhouette_finish(const float* __restrict__ ws_s, const int32_t* __restrict__ counts,
                                                           const int32_t* __restrict__ labels, int M, int k, int S,
                                                           float* __restrict__ s_out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M) return;
  const int own = min(max(labels[i], 0), k - 1);
  float a = 0.f, b = INFINITY;
  for (int c = 0; c < k; ++c) {
    const int nc = counts[c];
    if (nc <= 0) continue;                                     // a label nobody carries
    float sum = 0.f;
    for (int s = 0; s < S; ++s) {
      sum += ws_s[((size_t)(2 * s) * M + i) * k + c];
      sum += ws_s[((size_t)(2 * s + 1) * M + i) * k + c];
    }
    if (c == own) a = nc > 1 ? sum / (float)(nc - 1) : 0.f;
    else b = fminf(b, sum / (float)nc);
  }
  const float mx = fmaxf(a, b);
  float v = 0.f;
  if (counts[own] > 1 && b < INFINITY && mx > 0.f) v = (b - a) / mx;
  s_out[i] = v;
}

// mean of n floats in double, one workgroup: thread t sums elements t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void k_mean_double(const float* __restrict__ v, int n, double* __restrict__ mean) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < n; i += 256) acc += (double)v[i];
  s[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  if (tid == 0) mean[0] = s[0] / (double)n;
}

// ------------------------------------------------------------------------------------------ host side
inline int kmeans_shape_error(int64_t M, int64_t d, int64_t R, int64_t k) {
  if (M < 2 || d <= 0 || R < 1 || k < 2) return RGCN_ERR_ARG;
  if (d % BK || d > (1 << 20) || k > kMaxK || R > RGCN_CLUSTER_MAX_RESTARTS || M >= (1 << 30)) return RGCN_ERR_UNSUPPORTED;
  return RGCN_OK;
}

struct KmeansPlan {
  int kb, nblk, num_tiles, rows_per_chunk, chunks, ichunks;
  size_t o_cnorm, o_pkey, o_pid, o_part, o_pcnt, o_shift, o_ipart, bytes;
};

inline KmeansPlan plan_kmeans(int64_t M, int64_t d, int64_t R, int64_t k) {
  KmeansPlan p;
  p.kb = (int)ceil_div64(k, 32);
  p.nblk = (int)(R * p.kb);
  p.num_tiles = (int)ceil_div64((int64_t)p.nblk * 32, BN);
  p.rows_per_chunk = kUpdRows * (int)std::max<int64_t>(1, ceil_div64(M, (int64_t)kUpdRows * 64));   // at most 64 chunks
  p.chunks = (int)ceil_div64(M, p.rows_per_chunk);
  p.ichunks = (int)ceil_div64(M, kInertiaRows);
  size_t at = 0;
  p.o_cnorm = at; at += align256((size_t)R * k * 4);
  p.o_pkey = at;  at += align256((size_t)M * p.nblk * 4);
  p.o_pid = at;   at += align256((size_t)M * p.nblk * 4);
  p.o_part = at;  at += align256((size_t)R * p.chunks * k * d * 4);
  p.o_pcnt = at;  at += align256((size_t)R * p.chunks * k * 4);
  p.o_shift = at; at += align256((size_t)R * k * 4);
  p.o_ipart = at; at += align256((size_t)R * p.ichunks * 8);
  p.bytes = at;
  return p;
}

struct SilPlan {
  int num_tiles, tiles_per_slice, slices;
  size_t o_xnorm, o_cnorm, o_s, s_bytes, bytes;
};

// slices as rank_topk.hip chooses its own, for four workgroups per CU: a walk over all of xs is long (M / 128 column
// tiles), and 298 row tiles of one slice each (M = 19,051) left the CUs unevenly loaded - 1.94 ms against 1.42 ms at
// four slices (profiles/cluster_time.json)
inline SilPlan plan_silhouette(int64_t M, int64_t Mp, int64_t k, int64_t slices) {
  SilPlan p;
  p.num_tiles = (int)(Mp / BN);
  const int64_t row_tiles = ceil_div64(M, BM);
  const rgcn_slicing cut = rgcn_slice_tiles(p.num_tiles, slices > 0 ? slices : ceil_div64(4 * kCUs, row_tiles), kMaxSlices);
  p.tiles_per_slice = cut.tiles_per_slice;
  p.slices = cut.slices;
  size_t at = 0;
  p.o_xnorm = at; at += align256((size_t)M * 4);
  p.o_cnorm = at; at += align256((size_t)Mp * 4);
  p.o_s = at;
  p.s_bytes = (size_t)p.slices * 2 * M * k * 4;
  at += align256(p.s_bytes);
  p.bytes = at;
  return p;
}

inline bool silhouette_shape_ok(int64_t M, int64_t Mp, int64_t k, int64_t slices) {
  return M >= 2 && M < (1 << 30) && Mp >= M && Mp % BN == 0 && Mp < (1 << 30) && k >= 2 && k <= kMaxK && slices >= 0;
}

}  // namespace

extern "C" {

size_t rgcn_kmeans_workspace_bytes(int64_t M, int64_t d, int64_t R, int64_t k) {
  if (kmeans_shape_error(M, d, R, k)) return 0;
  return plan_kmeans(M, d, R, k).bytes;
}

int rgcn_kmeans_assign(const float* x, int64_t M, int64_t d, const float* centroids, int64_t R, int64_t k,
                       const int32_t* labels_prev, int32_t* labels, int32_t* num_changed, const int32_t* done, void* ws,
                       size_t ws_bytes, void* stream_) {
  const int bad = kmeans_shape_error(M, d, R, k);
  if (bad) return bad;
  if (!x || !centroids || !labels || !num_changed) return RGCN_ERR_ARG;
  const KmeansPlan p = plan_kmeans(M, d, R, k);
  if (!ws || ws_bytes < p.bytes) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, x, centroids, ws);          // rows and centroids stream in 16-byte DMA pieces
  RGCN_ALIGN_TRY(4, labels_prev, labels, num_changed, done);
  hipStream_t stream = (hipStream_t)stream_;
  static bool raised[64] = {};
  const int rc = raise_lds(k_assign, STAGE_BYTES, raised);
  if (rc) return rc;
  char* w = (char*)ws;
  float* cnorm = (float*)(w + p.o_cnorm);
  float* pkey = (float*)(w + p.o_pkey);
  int* pid = (int*)(w + p.o_pid);
  const int64_t crows = R * k;
  k_row_norms<<<(unsigned)ceil_div64(crows, 256), 256, 0, stream>>>(centroids, crows, (int)d, cnorm,
                                                                                         num_changed, (int)R, done);
  RGCN_HIP_TRY(hipGetLastError());
  k_assign<<<(unsigned)ceil_div64(M, BM), kThreads, STAGE_BYTES, stream>>>(x, centroids, cnorm, (int)M, (int)d, (int)R, (int)k,
                                                                          p.kb, p.num_tiles, pkey, pid);
  RGCN_HIP_TRY(hipGetLastError());
  k_assign_finish<<<dim3((unsigned)ceil_div64(M, 256), (unsigned)R), 256, 0, stream>>>(pkey, pid, (int)M, (int)R, p.kb,
                                                                                      labels_prev, labels, num_changed, done);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

int rgcn_kmeans_update(const float* x, int64_t M, int64_t d, float* centroids, int64_t R, int64_t k, const int32_t* labels,
                       const int32_t* num_changed, int32_t* counts, float* shift2, int32_t* num_iter, int32_t* done,
                       float tol_abs, void* ws, size_t ws_bytes, void* stream_) {
  const int bad = kmeans_shape_error(M, d, R, k);
  if (bad) return bad;
  if (!(tol_abs >= 0.f)) return RGCN_ERR_ARG;
  if (!x || !centroids || !labels || !num_changed || !counts || !shift2 || !num_iter) return RGCN_ERR_ARG;
  const KmeansPlan p = plan_kmeans(M, d, R, k);
  if (!ws || ws_bytes < p.bytes) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, x, centroids, ws);
  RGCN_ALIGN_TRY(4, labels, num_changed, counts, shift2, num_iter, done);
  hipStream_t stream = (hipStream_t)stream_;
  char* w = (char*)ws;
  float* part = (float*)(w + p.o_part);
  int32_t* pcnt = (int32_t*)(w + p.o_pcnt);
  float* shift_part = (float*)(w + p.o_shift);
  k_update_partial<<<dim3((unsigned)p.chunks, (unsigned)R, (unsigned)ceil_div64(d, kUpdCols)), kUpdCols, 0, stream>>>(
      x, labels, (int)M, (int)d, (int)k, p.rows_per_chunk, done, part, pcnt);
  RGCN_HIP_TRY(hipGetLastError());
  k_update_finish<<<dim3((unsigned)k, (unsigned)R), kUpdCols, 0, stream>>>(part, pcnt, p.chunks, (int)d, (int)k, done, centroids,
                                                                         counts, shift_part);
  RGCN_HIP_TRY(hipGetLastError());
  k_converge<<<(unsigned)ceil_div64(R, 64), 64, 0, stream>>>(shift_part, num_changed, (int)R, (int)k, tol_abs, shift2, num_iter, done);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

int rgcn_kmeans_inertia(const float* x, int64_t M, int64_t d, const float* centroids, int64_t R, int64_t k,
                        const int32_t* labels, double* inertia, void* ws, size_t ws_bytes, void* stream_) {
  const int bad = kmeans_shape_error(M, d, R, k);
  if (bad) return bad;
  if (!x || !centroids || !labels || !inertia) return RGCN_ERR_ARG;
  const KmeansPlan p = plan_kmeans(M, d, R, k);
  if (!ws || ws_bytes < p.bytes) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, x, centroids, ws);
  RGCN_ALIGN_TRY(8, inertia);
  RGCN_ALIGN_TRY(4, labels);
  hipStream_t stream = (hipStream_t)stream_;
  double* ipart = (double*)((char*)ws + p.o_ipart);
  k_inertia_partial<<<dim3((unsigned)p.ichunks, (unsigned)R), 256, 0, stream>>>(x, centroids, labels, (int)M, (int)d, (int)k, ipart);
  RGCN_HIP_TRY(hipGetLastError());
  k_inertia_finish<<<(unsigned)ceil_div64(R, 64), 64, 0, stream>>>(ipart, (int)R, p.ichunks, inertia);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

size_t rgcn_silhouette_workspace_bytes(int64_t M, int64_t Mp, int64_t k, int64_t slices) {
  if (!silhouette_shape_ok(M, Mp, k, slices)) return 0;
  return plan_silhouette(M, Mp, k, slices).bytes;
}

int rgcn_silhouette_samples(const float* x, const float* xs, const int32_t* col_row, const int32_t* blk_cluster,
                            const int32_t* counts, const int32_t* labels, int64_t M, int64_t Mp, int64_t d, int64_t k,
                            int64_t slices, float* s, double* mean, void* ws, size_t ws_bytes, void* stream_) {
  if (M < 2 || d <= 0 || k < 2 || slices < 0 || Mp < M || Mp % BN) return RGCN_ERR_ARG;
  if (d % BK || d > (1 << 20) || k > kMaxK || M >= (1 << 30) || Mp >= (1 << 30)) return RGCN_ERR_UNSUPPORTED;
  if (!x || !xs || !col_row || !blk_cluster || !counts || !labels || !s || !mean) return RGCN_ERR_ARG;
  const SilPlan p = plan_silhouette(M, Mp, k, slices);
  if (!ws || ws_bytes < p.bytes) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, x, xs, ws);
  RGCN_ALIGN_TRY(8, mean);
  RGCN_ALIGN_TRY(4, col_row, blk_cluster, counts, labels, s);
  hipStream_t stream = (hipStream_t)stream_;
  static bool raised[64] = {};
  const int rc = raise_lds(k_silhouette, STAGE_BYTES, raised);
  if (rc) return rc;
  char* w = (char*)ws;
  float* xnorm = (float*)(w + p.o_xnorm);
  float* cnorm = (float*)(w + p.o_cnorm);
  float* ws_s = (float*)(w + p.o_s);
  k_row_norms<<<(unsigned)ceil_div64(M, 256), 256, 0, stream>>>(x, M, (int)d, xnorm, nullptr, 0, nullptr);
  RGCN_HIP_TRY(hipGetLastError());
  k_row_norms<<<(unsigned)ceil_div64(Mp, 256), 256, 0, stream>>>(xs, Mp, (int)d, cnorm, nullptr, 0, nullptr);
  RGCN_HIP_TRY(hipGetLastError());
  RGCN_HIP_TRY(hipMemsetAsync(ws_s, 0, p.s_bytes, stream));
  k_silhouette<<<dim3((unsigned)ceil_div64(M, BM), (unsigned)p.slices), kThreads, STAGE_BYTES, stream>>>(
      x, xs, xnorm, cnorm, col_row, blk_cluster, (int)M, (int)Mp, (int)d, (int)k, p.tiles_per_slice, p.num_tiles, ws_s);
  RGCN_HIP_TRY(hipGetLastError());
  k_silhouette_finish<<<(unsigned)ceil_div64(M, 256), 256, 0, stream>>>(ws_s, counts, labels, (int)M, (int)k, p.slices, s);
  RGCN_HIP_TRY(hipGetLastError());
  k_mean_double<<<1, 256, 0, stream>>>(s, (int)M, mean);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
