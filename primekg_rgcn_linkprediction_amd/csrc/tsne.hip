// t-SNE projection of embedding rows (include/rgcn_tsne.h; the reference's visualize_embeddings.reduce_dimensions:
// TSNE(n_components = 2, perplexity = min(30, n - 1), max_iter = 1000)).
//
// The neighbour selection is rank_topk.hip's pass on augmented rows; what is new here:
//   k_knn_refine        one wave per row: drops the row itself from its k + 1 candidates, recomputes the k squared
//                       distances from the differences and orders them by counting.
//   k_tsne_affinities   one wave per row: scikit-learn's perplexity search, in double.
//   k_tsne_repulsion    the hot kernel, all pairs: a workgroup owns 256 rows (y_i in registers) and walks its slice of
//                       the columns through LDS - every lane reads the same y_j, a broadcast - with eight independent
//                       accumulator chains per row, folded after every 256 columns.  The self pair is masked only in
//                       the tile that holds the workgroup's own rows.  Per (slice, row) it leaves sum q (double),
//                       sum q^2 dx, sum q^2 dy.
//   k_tsne_z            per 256 rows: the slices of every row in slice order, the rows in a fixed tree, in double;
//                       k_sum_double adds the tiles.
//   k_tsne_attraction   one wave per CSR row (any length: a hub is everybody's neighbour), entries in column order,
//                       then the gradient and, when asked, the row's share of the KL sum in double.
//   k_tsne_update       scikit-learn's _gradient_descent body, elementwise, and the partial sums of |g|^2.
// No floating-point atomics anywhere: every order of summation is fixed by (M, nnz, slices).
#include <float.h>
#include <math.h>

#include "../../include/rgcn_tsne.h"
#include "rgcn_common.h"

namespace {

constexpr int kMaxK = RGCN_KNN_MAX_K;
constexpr int kSlots = 128;          // candidates of a row: k + 1 <= 128, two per lane
constexpr int kTile = 256;           // rows of a repulsion workgroup = the unit in which slices divide the columns
constexpr int kChunk = 1024;         // columns staged in LDS at a time (8 KB)
constexpr int kMaxSlices = 64;
constexpr int64_t kMaxM = (int64_t)1 << 24;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return __shfl(v, 0);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return __shfl(v, 0);
}

// sum of 256 doubles of a workgroup in a fixed tree; the result in thread 0
__device__ __forceinline__ double block_sum_256(double v, double* s, int tid) {
  s[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s[tid] += s[tid + o];
    __syncthreads();
  }
  return s[0];
}

// ------------------------------------------------------------------------------------------ neighbours
__device__ __forceinline__ float sqdist_rows(const float* __restrict__ a, const float* __restrict__ b, int d) {
  const float4* pa = reinterpret_cast<const float4*>(a);
  const float4* pb = reinterpret_cast<const float4*>(b);
  float acc = 0.f;
  for (int c = 0; c < d / 4; ++c) {
    const float4 u = pa[c], v = pb[c];
    float t = u.x - v.x; acc = __builtin_fmaf(t, t, acc);
    t = u.y - v.y; acc = __builtin_fmaf(t, t, acc);
    t = u.z - v.z; acc = __builtin_fmaf(t, t, acc);
    t = u.w - v.w; acc = __builtin_fmaf(t, t, acc);
  }
  return acc;
}

// grid ceil(M / 4), one wave per row; lane l holds candidates l and l + 64.  A slot that is not kept has key NaN.
__global__ __launch_bounds__(256) void k_knn_refine(const float* __restrict__ x, int M, int d,
                                                    const int64_t* __restrict__ cand, int k, int32_t* __restrict__ ids,
                                                    float* __restrict__ sqdist) {
  __shared__ float s_key[4][kSlots];
  __shared__ int s_id[4][kSlots];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x * 4 + wave;
  const bool row = i < M;
  const int n = k + 1;
  int id[2];
  float dist[2];
  bool self[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    const int64_t v = (row && c < n) ? cand[(size_t)i * n + c] : -1;
    id[h] = (v >= 0 && v < M) ? (int)v : -1;
    self[h] = row && c < n && id[h] == i;
  }
  const unsigned long long self0 = __ballot(self[0]), self1 = __ballot(self[1]);
  const int drop = self0 ? __ffsll((long long)self0) - 1 : self1 ? 64 + __ffsll((long long)self1) - 1 : k;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    const bool kept = row && c < n && c != drop;
    dist[h] = INFINITY;
    if (kept && id[h] >= 0) dist[h] = sqdist_rows(x + (size_t)i * d, x + (size_t)id[h] * d, d);
    s_key[wave][c] = kept ? (dist[h] != dist[h] ? INFINITY : dist[h]) : NAN;
    s_id[wave][c] = id[h];
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    const float key = s_key[wave][c];
    if (key != key) continue;                                  // not kept
    int rank = 0;
    for (int o = 0; o < n; ++o) {
      const float okey = s_key[wave][o];
      const int oid = s_id[wave][o];
      const bool before = okey < key || (okey == key && (oid < id[h] || (oid == id[h] && o < c)));
      rank += before;                                          // (a NaN key compares false: not kept, not counted)
    }
    ids[(size_t)i * k + rank] = id[h];
    sqdist[(size_t)i * k + rank] = dist[h];
  }
}

// ------------------------------------------------------------------------------------------ affinities
// grid ceil(M / 4), one wave per row, lane l holds neighbours l and l + 64 (k <= 127)
__global__ __launch_bounds__(256) void k_tsne_affinities(const float* __restrict__ sqdist, int M, int k, double log_perp,
                                                         float* __restrict__ cond_p, float* __restrict__ beta_out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;                                          // wave-uniform; no barrier below
  const bool has0 = lane < k, has1 = lane + 64 < k;
  const double d0 = has0 ? (double)sqdist[(size_t)i * k + lane] : 0.0;
  const double d1 = has1 ? (double)sqdist[(size_t)i * k + lane + 64] : 0.0;
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, p0 = 0.0, p1 = 0.0;
  for (int step = 0; step < 100; ++step) {
    p0 = has0 ? exp(-d0 * beta) : 0.0;
    p1 = has1 ? exp(-d1 * beta) : 0.0;
    double s = wave_sum(p0 + p1);
    if (s == 0.0) s = 1e-8;
    p0 /= s;
    p1 /= s;
    const double dp = wave_sum(d0 * p0 + d1 * p1);
    const double diff = (log(s) + beta * dp) - log_perp;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  if (has0) cond_p[(size_t)i * k + lane] = (float)p0;
  if (has1) cond_p[(size_t)i * k + lane + 64] = (float)p1;
  if (lane == 0) beta_out[i] = (float)beta;
}

// ------------------------------------------------------------------------------------------ gradient
// |dy|^2 as two rounded products and a rounded sum (never contracted to an fma), and q = 1 / (1 + |dy|^2) as IEEE division
// gives it: what a host restatement of the header computes, bit for bit
__device__ __forceinline__ float sq_norm(float dx, float dy) { return __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)); }

// one pair: q by the hardware reciprocal and two Newton steps - the second, from a faithful estimate and the exact residual,
// rounds correctly (Markstein) -, q into z, q^2 dy into (rx, ry)
template <bool DIAG>
__device__ __forceinline__ void pair(float2 yi, float2 yj, bool same, float& z, float& rx, float& ry) {
  const float dx = yi.x - yj.x, dy = yi.y - yj.y;
  const float a = __fadd_rn(1.f, sq_norm(dx, dy));
  float q = __builtin_amdgcn_rcpf(a);
  q = __builtin_fmaf(__builtin_fmaf(-a, q, 1.f), q, q);
  q = __builtin_fmaf(__builtin_fmaf(-a, q, 1.f), q, q);
  if (DIAG && same) q = 0.f;
  z += q;
  const float q2 = q * q;
  rx = __builtin_fmaf(q2, dx, rx);
  ry = __builtin_fmaf(q2, dy, ry);
}

constexpr int kChains = 8;           // independent accumulator chains of a row

__device__ __forceinline__ float tree8(const float (&v)[kChains]) {
  return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// one 256-column tile (n <= 256 columns of it exist) against the thread's row: chain u takes columns u, u + 8, ...
template <bool DIAG>
__device__ __forceinline__ void walk_tile(const float2* __restrict__ s_y, int n, int self, float2 yi, float (&z)[kChains],
                                          float (&rx)[kChains], float (&ry)[kChains]) {
  int j = 0;
  for (; j + kChains <= n; j += kChains) {
#pragma unroll
    for (int u = 0; u < kChains; ++u) pair<DIAG>(yi, s_y[j + u], j + u == self, z[u], rx[u], ry[u]);
  }
#pragma unroll
  for (int u = 0; u < kChains - 1; ++u)
    if (j + u < n) pair<DIAG>(yi, s_y[j + u], j + u == self, z[u], rx[u], ry[u]);
}

// grid (ceil(M / 256), S): slice s walks columns [s * tiles_per_slice * 256, ...).  Per 256-column tile the eight fp32
// chains of a row (32 terms each) are added in a fixed tree; the tiles are added in order - sum q in double (Z is a sum
// of M^2 terms of one sign and enters KL as log Z), the two force sums in fp32.  zpart double[S][M], rpart float32[S][2][M].
__global__ __launch_bounds__(kTile) void k_tsne_repulsion(const float2* __restrict__ y, int M, int tiles_per_slice,
                                                          double* __restrict__ zpart, float* __restrict__ rpart) {
  __shared__ __attribute__((aligned(16))) float2 s_y[kChunk];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kTile, i = r0 + tid;
  const int c_begin = blockIdx.y * tiles_per_slice * kTile;
  const int c_end = min(M, c_begin + tiles_per_slice * kTile);
  const float2 yi = i < M ? y[i] : make_float2(0.f, 0.f);
  double zsum = 0.0;
  float rxsum = 0.f, rysum = 0.f;
  for (int c = c_begin; c < c_end; c += kChunk) {
    const int n = min(kChunk, c_end - c);
    __syncthreads();                                           // everybody is done with the previous chunk
    for (int t = tid; t < n; t += kTile) s_y[t] = y[c + t];
    __syncthreads();
    for (int t0 = 0; t0 < n; t0 += kTile) {
      float z[kChains], rx[kChains], ry[kChains];
#pragma unroll
      for (int u = 0; u < kChains; ++u) z[u] = rx[u] = ry[u] = 0.f;
      const int nt = min(kTile, n - t0);
      if (c + t0 == r0) walk_tile<true>(s_y + t0, nt, tid, yi, z, rx, ry);     // the workgroup's own rows: mask the self pair
      else walk_tile<false>(s_y + t0, nt, -1, yi, z, rx, ry);
      zsum += (double)tree8(z);
      rxsum += tree8(rx);
      rysum += tree8(ry);
    }
  }
  if (i < M) {
    zpart[(size_t)blockIdx.y * M + i] = zsum;
    float* out = rpart + (size_t)blockIdx.y * 2 * M;
    out[i] = rxsum;
    out[(size_t)M + i] = rysum;
  }
}

// grid ceil(M / 256): ztile[t] = the sum over the 256 rows of tile t of the row's slices (slice order), in double, a fixed
// tree; k_sum_double then adds the tiles - no single workgroup walks all S * M partial sums
__global__ __launch_bounds__(256) void k_tsne_z(const double* __restrict__ zpart, int M, int S, double* __restrict__ ztile) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * kTile + tid;
  double row = 0.0;
  if (i < M)
    for (int sl = 0; sl < S; ++sl) row += zpart[(size_t)sl * M + i];
  const double total = block_sum_256(row, s, tid);
  if (tid == 0) ztile[blockIdx.x] = total;
}

// one workgroup: out[0] = the sum of n doubles, thread t takes t, t + 256, ... in order, then a fixed tree
__global__ __launch_bounds__(256) void k_sum_double(const double* __restrict__ v, int n, double* __restrict__ out) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  double acc = 0.0;
  for (int i = tid; i < n; i += 256) acc += v[i];
  const double total = block_sum_256(acc, s, tid);
  if (tid == 0) out[0] = total;
}

// grid ceil(M / 4), one wave per row of P: lane l takes entries l, l + 64, ... of the row (column order), the lanes are
// added by a butterfly.  klrow double[M]: the row's share of the KL sum (written only when ERR).
template <bool ERR>
__global__ __launch_bounds__(256) void k_tsne_attraction(const float2* __restrict__ y, int M,
                                                         const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, int nnz, float exaggeration,
                                                         const float* __restrict__ rpart, int S, const double* __restrict__ z,
                                                         float2* __restrict__ grad, double* __restrict__ klrow) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;                                          // wave-uniform; no barrier below
  const float2 yi = y[i];
  const double zz = z[0];
  const int b = min(max(rowptr[i], 0), nnz), e = min(max(rowptr[i + 1], b), nnz);
  float ax = 0.f, ay = 0.f;
  double kl = 0.0;
  for (int t = b + lane; t < e; t += 64) {
    const int j = min(max(col[t], 0), M - 1);
    const float p = val[t];
    const float2 yj = y[j];
    const float dx = yi.x - yj.x, dy = yi.y - yj.y;
    const float q = 1.f / __fadd_rn(1.f, sq_norm(dx, dy));
    const float w = p * q;
    ax = __builtin_fmaf(w, dx, ax);
    ay = __builtin_fmaf(w, dy, ay);
    if (ERR) {
      const float pe = exaggeration * p;
      kl += (double)pe * log((double)fmaxf(pe, FLT_MIN) / fmax((double)q / zz, (double)FLT_MIN));
    }
  }
  ax = wave_sum(ax);
  ay = wave_sum(ay);
  if (ERR) kl = wave_sum(kl);
  float rx = 0.f, ry = 0.f;
  for (int sl = 0; sl < S; ++sl) {
    rx += rpart[(size_t)sl * 2 * M + i];
    ry += rpart[((size_t)sl * 2 + 1) * M + i];
  }
  if (lane == 0) {
    grad[i] = make_float2(4.f * (exaggeration * ax - (float)((double)rx / zz)),
                          4.f * (exaggeration * ay - (float)((double)ry / zz)));
    if (ERR) klrow[i] = kl;
  }
}

// ------------------------------------------------------------------------------------------ update
// one thread per entry of [M, 2]; npart double[gridDim.x]: the workgroup's sum of g^2
__global__ __launch_bounds__(256) void k_tsne_update(const float* __restrict__ grad, int n, float momentum, float lr,
                                                     float min_gain, float* __restrict__ y, float* __restrict__ update,
                                                     float* __restrict__ gains, double* __restrict__ npart) {
  __shared__ double s[256];
  const int tid = threadIdx.x;
  const int e = blockIdx.x * 256 + tid;
  double g2 = 0.0;
  if (e < n) {
    const float gr = grad[e], up = update[e];
    float gain = gains[e];
    gain = (up * gr < 0.f) ? gain + 0.2f : gain * 0.8f;
    gain = fmaxf(gain, min_gain);
    const float g = gr * gain;
    const float nu = momentum * up - lr * g;
    gains[e] = gain;
    update[e] = nu;
    y[e] += nu;
    g2 = (double)g * (double)g;
  }
  const double total = block_sum_256(g2, s, tid);
  if (tid == 0) npart[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------ host side
struct TsnePlan {
  int tiles, tiles_per_slice, slices, upd_blocks;
  size_t o_npart, o_klrow, o_ztile, o_zpart, o_rpart, upd_bytes, bytes;
};

inline bool tsne_shape_ok(int64_t M, int64_t slices) { return M >= 2 && M < kMaxM && slices >= 0; }

inline TsnePlan plan_tsne(int64_t M, int64_t slices) {
  TsnePlan p;
  p.tiles = (int)ceil_div64(M, kTile);
  const rgcn_slicing cut = rgcn_slice_tiles(p.tiles, slices > 0 ? slices : ceil_div64(4 * kCUs, p.tiles), kMaxSlices);
  p.tiles_per_slice = cut.tiles_per_slice;
  p.slices = cut.slices;
  p.upd_blocks = (int)ceil_div64(2 * M, 256);
  size_t at = 0;
  p.o_npart = at; at += align256((size_t)p.upd_blocks * 8);
  p.upd_bytes = at;                                            // what the update alone needs: the same for every slices
  p.o_klrow = at; at += align256((size_t)M * 8);
  p.o_ztile = at; at += align256((size_t)p.tiles * 8);
  p.o_zpart = at; at += align256((size_t)p.slices * M * 8);
  p.o_rpart = at; at += align256((size_t)p.slices * 2 * M * 4);
  p.bytes = at;
  return p;
}

}  // namespace

extern "C" {

int rgcn_knn_refine(const float* x, int64_t M, int64_t d, const int64_t* cand, int64_t k, int32_t* ids, float* sqdist,
                    void* stream_) {
  if (M < 2 || d <= 0 || k < 1) return RGCN_ERR_ARG;
  if (d % 4 || d > (1 << 20) || k > kMaxK || M >= kMaxM) return RGCN_ERR_UNSUPPORTED;
  if (k + 1 > M || !x || !cand || !ids || !sqdist) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, x);                         // rows are read as float4; everything else one element at a time
  RGCN_ALIGN_TRY(8, cand);
  RGCN_ALIGN_TRY(4, ids, sqdist);
  hipStream_t stream = (hipStream_t)stream_;
  k_knn_refine<<<(unsigned)ceil_div64(M, 4), 256, 0, stream>>>(x, (int)M, (int)d, cand, (int)k, ids, sqdist);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

int rgcn_tsne_affinities(const float* sqdist, int64_t M, int64_t k, double perplexity, float* cond_p, float* beta,
                         void* stream_) {
  if (M < 1 || k < 2) return RGCN_ERR_ARG;
  if (k > kMaxK || M >= kMaxM) return RGCN_ERR_UNSUPPORTED;
  if (!(perplexity > 0.0) || !(perplexity < (double)k) || !sqdist || !cond_p || !beta) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(4, sqdist, cond_p, beta);
  hipStream_t stream = (hipStream_t)stream_;
  k_tsne_affinities<<<(unsigned)ceil_div64(M, 4), 256, 0, stream>>>(sqdist, (int)M, (int)k, log(perplexity), cond_p, beta);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

size_t rgcn_tsne_workspace_bytes(int64_t M, int64_t slices) {
  if (!tsne_shape_ok(M, slices)) return 0;
  return plan_tsne(M, slices).bytes;
}

int rgcn_tsne_gradient(const float* y, int64_t M, const int32_t* rowptr, const int32_t* col, const float* val, int64_t nnz,
                       float exaggeration, int64_t slices, int compute_error, float* grad, double* z, double* kl, void* ws,
                       size_t ws_bytes, void* stream_) {
  if (M < 2 || nnz < 0 || slices < 0) return RGCN_ERR_ARG;
  if (M >= kMaxM || nnz >= ((int64_t)1 << 31)) return RGCN_ERR_UNSUPPORTED;
  if (!(exaggeration > 0.f) || !(exaggeration < INFINITY)) return RGCN_ERR_ARG;
  if (!y || !rowptr || !col || !val || !grad || !z || !kl) return RGCN_ERR_ARG;
  const TsnePlan p = plan_tsne(M, slices);
  if (!ws || ws_bytes < p.bytes) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, ws);
  RGCN_ALIGN_TRY(8, y, grad, z, kl);             // the layout and its gradient go as float2 points
  RGCN_ALIGN_TRY(4, rowptr, col, val);
  hipStream_t stream = (hipStream_t)stream_;
  char* w = (char*)ws;
  double* klrow = (double*)(w + p.o_klrow);
  double* ztile = (double*)(w + p.o_ztile);
  double* zpart = (double*)(w + p.o_zpart);
  float* rpart = (float*)(w + p.o_rpart);
  const float2* y2 = reinterpret_cast<const float2*>(y);
  k_tsne_repulsion<<<dim3((unsigned)p.tiles, (unsigned)p.slices), kTile, 0, stream>>>(y2, (int)M, p.tiles_per_slice, zpart, rpart);
  RGCN_HIP_TRY(hipGetLastError());
  k_tsne_z<<<(unsigned)p.tiles, 256, 0, stream>>>(zpart, (int)M, p.slices, ztile);
  RGCN_HIP_TRY(hipGetLastError());
  k_sum_double<<<1, 256, 0, stream>>>(ztile, p.tiles, z);
  RGCN_HIP_TRY(hipGetLastError());
  const unsigned rows = (unsigned)ceil_div64(M, 4);
  if (compute_error) {
    k_tsne_attraction<true><<<rows, 256, 0, stream>>>(y2, (int)M, rowptr, col, val, (int)nnz, exaggeration, rpart, p.slices, z,
                                                      reinterpret_cast<float2*>(grad), klrow);
    RGCN_HIP_TRY(hipGetLastError());
    k_sum_double<<<1, 256, 0, stream>>>(klrow, (int)M, kl);
  } else {
    k_tsne_attraction<false><<<rows, 256, 0, stream>>>(y2, (int)M, rowptr, col, val, (int)nnz, exaggeration, rpart, p.slices, z,
                                                       reinterpret_cast<float2*>(grad), klrow);
  }
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

int rgcn_tsne_update(const float* grad, int64_t M, float momentum, float learning_rate, float min_gain, float* y,
                     float* update, float* gains, double* grad_norm2, void* ws, size_t ws_bytes, void* stream_) {
  if (M < 2) return RGCN_ERR_ARG;
  if (M >= kMaxM) return RGCN_ERR_UNSUPPORTED;
  if (momentum != momentum || learning_rate != learning_rate || min_gain != min_gain) return RGCN_ERR_ARG;
  if (!grad || !y || !update || !gains || !grad_norm2) return RGCN_ERR_ARG;
  const TsnePlan p = plan_tsne(M, 1);
  if (!ws || ws_bytes < p.upd_bytes) return RGCN_ERR_ARG;
  RGCN_ALIGN_TRY(16, ws);
  RGCN_ALIGN_TRY(8, grad_norm2);
  RGCN_ALIGN_TRY(4, grad, y, update, gains);     // one thread per coordinate
  hipStream_t stream = (hipStream_t)stream_;
  double* npart = (double*)((char*)ws + p.o_npart);
  k_tsne_update<<<(unsigned)p.upd_blocks, 256, 0, stream>>>(grad, (int)(2 * M), momentum, learning_rate, min_gain, y, update,
                                                           gains, npart);
  RGCN_HIP_TRY(hipGetLastError());
  k_sum_double<<<1, 256, 0, stream>>>(npart, p.upd_blocks, grad_norm2);
  RGCN_HIP_TRY(hipGetLastError());
  return RGCN_OK;
}

}  // extern "C"
